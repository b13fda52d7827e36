"""GPU: the SE-Res2Block seam folded into the next block's conv1 (option seam_fold, default on).

The first two blocks used to end with a pass x_{L+1} = x_L + g (.) h3 of their own.  With
seam_fold the next block's conv1 forms that sum while it stages its A operand — fma(h3, g, x),
the rounding the pass produced — splits it once into bf16 hi / lo, and stores it on the way for
its later readers.  Same split, same MFMA order, same epilogue: the embeddings must equal
seam_fold 0 bit for bit, and stay within test_gpu_gate_fold.py's bars of the oracle (1e-4 /
cos 0.9999).

Shapes as test_gpu_gate_fold.py: B = 3 x T = 300 puts a 256-row tile across utterances 0 / 1
and leaves a partial last tile; 1 x 256 keeps a tile inside one utterance; 2 x 257 puts the
boundary one row into a tile; c1024 at 2 x 300 runs four column tiles per row tile (each stores
a quarter of the sum's k-tiles).  Ragged batches, T < 256 and precision 0 keep the pass.  The
profile tags show the route: `seam` counts the fused launches, `se.scale` the block outputs that
get materialised (2 with gate_fold, 3 without — whichever kernel stores them).
tools/gemm_check's case seam compares the kernel's stored sum with residual_scale<true> and its
GEMM output with family 7 on that sum at M = 3 x 300, N = K = 512 and 1024, guard rows intact."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from oracle import models_ref
from wespeaker_hubert_amd.synthetic import synth_feats, synth_state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEMM_CHECK = os.path.join(ROOT, "tools", "gemm_check")

_models = {}


def _model(arch):
    """One handle per architecture (seam_fold is a run-time option) and its state dict."""
    if arch not in _models:
        from wespeaker_hubert_amd.speaker_model import HipSpeakerModel
        m = HipSpeakerModel(arch, feat_dim=80, embed_dim=192)
        sd = synth_state_dict(47, m.state_dict_layout())
        m.load_state_dict(sd)
        m.to(DEV)
        assert (m.get_option("seam_fold"), m.get_option("gate_fold")) == (1, 1)  # the defaults
        _models[arch] = (m, sd)
    return _models[arch]


def _run(m, seam, fn, gate_fold=1):
    """fn() with seam_fold = seam under profiling -> (embeddings, seam launches, se.scale launches)."""
    m.set_option("seam_fold", seam)
    m.set_option("gate_fold", gate_fold)
    assert m.get_option("seam_fold") == seam
    m.profile(True)
    try:
        out = fn().cpu().numpy()
        torch.cuda.synchronize()
        ns, _, _ = m.profile_query("seam")
        nr, _, _ = m.profile_query("se.scale")
    finally:
        m.profile(False)
        m.set_option("seam_fold", 1)
        m.set_option("gate_fold", 1)
    return out, ns, nr


@pytest.mark.parametrize("arch,B,T", [("ECAPA_TDNN_c512", 3, 300), ("ECAPA_TDNN_c512", 1, 256),
                                      ("ECAPA_TDNN_c512", 2, 257), ("ECAPA_TDNN_c1024", 2, 300)])
def test_seam_fold_equals_residual_pass_and_oracle(arch, B, T):
    m, sd = _model(arch)
    m.set_option("precision", 1)
    x = torch.from_numpy(synth_feats(9, B, T, 80)).to(DEV)
    a, sa, ra = _run(m, 1, lambda: m.embed(x))
    b, sb, rb = _run(m, 0, lambda: m.embed(x))
    assert (sa, sb) == (2, 0)  # both seams fused / none
    assert (ra, rb) == (2, 2)  # the same two block outputs are stored either way
    c, sc, rc = _run(m, 1, lambda: m.embed(x), gate_fold=0)
    assert (sc, rc) == (2, 3)  # gate_fold 0: the last block's gate pass is back
    assert np.all(np.isfinite(a))
    assert np.array_equal(a, b)
    assert np.array_equal(a, c)
    with torch.no_grad():
        _, ref = models_ref.forward(arch, x.cpu(), {k: torch.from_numpy(v) for k, v in sd.items()})
    ref = ref.numpy()
    print("max |emb - oracle|", np.abs(a - ref).max())
    assert np.abs(a - ref).max() < 1e-4
    cos = (a * ref).sum(1) / np.linalg.norm(a, axis=1) / np.linalg.norm(ref, axis=1)
    assert cos.min() >= 0.9999


def test_seam_fold_ragged_falls_back():
    m, _ = _model("ECAPA_TDNN_c512")
    m.set_option("precision", 1)
    frames = [300, 120, 257]
    feats = np.concatenate([synth_feats(800 + i, 1, t, 80)[0] for i, t in enumerate(frames)])
    cat = torch.from_numpy(feats).to(DEV)
    off = torch.tensor(np.concatenate([[0], np.cumsum(frames)]), dtype=torch.int32, device=DEV)
    a, sa, ra = _run(m, 1, lambda: m.embed_segments(cat, off))
    b, sb, rb = _run(m, 0, lambda: m.embed_segments(cat, off))
    assert (sa, sb) == (0, 0) and (ra, rb) == (3, 3)  # every pass stays
    assert np.all(np.isfinite(a)) and np.array_equal(a, b)


@pytest.mark.parametrize("T,precision", [(200, 1), (300, 0)])
def test_seam_fold_short_and_f32_fall_back(T, precision):
    m, _ = _model("ECAPA_TDNN_c512")
    m.set_option("precision", precision)
    x = torch.from_numpy(synth_feats(10, 2, T, 80)).to(DEV)
    try:
        a, sa, ra = _run(m, 1, lambda: m.embed(x))
        b, sb, rb = _run(m, 0, lambda: m.embed(x))
    finally:
        m.set_option("precision", 1)
    assert (sa, sb) == (0, 0) and (ra, rb) == (3, 3)  # every pass stays
    assert np.all(np.isfinite(a)) and np.array_equal(a, b)


def test_gemm_check_seam():
    if not os.path.exists(GEMM_CHECK):
        pytest.fail(f"{GEMM_CHECK} not built (run __graft_entry__.build())")
    p = subprocess.run([GEMM_CHECK, "seam", "1"], capture_output=True, text=True, timeout=120)
    out = p.stdout + p.stderr
    assert p.returncode == 0, out
    sums = re.findall(r"seam C=(\d+) (\S+) sum vs residual_scale<true>: (\d+) of (\d+) words differ, "
                      r"(\d+) of (\d+) guard words touched", out)
    gemms = re.findall(r"seam C=(\d+) (\S+) GEMM vs family 7 on the stored sum: (\d+) of (\d+) outputs differ", out)
    forms = [(str(C), f) for C in (512, 1024) for f in ("balanced", "first-block")]
    assert [(c, f) for c, f, *_ in sums] == forms and [(c, f) for c, f, *_ in gemms] == forms, out
    for c, _, d, n, dg, ng in sums:
        assert (d, dg) == ("0", "0") and int(n) == 900 * int(c) and int(ng) == 8 * int(c), out
    for c, _, d, n in gemms:
        assert d == "0" and int(n) == 900 * int(c), out
    assert "all families bit-identical" in out
