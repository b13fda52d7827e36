"""GPU: the last SE gate folded into conv_cat's A fragments (option gate_fold, default on).

With cat_gate the last SE_Res2Block used to store d4 = g4 * h3 and conv_cat read it back as
its third A segment.  With gate_fold conv_cat reads h3 itself and multiplies by the gate row
of each frame's utterance while it splits its A fragments: the same fp32 product, the same
split, the same MFMA order, so the embeddings must equal gate_fold 0 bit for bit, and stay
within test_gpu_catgate.py's bars of the oracle (1e-4 / cos 0.9999).

Shapes: B = 3 x T = 300 puts a 256-row tile across utterances 0 / 1 and leaves a partial last
tile; B = 1 x 256 keeps a tile inside one utterance; B = 2 x 257 puts the boundary one row
into a tile.  Ragged batches, T < 256 and precision 0 keep the gate pass: the profile counter
of its launch (tag se.scale) shows the route, and the results equal gate_fold 0 bit for bit.
tools/gemm_check's case gate_seg compares the gated kernel instance with residual_scale<false>
followed by the ungated instance at M = 3 x 300, N = 1536, K = 3 x 512."""
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
    """One handle per architecture (gate_fold is a run-time option) and its state dict."""
    if arch not in _models:
        from wespeaker_hubert_amd.speaker_model import HipSpeakerModel
        m = HipSpeakerModel(arch, feat_dim=80, embed_dim=192)
        sd = synth_state_dict(43, m.state_dict_layout())
        m.load_state_dict(sd)
        m.to(DEV)
        assert (m.get_option("cat_gate"), m.get_option("gate_fold")) == (1, 1)  # the defaults
        _models[arch] = (m, sd)
    return _models[arch]


def _run(m, fold, fn):
    """fn() with gate_fold = fold under profiling -> (embeddings, gate-pass launches)."""
    m.set_option("gate_fold", fold)
    assert m.get_option("gate_fold") == fold
    m.profile(True)
    out = fn().cpu().numpy()
    torch.cuda.synchronize()
    n, _, _ = m.profile_query("se.scale")
    m.profile(False)
    return out, n


@pytest.mark.parametrize("arch,B,T", [("ECAPA_TDNN_c512", 3, 300), ("ECAPA_TDNN_c512", 1, 256),
                                      ("ECAPA_TDNN_c512", 2, 257), ("ECAPA_TDNN_c1024", 2, 300)])
def test_gate_fold_equals_gate_pass_and_oracle(arch, B, T):
    m, sd = _model(arch)
    m.set_option("precision", 1)
    x = torch.from_numpy(synth_feats(9, B, T, 80)).to(DEV)
    a, na = _run(m, 1, lambda: m.embed(x))
    b, nb = _run(m, 0, lambda: m.embed(x))
    assert (na, nb) == (2, 3)  # folded: the last block's gate pass is gone
    assert np.all(np.isfinite(a))
    assert np.array_equal(a, b)
    with torch.no_grad():
        _, ref = models_ref.forward(arch, x.cpu(), {k: torch.from_numpy(v) for k, v in sd.items()})
    ref = ref.numpy()
    print("max |emb - oracle|", np.abs(a - ref).max())
    assert np.abs(a - ref).max() < 1e-4
    cos = (a * ref).sum(1) / np.linalg.norm(a, axis=1) / np.linalg.norm(ref, axis=1)
    assert cos.min() >= 0.9999


def test_gate_fold_ragged_falls_back():
    m, _ = _model("ECAPA_TDNN_c512")
    m.set_option("precision", 1)
    frames = [300, 120, 257]
    feats = np.concatenate([synth_feats(800 + i, 1, t, 80)[0] for i, t in enumerate(frames)])
    cat = torch.from_numpy(feats).to(DEV)
    off = torch.tensor(np.concatenate([[0], np.cumsum(frames)]), dtype=torch.int32, device=DEV)
    a, na = _run(m, 1, lambda: m.embed_segments(cat, off))
    b, nb = _run(m, 0, lambda: m.embed_segments(cat, off))
    assert (na, nb) == (3, 3)  # the gate pass stays
    assert np.all(np.isfinite(a)) and np.array_equal(a, b)


@pytest.mark.parametrize("T,precision", [(200, 1), (300, 0)])
def test_gate_fold_short_and_f32_fall_back(T, precision):
    m, _ = _model("ECAPA_TDNN_c512")
    m.set_option("precision", precision)
    x = torch.from_numpy(synth_feats(10, 2, T, 80)).to(DEV)
    try:
        a, na = _run(m, 1, lambda: m.embed(x))
        b, nb = _run(m, 0, lambda: m.embed(x))
    finally:
        m.set_option("precision", 1)
    assert (na, nb) == (3, 3)  # the gate pass stays
    assert np.all(np.isfinite(a)) and np.array_equal(a, b)


def test_gemm_check_gate_seg():
    if not os.path.exists(GEMM_CHECK):
        pytest.fail(f"{GEMM_CHECK} not built (run __graft_entry__.build())")
    p = subprocess.run([GEMM_CHECK, "gate_seg", "1"], capture_output=True, text=True, timeout=120)
    out = p.stdout + p.stderr
    assert p.returncode == 0, out
    m = re.search(r"family 7 gated vs residual_scale \+ family 7: (\d+) of (\d+) outputs differ", out)
    assert m and m.group(1) == "0" and int(m.group(2)) == 900 * 1536, out
    assert "all families bit-identical" in out
