"""The x-vector TDNN (XVEC, XI_VEC_XVEC) and the XI-pooled ECAPA (XI_VEC_ECAPA_TDNN_c512 / c1024) on the
HIP path against the reference fixtures and tests/xvec_ref.py in float64: every fixture, synthetic
shapes, batch invariance, run-to-run bit identity, ragged batches against batch-of-one results, the
refusal of inputs too short to pool, the profile classes and the front door (config.yaml +
avg_model.pt -> load_model -> wav, bin/extract).

Measured on an MI355X, max |delta| against the fixtures (bar 1e-4; the two x 8 fixtures 1e-4 x rms of
the reference embedding, 1.04e-4 and 4.9e-4): XVEC 1.5e-6 (T = 200), 1.7e-6 (T = 37), 4.6e-6 (F = 40, T = 16);
XI_VEC_XVEC 1.7e-6 (T = 200), 2.6e-6 (T = 15), x 8 2.0e-5; XI_VEC_ECAPA_TDNN_c512 6.4e-6 (T = 200),
5.3e-6 (emb_bn, T = 33), x 8 1.1e-4; c1024 4.7e-6; the xvec_ref float64 shapes <= 6.9e-6.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import xvec_ref  # noqa: E402
from oracle import fbank_ref  # noqa: E402
from xvec_cases import FIXTURES, IDS, SEED, load_case, synth_case  # noqa: E402
from wespeaker_hubert_amd.audio import write_wav  # noqa: E402
from wespeaker_hubert_amd.kaldi_io import load_scp_sequential  # noqa: E402
from wespeaker_hubert_amd.speaker_model import HipSpeakerModel  # noqa: E402
from wespeaker_hubert_amd.synthetic import synth_audio, synth_feats, synth_state_dict  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EMB_ATOL, EMB_COS = 1e-4, 0.9999
XV, XIV, XE512, XE1024 = "XVEC", "XI_VEC_XVEC", "XI_VEC_ECAPA_TDNN_c512", "XI_VEC_ECAPA_TDNN_c1024"


def _assert_emb(got, ref, atol=EMB_ATOL):
    assert got.shape == ref.shape
    assert np.all(np.isfinite(got))
    d = np.abs(got - ref).max()
    print(f"max |delta| {d:.3e} (bar {atol:.3e})")
    assert d < atol, f"max |delta| {d}"
    g, r = got.astype(np.float64), ref.astype(np.float64)
    cos = (g * r).sum(1) / np.linalg.norm(g, axis=1) / np.linalg.norm(r, axis=1)
    assert cos.min() >= EMB_COS, cos.min()


_MODELS = {}


def _model(arch, feat_dim=80, embed_dim=None, emb_bn=False):
    """One device handle per (arch, dims), shared by the tests (weights are never changed)."""
    embed_dim = embed_dim or (192 if "ECAPA" in arch else 512)
    key = (arch, feat_dim, embed_dim, emb_bn)
    if key not in _MODELS:
        kw = {"emb_bn": True} if emb_bn else {}
        m = HipSpeakerModel(arch, feat_dim=feat_dim, embed_dim=embed_dim, **kw)
        sd = synth_state_dict(SEED, m.state_dict_layout())
        m.load_state_dict(sd)
        m.to(DEV)
        _MODELS[key] = (m, sd)
    return _MODELS[key]


def _embed(m, x):
    out = m(torch.from_numpy(x).to(DEV))
    assert isinstance(out, tuple) and len(out) == 2 and out[0] is None  # (aux, embed): outputs[-1] is the embedding
    return out[1].cpu().numpy()


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_fixture(path):
    """Unscaled fixtures: the project's bars (per-dim 1e-4, cosine 0.9999) on O(1) embeddings.  The
    x 8 fixtures (embeddings up to 3.4 and 15): 1e-4 x rms of the reference embedding, as the ERes2Net
    x 8 fixtures."""
    z, spec, _, _, x = load_case(path)
    m, _ = _model(spec.arch, spec.feat_dim, spec.embed_dim, spec.emb_bn)
    ref = z["embed"]
    atol = EMB_ATOL
    if float(z["input_scale"]) != 1.0:
        atol = 1e-4 * float(np.sqrt((ref.astype(np.float64) ** 2).mean()))
    _assert_emb(_embed(m, x), ref, atol)


# XVEC: T' = 2 with a 3-utterance batch, odd T, more than one row block, the long recipe length;
# XI_VEC_XVEC at T' = 1; XI-ECAPA at the ECAPA path's own minimum, odd T, and T = 300 (gate_fold)
SHAPES = [(XV, 3, 16), (XV, 2, 37), (XV, 4, 143), (XV, 1, 498), (XIV, 3, 15), (XE512, 2, 1), (XE512, 3, 37), (XE512, 1, 300)]
SHAPE_IDS = [f"{a}-b{b}-t{t}" for a, b, t in SHAPES]
_REF = {}


def _shape_case(arch, B, T):
    key = (arch, B, T)
    if key not in _REF:
        m, sd = _model(arch)
        x = synth_feats(1000 + 7 * B + T, B, T, 80)
        ref = xvec_ref.forward(x, sd, arch, m.spec.pooling_func, dtype=torch.float64).numpy().astype(np.float32)
        _REF[key] = (x, ref)
    return _REF[key]


@pytest.mark.parametrize("arch,B,T", SHAPES, ids=SHAPE_IDS)
def test_against_ref(arch, B, T):
    m, _ = _model(arch)
    x, ref = _shape_case(arch, B, T)
    _assert_emb(_embed(m, x), ref)


@pytest.mark.parametrize("arch,B,T", [s for s in SHAPES if s[1] > 1], ids=[i for s, i in zip(SHAPES, SHAPE_IDS) if s[1] > 1])
def test_each_utterance_alone_equals_its_batch_row(arch, B, T):
    m, _ = _model(arch)
    x, _ = _shape_case(arch, B, T)
    full = _embed(m, x)
    for b in range(B):
        assert np.array_equal(_embed(m, x[b:b + 1])[0], full[b]), b


@pytest.mark.parametrize("arch,B,T", [(XV, 2, 37), (XIV, 3, 15), (XE512, 3, 37)])
def test_two_runs_are_bit_identical(arch, B, T):
    m, _ = _model(arch)
    x, _ = _shape_case(arch, B, T)
    a, b = _embed(m, x), _embed(m, x)
    assert a.tobytes() == b.tobytes()


RAGGED = [(XV, [16, 17, 47, 200, 31, 498]), (XIV, [15, 16, 47, 200, 31, 498]), (XE512, [1, 7, 200, 33, 301])]


@pytest.mark.parametrize("arch,lens", RAGGED, ids=[a for a, _ in RAGGED])
def test_ragged_batch_equals_batch_of_one(arch, lens):
    """embed_segments row b == embed(utterance b alone), bit for bit: the unpadded convs of the TDNN
    take the per-layer offset tables (off[b] - b x {4, 8, 14}), so no utterance reads another's rows."""
    m, _ = _model(arch)
    utts = [synth_feats(2000 + i, 1, n, 80)[0] for i, n in enumerate(lens)]
    feats = torch.from_numpy(np.concatenate(utts)).to(DEV)
    off = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device=DEV)
    got = m.embed_segments(feats, off).cpu().numpy()
    assert got.shape == (len(lens), m.spec.embed_dim) and np.isfinite(got).all()
    for b, u in enumerate(utts):
        assert np.array_equal(_embed(m, u[None])[0], got[b]), (b, lens[b])


@pytest.mark.parametrize("arch,T,need", [(XV, 14, 16), (XV, 15, 16), (XIV, 14, 15)])
def test_too_short_input_is_refused(arch, T, need):
    m, _ = _model(arch)
    with pytest.raises(RuntimeError, match=f">= {need} frames"):
        m.embed(torch.zeros(2, T, 80, device=DEV))
    with pytest.raises(RuntimeError, match=f">= {need} frames"):
        m.embed_segments(torch.zeros(T + 40, 80, device=DEV), torch.tensor([0, 40, T + 40], dtype=torch.int32, device=DEV))
    x, ref = _shape_case(arch, 3, need)  # the handle stays usable
    _assert_emb(_embed(m, x), ref)


def _launches(m, x, tags):
    m.profile(True)
    try:
        _embed(m, x)
    finally:
        m.profile(False)
    return {k: m.profile_query(k)[0] for k in tags}


def test_profile_classes():
    tags = ("tdnn_k5", "tdnn_k3", "tdnn_1x1", "tstp", "xi_lin1", "xi_lin2", "xi_pool", "head")
    m, _ = _model(XV)
    assert _launches(m, _shape_case(XV, 2, 37)[0], tags) == {
        "tdnn_k5": 1, "tdnn_k3": 2, "tdnn_1x1": 2, "tstp": 1, "xi_lin1": 0, "xi_lin2": 0, "xi_pool": 0, "head": 1}
    m, _ = _model(XIV)
    assert _launches(m, _shape_case(XIV, 3, 15)[0], tags) == {
        "tdnn_k5": 1, "tdnn_k3": 2, "tdnn_1x1": 2, "tstp": 0, "xi_lin1": 1, "xi_lin2": 1, "xi_pool": 1, "head": 1}
    m, _ = _model(XE512)
    got = _launches(m, _shape_case(XE512, 3, 37)[0], ("conv_cat", "xi_lin1", "xi_lin2", "xi_pool", "astp", "pool_linear1", "head"))
    assert got == {"conv_cat": 1, "xi_lin1": 1, "xi_lin2": 1, "xi_pool": 1, "astp": 0, "pool_linear1": 0, "head": 1}


FRONT = [(XV, {"feat_dim": 80, "embed_dim": 512, "pooling_func": "TSTP"}),
         (XE512, {"feat_dim": 80, "embed_dim": 192, "pooling_func": "XI"})]


@pytest.mark.parametrize("arch,margs", FRONT, ids=[a for a, _ in FRONT])
def test_front_door_model_dir_to_embedding(tmp_path, arch, margs):
    """config.yaml with the recipe's model_args (xvec.yaml, xi_vector.yaml) + avg_model.pt ->
    load_model -> extract_embedding(wav), and bin/extract.py with batch size 1 on three short wavs
    (the ragged route), against fbank_ref + xvec_ref."""
    import wespeaker_hubert_amd as wespeaker
    from wespeaker_hubert_amd.bin.extract import extract
    from wespeaker_hubert_amd.cli.speaker import load_model_pt
    _, _, sd, _ = synth_case(arch, 89, 0, 1, 16, 80, margs["embed_dim"])
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, tmp_path / "avg_model.pt")
    with open(tmp_path / "config.yaml", "w") as f:
        yaml.safe_dump({"model": arch, "model_args": margs,
                        "dataset_args": {"frontend": "fbank", "resample_rate": 16000, "num_frms": 200,
                                         "fbank_args": {"num_mel_bins": 80, "frame_shift": 10, "frame_length": 25}}}, f)
    m = load_model_pt(str(tmp_path))
    assert isinstance(m, HipSpeakerModel) and m.supports_segments
    pcms = {f"u{i}": synth_audio(56 + i, 1, n)[0] for i, n in enumerate((8801, 12000, 16160))}
    refs = {k: xvec_ref.forward(fbank_ref.fbank(p, cmn=True)[None], sd, arch, margs["pooling_func"])[0].numpy()
            for k, p in pcms.items()}
    for k, p in pcms.items():
        write_wav(str(tmp_path / f"{k}.wav"), p)
    spk = wespeaker.load_model(str(tmp_path))
    got = spk.extract_embedding(str(tmp_path / "u1.wav")).numpy()[None]
    _assert_emb(got, refs["u1"][None])
    with open(tmp_path / "raw.list", "w") as f:
        for k in pcms:
            f.write(json.dumps({"key": k, "wav": str(tmp_path / f"{k}.wav"), "spk": "s0"}) + "\n")
    scp = extract(config=str(tmp_path / "config.yaml"), model_path=str(tmp_path / "avg_model.pt"), data_type="raw",
                  data_list=str(tmp_path / "raw.list"), embed_ark=str(tmp_path / "xvector.ark"), batch_size=1,
                  num_workers=1)
    rows = dict(load_scp_sequential(scp))
    assert sorted(rows) == sorted(pcms)
    for k, e in rows.items():
        _assert_emb(e[None], refs[k][None])
