"""CAM++ (CAMPPlus) on the HIP path against the reference fixtures and tests/campplus_ref.py:
every fixture, tile-tail / segment-boundary shapes, batch invariance, run-to-run bit identity
and the model-directory front door (config.yaml + avg_model.pt -> load_model -> wav)."""
import os
import sys

import numpy as np
import pytest
import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import campplus_ref  # noqa: E402
from oracle import fbank_ref  # noqa: E402
from campplus_cases import FIXTURES, IDS, load_case  # noqa: E402
from wespeaker_hubert_amd import arch as A  # noqa: E402
from wespeaker_hubert_amd.audio import write_wav  # noqa: E402
from wespeaker_hubert_amd.speaker_model import HipSpeakerModel  # noqa: E402
from wespeaker_hubert_amd.synthetic import synth_audio, synth_feats, synth_state_dict  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EMB_ATOL, EMB_COS = 1e-4, 0.9999


def _assert_emb(got, ref):
    assert got.shape == ref.shape
    assert np.all(np.isfinite(got))
    d = np.abs(got - ref).max()
    assert d < EMB_ATOL, f"max |delta| {d}"
    g, r = got.astype(np.float64), ref.astype(np.float64)
    cos = (g * r).sum(1) / np.linalg.norm(g, axis=1) / np.linalg.norm(r, axis=1)
    assert cos.min() >= EMB_COS, cos.min()


_MODELS = {}


def _model(seed, feat_dim=80, embed_dim=512):
    """One device handle per (seed, shape), shared by the tests (weights are never changed)."""
    key = (seed, feat_dim, embed_dim)
    if key not in _MODELS:
        m = HipSpeakerModel("CAMPPlus", feat_dim=feat_dim, embed_dim=embed_dim)
        sd = synth_state_dict(seed, m.state_dict_layout())
        m.load_state_dict(sd)
        m.to(DEV)
        _MODELS[key] = (m, sd)
    return _MODELS[key]


def _embed(m, x):
    out = m(torch.from_numpy(x).to(DEV))
    assert isinstance(out, torch.Tensor)  # CAMPPlus.forward returns the embedding itself
    return out.cpu().numpy()


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_fixture(path):
    z, spec, _, _, x = load_case(path)
    m, _ = _model(int(z["weight_seed"]), spec.feat_dim, spec.embed_dim)
    _assert_emb(_embed(m, x), z["embed"])


# M = B T' rows: 303 (a tile tail, a 1-frame last segment), T' = 200 / 201 (segment boundary), T' = 2
SHAPES = [(3, 201), (2, 399), (2, 401), (4, 3)]
_REF = {}


def _shape_case(B, T):
    if (B, T) not in _REF:
        m, sd = _model(41)
        x = synth_feats(700 + T, B, T, 80)
        _REF[(B, T)] = (x, campplus_ref.forward(x, sd).numpy())
    return _REF[(B, T)]


@pytest.mark.parametrize("B,T", SHAPES)
def test_against_ref(B, T):
    m, _ = _model(41)
    x, ref = _shape_case(B, T)
    _assert_emb(_embed(m, x), ref)


@pytest.mark.parametrize("B,T", SHAPES)
def test_each_utterance_alone_equals_its_batch_row(B, T):
    m, _ = _model(41)
    x, _ = _shape_case(B, T)
    full = _embed(m, x)
    for b in range(B):
        one = _embed(m, x[b:b + 1])
        assert np.abs(one[0] - full[b]).max() <= 1e-5


def test_two_runs_are_bit_identical():
    m, _ = _model(41)
    x, _ = _shape_case(3, 201)
    a, b = _embed(m, x), _embed(m, x)
    assert a.tobytes() == b.tobytes()


def test_batch_wider_than_one_operand_chunk():
    """B = 200 x T = 1000: the stem's output is 10.24 MB per utterance, so the 2 GiB operand cap
    splits the batch into two chunks of 100; utterance b carries features b % 2, so every row must
    equal the B = 2 run's row b % 2 (each utterance's result is independent of its batch)."""
    m, _ = _model(41)
    two = synth_feats(801, 2, 1000, 80)
    small = _embed(m, two)
    big = m(torch.from_numpy(two).to(DEV).repeat(100, 1, 1)).cpu().numpy()
    assert big.shape == (200, 512) and np.isfinite(big).all()
    assert np.abs(big - np.tile(small, (100, 1))).max() <= 1e-5


def test_unfused_option_computes_the_same():
    """cam_fused = 0 (the BN-ReLU as a pass of its own, A/B runs only) rounds the same f32 fma
    before the same split: bit-identical embeddings."""
    m, _ = _model(41)
    x, _ = _shape_case(2, 401)
    a = _embed(m, x)
    m.set_option("cam_fused", 0)
    try:
        b = _embed(m, x)
    finally:
        m.set_option("cam_fused", 1)
    assert a.tobytes() == b.tobytes()


def test_too_short_and_profile_classes():
    m, _ = _model(41)
    with pytest.raises(RuntimeError, match="3 frames"):
        m.embed(torch.zeros(1, 2, 80, device=DEV))
    x, _ = _shape_case(2, 399)
    m.profile(True)
    try:
        _embed(m, x)
    finally:
        m.profile(False)
    n = {k: m.profile_query(k)[0] for k in ("stem", "fcm_strided", "fcm_conv3x3", "cam_tdnn", "cam_gemm", "cam_mask",
                                            "cam_local", "cam_transit", "tstp_head")}
    assert n == {"stem": 1, "fcm_strided": 3, "fcm_conv3x3": 6, "cam_tdnn": 1, "cam_gemm": 52, "cam_mask": 52,
                 "cam_local": 52, "cam_transit": 3, "tstp_head": 1}


def test_front_door_model_dir_to_embedding(tmp_path):
    import wespeaker_hubert_amd as wespeaker
    from wespeaker_hubert_amd.cli.speaker import load_model_pt
    spec = A.make_spec("CAMPPlus", feat_dim=80, embed_dim=192)
    sd = synth_state_dict(45, A.param_list(spec))
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, tmp_path / "avg_model.pt")
    with open(tmp_path / "config.yaml", "w") as f:  # the hub's campplus model_args
        yaml.safe_dump({"model": "CAMPPlus", "model_args": {"feat_dim": 80, "embed_dim": 192, "pooling_func": "TSTP"},
                        "dataset_args": {"fbank_args": {"num_mel_bins": 80, "frame_shift": 10, "frame_length": 25}}}, f)
    m = load_model_pt(str(tmp_path))
    assert isinstance(m, HipSpeakerModel) and m.spec.family == "campplus"
    pcm = synth_audio(46, 1, 24011)[0]
    write_wav(str(tmp_path / "u.wav"), pcm)
    spk = wespeaker.load_model(str(tmp_path))
    got = spk.extract_embedding(str(tmp_path / "u.wav")).numpy()[None]
    feats = fbank_ref.fbank(pcm, cmn=True)[None]
    _assert_emb(got, campplus_ref.forward(feats, sd).numpy())
