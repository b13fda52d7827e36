"""Gemini DF-ResNet (60 / 114 / 183 / 237) on the HIP path against the reference fixtures and
tests/gemini_ref.py: every fixture (114 and 60 under both ib_fused routes), tile-tail shapes, batch
invariance, run-to-run bit identity, a batch wider than one operand chunk, the refusal of inputs
too short to pool, the profile classes and the front door (config.yaml + avg_model.pt ->
load_model -> wav, bin/extract).

Measured on an MI355X, max |delta| against the fixtures (bar 1e-4), default route: 114 3.6e-6,
183 5.9e-6, 237 8.9e-6, 60 (F = 16, T = 3) 2.2e-6, 60 with two_emb_layer 1.6e-6, 60 (T = 37) 1.9e-6;
with ib_fused = 1: 114 3.6e-6, 60 (T = 37) 1.8e-6; the gemini_ref shapes <= 1.1e-5 (237 at T = 3).
"""
import json
import os
import sys

import numpy as np
import pytest
import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gemini_ref  # noqa: E402
from oracle import fbank_ref  # noqa: E402
from gemini_cases import FIXTURES, IDS, load_case, synth_case  # noqa: E402
from wespeaker_hubert_amd.audio import write_wav  # noqa: E402
from wespeaker_hubert_amd.kaldi_io import load_scp_sequential  # noqa: E402
from wespeaker_hubert_amd.speaker_model import HipSpeakerModel  # noqa: E402
from wespeaker_hubert_amd.synthetic import synth_audio, synth_feats, synth_state_dict  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EMB_ATOL, EMB_COS = 1e-4, 0.9999
SEED = 71  # every fixture's weight seed
G60, G237 = "Gemini_DF_ResNet60", "Gemini_DF_ResNet237"


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


def _model(arch, feat_dim=80, embed_dim=256, two_emb=False):
    """One device handle per (arch, dims), shared by the tests (weights are never changed; a test
    that sets ib_fused puts the default back)."""
    key = (arch, feat_dim, embed_dim, two_emb)
    if key not in _MODELS:
        m = HipSpeakerModel(arch, feat_dim=feat_dim, embed_dim=embed_dim, two_emb_layer=two_emb)
        sd = synth_state_dict(SEED, m.state_dict_layout(), residual_tame=True)
        m.load_state_dict(sd)
        m.to(DEV)
        _MODELS[key] = (m, sd, m.get_option("ib_fused"))
    return _MODELS[key]


def _embed(m, x):
    out = m(torch.from_numpy(x).to(DEV))
    assert isinstance(out, tuple) and len(out) == 2 and out[0] is None  # (aux, embed), as the ResNet path
    return out[1].cpu().numpy()


def _with_route(m, default, fused, fn):
    m.set_option("ib_fused", fused)
    try:
        return fn()
    finally:
        m.set_option("ib_fused", default)


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_fixture(path):
    """The project's bars (per-dim 1e-4, cosine 0.9999) on O(1) embeddings, default route."""
    z, spec, _, _, x = load_case(path)
    assert int(z["weight_seed"]) == SEED
    m, _, _ = _model(spec.arch, spec.feat_dim, spec.embed_dim, spec.two_emb_layer)
    _assert_emb(_embed(m, x), z["embed"])


BOTH = [p for p in FIXTURES if os.path.basename(p).startswith(("gemini114_", "gemini60_f80"))]


@pytest.mark.parametrize("fused", (0, 1))
@pytest.mark.parametrize("path", BOTH, ids=[os.path.basename(p)[:-4] for p in BOTH])
def test_fixture_under_both_routes(path, fused):
    z, spec, _, _, x = load_case(path)
    m, _, default = _model(spec.arch, spec.feat_dim, spec.embed_dim)
    _assert_emb(_with_route(m, default, fused, lambda: _embed(m, x)), z["embed"])


# Gemini60 (embed 256): T' = 2 with a 3-utterance batch, T odd (37 -> 19), T' = 5, the recipe
# length; 237 at the shortest input
SHAPES = [(G60, 3, 3), (G60, 2, 37), (G60, 4, 10), (G60, 1, 200), (G237, 1, 3)]
SHAPE_IDS = [f"{a[-3:].lstrip('t')}-b{b}-t{t}" for a, b, t in SHAPES]
_REF = {}


def _shape_case(arch, B, T):
    key = (arch, B, T)
    if key not in _REF:
        _, sd, _ = _model(arch)
        x = synth_feats(900 + T, B, T, 80)
        _REF[key] = (x, gemini_ref.forward(x, sd, arch).numpy())
    return _REF[key]


@pytest.mark.parametrize("arch,B,T", SHAPES, ids=SHAPE_IDS)
def test_against_ref(arch, B, T):
    m, _, _ = _model(arch)
    x, ref = _shape_case(arch, B, T)
    _assert_emb(_embed(m, x), ref)


@pytest.mark.parametrize("arch,B,T", [s for s in SHAPES if s[1] > 1], ids=[i for s, i in zip(SHAPES, SHAPE_IDS) if s[1] > 1])
def test_each_utterance_alone_equals_its_batch_row(arch, B, T):
    m, _, _ = _model(arch)
    x, _ = _shape_case(arch, B, T)
    full = _embed(m, x)
    for b in range(B):
        one = _embed(m, x[b:b + 1])
        assert np.abs(one[0] - full[b]).max() <= 1e-5


def test_two_runs_are_bit_identical():
    m, _, _ = _model(G60)
    x, _ = _shape_case(G60, 2, 37)
    a, b = _embed(m, x), _embed(m, x)
    assert a.tobytes() == b.tobytes()


def test_batch_wider_than_one_operand_chunk():
    """Gemini60, B = 128 x T = 1000: the 4d-wide tensor of level 1 is 20.5 MB per utterance, so the
    2 GiB operand cap splits the batch into two chunks of 64; utterance b carries features b % 2, so
    every row must equal the B = 2 run's row b % 2 (each utterance's result is independent of its
    batch)."""
    m, _, _ = _model(G60)
    two = synth_feats(801, 2, 1000, 80)
    small = _embed(m, two)
    big = m.embed(torch.from_numpy(two).to(DEV).repeat(64, 1, 1)).cpu().numpy()
    assert big.shape == (128, 256) and np.isfinite(big).all()
    assert np.abs(big - np.tile(small, (64, 1))).max() <= 1e-5


def test_too_short_input_is_refused():
    m, _, _ = _model(G60)
    with pytest.raises(RuntimeError, match="3 frames"):
        m.embed(torch.zeros(1, 2, 80, device=DEV))


TAGS = ("stem", "gem_down", "gem_pw1", "gem_dw", "gem_pw2", "gem_tail", "tstp_head")


def _launches(m, x):
    m.profile(True)
    try:
        _embed(m, x)
    finally:
        m.profile(False)
    return {k: m.profile_query(k)[0] for k in TAGS}


def test_profile_classes():
    """Gemini60 has 3 + 3 + 9 + 3 = 18 inverted bottlenecks and four downsample convs: the fused
    route is conv1 + tail per block, the three-launch route conv1 + depthwise conv + conv3."""
    m, _, default = _model(G60)
    x, _ = _shape_case(G60, 2, 37)
    assert _with_route(m, default, 1, lambda: _launches(m, x)) == {
        "stem": 1, "gem_down": 4, "gem_pw1": 18, "gem_dw": 0, "gem_pw2": 0, "gem_tail": 18, "tstp_head": 1}
    assert _with_route(m, default, 0, lambda: _launches(m, x)) == {
        "stem": 1, "gem_down": 4, "gem_pw1": 18, "gem_dw": 18, "gem_pw2": 18, "gem_tail": 0, "tstp_head": 1}


def test_front_door_model_dir_to_embedding(tmp_path):
    """config.yaml with the recipe's model_args (gemini_dfresnet_adam.yaml) + avg_model.pt ->
    load_model -> extract_embedding(wav), and bin/extract.py on three short wavs, against
    fbank_ref + gemini_ref."""
    import wespeaker_hubert_amd as wespeaker
    from wespeaker_hubert_amd.bin.extract import extract
    from wespeaker_hubert_amd.cli.speaker import load_model_pt
    arch = "Gemini_DF_ResNet114"
    _, _, sd, _ = synth_case(arch, 79, 0, 1, 3, 80, 256)
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, tmp_path / "avg_model.pt")
    with open(tmp_path / "config.yaml", "w") as f:
        yaml.safe_dump({"model": arch,
                        "model_args": {"feat_dim": 80, "embed_dim": 256, "pooling_func": "TSTP", "two_emb_layer": False},
                        "dataset_args": {"frontend": "fbank", "resample_rate": 16000, "num_frms": 200,
                                         "fbank_args": {"num_mel_bins": 80, "frame_shift": 10, "frame_length": 25}}}, f)
    m = load_model_pt(str(tmp_path))
    assert isinstance(m, HipSpeakerModel) and m.spec.family == "gemini"
    pcms = {f"u{i}": synth_audio(46 + i, 1, n)[0] for i, n in enumerate((8801, 12000, 16160))}
    refs = {k: gemini_ref.forward(fbank_ref.fbank(p, cmn=True)[None], sd, arch)[0].numpy() for k, p in pcms.items()}
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
