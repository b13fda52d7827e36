"""Res2Net (Res2Net34_Base, Res2Net34_Large) on the HIP path against the reference fixtures and
tests/res2net_ref.py, under both schedules of the block tail (option res2_tail: 2 = the fused tail in
every stage, 0 = 3x3 conv + conv3 over the concatenated operand): every fixture (the two x 8 ones
drive activations into the clamp), tile-tail shapes, batch invariance, run-to-run bit identity, the
refusal of T = 8, the profile classes and the front door (config.yaml + avg_model.pt -> load_model ->
wav, bin/extract).  The operand-chunk path (B = 128 x T = 1000) is too slow for this suite: the chunk
rule is checked through the workspace query in tests/test_res2net_cpu.py."""
import json
import os
import sys

import numpy as np
import pytest
import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import res2net_ref  # noqa: E402
from oracle import fbank_ref  # noqa: E402
from res2net_cases import FIXTURES, IDS, load_case, synth_case  # noqa: E402
from wespeaker_hubert_amd.audio import write_wav  # noqa: E402
from wespeaker_hubert_amd.kaldi_io import load_scp_sequential  # noqa: E402
from wespeaker_hubert_amd.speaker_model import HipSpeakerModel  # noqa: E402
from wespeaker_hubert_amd.synthetic import synth_audio, synth_feats, synth_state_dict  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EMB_ATOL, EMB_COS = 1e-4, 0.9999
TAILS = (2, 0)  # fused in every stage, unfused


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


def _model(arch, seed, feat_dim=80, embed_dim=256, two_emb=False):
    """One device handle per (arch, seed, dims), shared by the tests (weights are never changed; a test
    that sets res2_tail puts the default back)."""
    key = (arch, seed, feat_dim, embed_dim, two_emb)
    if key not in _MODELS:
        m = HipSpeakerModel(arch, feat_dim=feat_dim, embed_dim=embed_dim, two_emb_layer=two_emb)
        sd = synth_state_dict(seed, m.state_dict_layout(), residual_tame=True)
        m.load_state_dict(sd)
        m.to(DEV)
        assert m.get_option("res2_tail") == 1
        _MODELS[key] = (m, sd)
    return _MODELS[key]


def _embed(m, x, tail=None):
    if tail is not None:
        m.set_option("res2_tail", tail)
    try:
        out = m(torch.from_numpy(x).to(DEV))
    finally:
        if tail is not None:
            m.set_option("res2_tail", 1)
    assert isinstance(out, torch.Tensor)  # Res2Net.forward returns the embedding itself
    return out.cpu().numpy()


@pytest.mark.parametrize("tail", TAILS, ids=["fused", "unfused"])
@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_fixture(path, tail):
    """Unscaled fixtures: the project's bars (per-dim 1e-4, cosine 0.9999) on O(1) embeddings.  The
    x 8 fixtures: 1e-4 x rms of the reference embedding, as the ERes2Net ones."""
    z, spec, _, _, x = load_case(path)
    m, _ = _model(spec.arch, int(z["weight_seed"]), spec.feat_dim, spec.embed_dim, spec.two_emb_layer)
    ref = z["embed"]
    atol = EMB_ATOL
    if float(z["input_scale"]) != 1.0:
        atol = 1e-4 * float(np.sqrt((ref.astype(np.float64) ** 2).mean()))
    _assert_emb(_embed(m, x, tail), ref, atol)


def test_default_schedule_on_the_recipe_fixture():
    """res2_tail = 1, what a handle runs unless told otherwise."""
    z, spec, _, _, x = load_case(FIXTURES[IDS.index("res2net_base_f80_e256_b2_t200")])
    m, _ = _model(spec.arch, int(z["weight_seed"]), spec.feat_dim, spec.embed_dim)
    _assert_emb(_embed(m, x), z["embed"])


# Base (weights of the first fixture): T' = 2 with a 3-utterance batch, T odd at every level, T even
# then odd, the recipe length; Large (weights of its fixture): the shortest input and T = 75
SHAPES = [("Res2Net34_Base", 171, 3, 9), ("Res2Net34_Base", 171, 2, 37), ("Res2Net34_Base", 171, 4, 10),
          ("Res2Net34_Base", 171, 1, 200), ("Res2Net34_Large", 175, 2, 9), ("Res2Net34_Large", 175, 1, 75)]
SHAPE_IDS = [f"{a.split('_')[1]}-b{b}-t{t}" for a, _, b, t in SHAPES]
_REF = {}


def _shape_case(arch, seed, B, T):
    key = (arch, B, T)
    if key not in _REF:
        _, sd = _model(arch, seed)
        x = synth_feats(1900 + T, B, T, 80)
        _REF[key] = (x, res2net_ref.forward(x, sd, arch).numpy())
    return _REF[key]


@pytest.mark.parametrize("tail", TAILS, ids=["fused", "unfused"])
@pytest.mark.parametrize("arch,seed,B,T", SHAPES, ids=SHAPE_IDS)
def test_against_ref(arch, seed, B, T, tail):
    m, _ = _model(arch, seed)
    x, ref = _shape_case(arch, seed, B, T)
    _assert_emb(_embed(m, x, tail), ref)


@pytest.mark.parametrize("tail", TAILS, ids=["fused", "unfused"])
@pytest.mark.parametrize("arch,seed,B,T", [s for s in SHAPES if s[2] > 1],
                         ids=[i for s, i in zip(SHAPES, SHAPE_IDS) if s[2] > 1])
def test_each_utterance_alone_equals_its_batch_row(arch, seed, B, T, tail):
    m, _ = _model(arch, seed)
    x, _ = _shape_case(arch, seed, B, T)
    full = _embed(m, x, tail)
    for b in range(B):
        one = _embed(m, x[b:b + 1], tail)
        assert np.abs(one[0] - full[b]).max() <= 1e-5


@pytest.mark.parametrize("tail", TAILS, ids=["fused", "unfused"])
def test_two_runs_are_bit_identical(tail):
    m, _ = _model("Res2Net34_Base", 171)
    x, _ = _shape_case("Res2Net34_Base", 171, 2, 37)
    a, b = _embed(m, x, tail), _embed(m, x, tail)
    assert a.tobytes() == b.tobytes()


def test_too_short_input_is_refused():
    m, _ = _model("Res2Net34_Base", 171)
    with pytest.raises(RuntimeError, match="9 frames"):
        m.embed(torch.zeros(1, 8, 80, device=DEV))


TAGS = ("stem", "res2_pw", "res2_pw.c1", "res2_pw.sc", "res2_pw.c3", "res2_conv3x3", "res2_tail", "tstp_head")


def _launches(m, x, tail):
    m.set_option("res2_tail", tail)
    m.profile(True)
    try:
        m(torch.from_numpy(x).to(DEV))
    finally:
        m.profile(False)
        m.set_option("res2_tail", 1)
    return {k: m.profile_query(k)[0] for k in TAGS}


def test_profile_classes():
    """16 blocks, 4 of them with a projection shortcut.  Fused in every stage: conv1 + one tail launch
    per block, no 3x3 and no conv3 launch.  Unfused: conv1, the 3x3 conv and conv3 per block."""
    m, _ = _model("Res2Net34_Base", 171)
    x, _ = _shape_case("Res2Net34_Base", 171, 2, 37)
    assert _launches(m, x, 2) == {"stem": 1, "res2_pw": 20, "res2_pw.c1": 16, "res2_pw.sc": 4, "res2_pw.c3": 0,
                                  "res2_conv3x3": 0, "res2_tail": 16, "tstp_head": 1}
    assert _launches(m, x, 0) == {"stem": 1, "res2_pw": 36, "res2_pw.c1": 16, "res2_pw.sc": 4, "res2_pw.c3": 16,
                                  "res2_conv3x3": 16, "res2_tail": 0, "tstp_head": 1}


def test_front_door_model_dir_to_embedding(tmp_path):
    """config.yaml with the recipe's model_args (res2net.yaml) + avg_model.pt -> load_model ->
    extract_embedding(wav), and bin/extract.py on three short wavs, against fbank_ref + res2net_ref."""
    import wespeaker_hubert_amd as wespeaker
    from wespeaker_hubert_amd.bin.extract import extract
    from wespeaker_hubert_amd.cli.speaker import load_model_pt
    _, _, sd, _ = synth_case("Res2Net34_Base", 179, 0, 1, 9, 80, 256)
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, tmp_path / "avg_model.pt")
    with open(tmp_path / "config.yaml", "w") as f:
        yaml.safe_dump({"model": "Res2Net34_Base",
                        "model_args": {"feat_dim": 80, "embed_dim": 256, "pooling_func": "TSTP", "two_emb_layer": False},
                        "dataset_args": {"frontend": "fbank", "resample_rate": 16000, "num_frms": 200,
                                         "fbank_args": {"num_mel_bins": 80, "frame_shift": 10, "frame_length": 25}}}, f)
    m = load_model_pt(str(tmp_path))
    assert isinstance(m, HipSpeakerModel) and m.spec.family == "res2net"
    pcms = {f"u{i}": synth_audio(146 + i, 1, n)[0] for i, n in enumerate((8801, 12000, 16160))}
    refs = {k: res2net_ref.forward(fbank_ref.fbank(p, cmn=True)[None], sd)[0].numpy() for k, p in pcms.items()}
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
