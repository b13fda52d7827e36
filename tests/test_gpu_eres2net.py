"""ERes2Net (Base, Large, aug) on the HIP path against the reference fixtures and
tests/eres2net_ref.py: every fixture (the two x 8 ones drive activations into the clamp), tile-tail
shapes, batch invariance, run-to-run bit identity, a batch wider than one operand chunk, the
profile classes and the front door (config.yaml + avg_model.pt -> load_model -> wav, bin/extract)."""
import json
import os
import sys

import numpy as np
import pytest
import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import eres2net_ref  # noqa: E402
from oracle import fbank_ref  # noqa: E402
from eres2net_cases import FIXTURES, IDS, load_case, synth_case  # noqa: E402
from wespeaker_hubert_amd.audio import write_wav  # noqa: E402
from wespeaker_hubert_amd.kaldi_io import load_scp_sequential  # noqa: E402
from wespeaker_hubert_amd.speaker_model import HipSpeakerModel  # noqa: E402
from wespeaker_hubert_amd.synthetic import synth_audio, synth_feats, synth_state_dict  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EMB_ATOL, EMB_COS = 1e-4, 0.9999


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


def _model(arch, seed, feat_dim=80, embed_dim=512, two_emb=False):
    """One device handle per (arch, seed, dims), shared by the tests (weights are never changed)."""
    key = (arch, seed, feat_dim, embed_dim, two_emb)
    if key not in _MODELS:
        m = HipSpeakerModel(arch, feat_dim=feat_dim, embed_dim=embed_dim, two_emb_layer=two_emb)
        sd = synth_state_dict(seed, m.state_dict_layout(), residual_tame=True)
        m.load_state_dict(sd)
        m.to(DEV)
        _MODELS[key] = (m, sd)
    return _MODELS[key]


def _embed(m, x):
    out = m(torch.from_numpy(x).to(DEV))
    assert isinstance(out, torch.Tensor)  # ERes2Net.forward returns the embedding itself
    return out.cpu().numpy()


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_fixture(path):
    """Unscaled fixtures: the project's bars (per-dim 1e-4, cosine 0.9999) on O(1) embeddings.  The
    x 8 fixtures (embeddings up to 39): 1e-4 x rms of the reference embedding, 1.15e-3 (Base) and
    9.7e-4 (aug)."""
    z, spec, _, _, x = load_case(path)
    m, _ = _model(spec.arch, int(z["weight_seed"]), spec.feat_dim, spec.embed_dim, spec.two_emb_layer)
    ref = z["embed"]
    atol = EMB_ATOL
    if float(z["input_scale"]) != 1.0:
        atol = 1e-4 * float(np.sqrt((ref.astype(np.float64) ** 2).mean()))
    _assert_emb(_embed(m, x), ref, atol)


# Base (weights of the first fixture): T' = 2 with a 3-utterance batch, T odd at every level, the
# recipe length, T even then odd; aug (weights of its fixture): the shortest input and T = 75
SHAPES = [("ERes2Net34_Base", 71, 512, 3, 9), ("ERes2Net34_Base", 71, 512, 2, 37), ("ERes2Net34_Base", 71, 512, 1, 200),
          ("ERes2Net34_Base", 71, 512, 4, 10), ("ERes2Net34_aug", 76, 192, 2, 9), ("ERes2Net34_aug", 76, 192, 1, 75)]
SHAPE_IDS = [f"{a.split('_')[1]}-b{b}-t{t}" for a, _, _, b, t in SHAPES]
_REF = {}


def _shape_case(arch, seed, emb, B, T):
    key = (arch, B, T)
    if key not in _REF:
        _, sd = _model(arch, seed, 80, emb)
        x = synth_feats(900 + T, B, T, 80)
        _REF[key] = (x, eres2net_ref.forward(x, sd, arch).numpy())
    return _REF[key]


@pytest.mark.parametrize("arch,seed,emb,B,T", SHAPES, ids=SHAPE_IDS)
def test_against_ref(arch, seed, emb, B, T):
    m, _ = _model(arch, seed, 80, emb)
    x, ref = _shape_case(arch, seed, emb, B, T)
    _assert_emb(_embed(m, x), ref)


@pytest.mark.parametrize("arch,seed,emb,B,T", [s for s in SHAPES if s[3] > 1],
                         ids=[i for s, i in zip(SHAPES, SHAPE_IDS) if s[3] > 1])
def test_each_utterance_alone_equals_its_batch_row(arch, seed, emb, B, T):
    m, _ = _model(arch, seed, 80, emb)
    x, _ = _shape_case(arch, seed, emb, B, T)
    full = _embed(m, x)
    for b in range(B):
        one = _embed(m, x[b:b + 1])
        assert np.abs(one[0] - full[b]).max() <= 1e-5


def test_two_runs_are_bit_identical():
    m, _ = _model("ERes2Net34_Base", 71)
    x, _ = _shape_case("ERes2Net34_Base", 71, 512, 2, 37)
    a, b = _embed(m, x), _embed(m, x)
    assert a.tobytes() == b.tobytes()


def test_batch_wider_than_one_operand_chunk():
    """Base, B = 128 x T = 1000: a stage-1 block output is 20.5 MB per utterance, so the 2 GiB
    operand cap splits the batch into two chunks of 64; utterance b carries features b % 2, so every
    row must equal the B = 2 run's row b % 2 (each utterance's result is independent of its batch)."""
    m, _ = _model("ERes2Net34_Base", 71)
    two = synth_feats(801, 2, 1000, 80)
    small = _embed(m, two)
    big = m(torch.from_numpy(two).to(DEV).repeat(64, 1, 1)).cpu().numpy()
    assert big.shape == (128, 512) and np.isfinite(big).all()
    assert np.abs(big - np.tile(small, (64, 1))).max() <= 1e-5


def test_too_short_input_is_refused():
    m, _ = _model("ERes2Net34_Base", 71)
    with pytest.raises(RuntimeError, match="9 frames"):
        m.embed(torch.zeros(1, 8, 80, device=DEV))


def _launches(m, x, tags):
    m.profile(True)
    try:
        _embed(m, x)
    finally:
        m.profile(False)
    return {k: m.profile_query(k)[0] for k in tags}


def test_profile_classes():
    """One launch per Res2 step (no step fusion): 16 blocks x scale 2 = 32 `eres_conv3x3`; an AFF in
    front of the second step of the 9 blocks of stages 3-4 plus the 3 bottom-up ones = 12 `eres_aff`;
    the 1x1 convs are `eres_pw` (conv1 and conv3 of 16 blocks, 4 projection shortcuts).  aug (scale
    3): 9 x 2 + 3 AFFs, 48 steps."""
    m, _ = _model("ERes2Net34_Base", 71)
    x, _ = _shape_case("ERes2Net34_Base", 71, 512, 2, 37)
    n = _launches(m, x, ("stem", "eres_pw", "eres_pw.c1", "eres_pw.sc", "eres_conv3x3", "eres_aff", "eres_down",
                         "tstp_head"))
    assert n == {"stem": 1, "eres_pw": 36, "eres_pw.c1": 16, "eres_pw.sc": 4, "eres_conv3x3": 32, "eres_aff": 12,
                 "eres_down": 3, "tstp_head": 1}
    m, _ = _model("ERes2Net34_aug", 76, 80, 192)
    x, _ = _shape_case("ERes2Net34_aug", 76, 192, 2, 9)
    assert _launches(m, x, ("eres_aff", "eres_conv3x3", "eres_down")) == {"eres_aff": 21, "eres_conv3x3": 48,
                                                                           "eres_down": 3}


def test_front_door_model_dir_to_embedding(tmp_path):
    """config.yaml with the recipe's model_args (eres2net.yaml) + avg_model.pt -> load_model ->
    extract_embedding(wav), and bin/extract.py on three short wavs, against fbank_ref + eres2net_ref."""
    import wespeaker_hubert_amd as wespeaker
    from wespeaker_hubert_amd.bin.extract import extract
    from wespeaker_hubert_amd.cli.speaker import load_model_pt
    _, _, sd, _ = synth_case("ERes2Net34_Base", 79, 0, 1, 9, 80, 512)
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, tmp_path / "avg_model.pt")
    with open(tmp_path / "config.yaml", "w") as f:
        yaml.safe_dump({"model": "ERes2Net34_Base",
                        "model_args": {"feat_dim": 80, "embed_dim": 512, "pooling_func": "TSTP", "two_emb_layer": False},
                        "dataset_args": {"frontend": "fbank", "resample_rate": 16000, "num_frms": 200,
                                         "fbank_args": {"num_mel_bins": 80, "frame_shift": 10, "frame_length": 25}}}, f)
    m = load_model_pt(str(tmp_path))
    assert isinstance(m, HipSpeakerModel) and m.spec.family == "eres2net"
    pcms = {f"u{i}": synth_audio(46 + i, 1, n)[0] for i, n in enumerate((8801, 12000, 16160))}
    refs = {k: eres2net_ref.forward(fbank_ref.fbank(p, cmn=True)[None], sd)[0].numpy() for k, p in pcms.items()}
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
