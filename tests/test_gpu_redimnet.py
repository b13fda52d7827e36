"""ReDimNetB2 on the HIP path against the reference fixtures' float64 embeddings: every fixture
under both GEMM precisions (the project's bars: per-dim 1e-4 and cosine 0.9999 on O(1) embeddings,
about 20x the reference's own float32 error of <= 4.6e-6 on these cases), each batch row bit-equal
to its batch of one, two handles side by side, the refusal of T = 1, the profile classes, and one
bin/extract.py run from a reference-style config with 72 mel bins.

Measured on an MI355X, max |emb - embed64| (bar 1e-4), precision 1 / 0:
  b2_t200 6.4e-6 / 1.1e-6, b3_t2 1.6e-5 / 3.6e-6, b1_t30 7.5e-6 / 1.3e-6,
  b1_t37_e256_2emb 5.9e-6 / 7.5e-7, b2_t301 7.0e-6 / 8.8e-7, b3_t64_mixed 9.4e-6 / 1.5e-6;
  bin/extract.py on three wavs <= 8.4e-6.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import redimnet_ref  # noqa: E402
from oracle import fbank_ref  # noqa: E402
from redimnet_cases import ARCH, FIXTURES, IDS, SEED, load_case, synth_case  # noqa: E402
from wespeaker_hubert_amd.audio import write_wav  # noqa: E402
from wespeaker_hubert_amd.kaldi_io import load_scp_sequential  # noqa: E402
from wespeaker_hubert_amd.speaker_model import HipSpeakerModel  # noqa: E402
from wespeaker_hubert_amd.synthetic import synth_audio, synth_state_dict  # noqa: E402

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


def _model(embed_dim=192, two_emb=False, key=0):
    """One device handle per (dims, key), shared by the tests (weights are never changed; a test that
    sets the precision puts the default back)."""
    k = (embed_dim, two_emb, key)
    if k not in _MODELS:
        m = HipSpeakerModel(ARCH, feat_dim=72, embed_dim=embed_dim, two_emb_layer=two_emb)
        m.load_state_dict(synth_state_dict(SEED, m.state_dict_layout()))
        m.to(DEV)
        _MODELS[k] = m
    return _MODELS[k]


def _embed(m, x):
    out = m(torch.from_numpy(x).to(DEV))
    assert isinstance(out, tuple) and len(out) == 2 and out[0] is None  # the default (aux, embed) branch
    return out[1].cpu().numpy()


@pytest.mark.parametrize("precision", (1, 0))
@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_fixture(path, precision):
    z, spec, _, _, x = load_case(path)
    m = _model(spec.embed_dim, spec.two_emb_layer)
    m.set_option("precision", precision)
    try:
        got = _embed(m, x)
    finally:
        m.set_option("precision", 1)
    _assert_emb(got, z["embed64"])


@pytest.mark.parametrize("path", [p for p in FIXTURES if "_b1_" not in p], ids=[i for i in IDS if "_b1_" not in i])
def test_each_batch_row_is_bit_equal_to_its_batch_of_one(path):
    _, spec, _, _, x = load_case(path)
    m = _model(spec.embed_dim, spec.two_emb_layer)
    full = _embed(m, x)
    for b in range(x.shape[0]):
        assert _embed(m, x[b:b + 1])[0].tobytes() == full[b].tobytes(), b


def test_two_handles_do_not_disturb_each_other():
    """A second handle with other weights, created and run between two runs of the first."""
    z, _, _, _, x = load_case([p for p in FIXTURES if p.endswith("redimnet_b1_t30.npz")][0])
    a = _model()
    first = _embed(a, x)
    b = HipSpeakerModel(ARCH, feat_dim=72, embed_dim=192)
    sd_b = synth_state_dict(SEED + 1, b.state_dict_layout())
    b.load_state_dict(sd_b)
    b.to(DEV)
    got_b = _embed(b, x)
    again = _embed(a, x)
    assert first.tobytes() == again.tobytes()
    _assert_emb(first, z["embed64"])
    _assert_emb(got_b, redimnet_ref.forward(x, sd_b).numpy())
    assert np.abs(got_b - first).max() > 0.1


def test_one_frame_is_refused():
    m = _model()
    with pytest.raises(RuntimeError, match="T >= 2"):
        m.embed(torch.zeros(1, 1, 72, device=DEV))


TAGS = {"rd_stem": 1, "rd_entry": 6, "rd_block2d": 19, "rd_red": 6, "rd_ln": 18, "rd_block1d": 24, "rd_qkv": 6,
        "rd_attn": 6, "rd_lin": 18, "rd_gelu": 6, "rd_exp": 6, "rd_wsum": 1, "glob_ctx": 1, "pool_linear1": 1,
        "pool_linear2": 1, "astp": 1, "head": 1}


def test_profile_classes():
    """One launch per block: 19 2-D blocks, 6 entries, 24 1-D blocks, 6 attentions."""
    _, _, _, _, x = load_case([p for p in FIXTURES if p.endswith("redimnet_b1_t30.npz")][0])
    m = _model()
    m.profile(True)
    try:
        _embed(m, x)
    finally:
        m.profile(False)
    assert {k: m.profile_query(k)[0] for k in TAGS} == TAGS


def test_extract_from_a_reference_style_config(tmp_path):
    """config.yaml with the recipe's model_args (redimnet.yaml: feat_dim 72, num_mel_bins 72) +
    avg_model.pt -> bin/extract.py on three short wavs, against fbank_ref + redimnet_ref."""
    from wespeaker_hubert_amd.bin.extract import extract
    _, _, sd, _ = synth_case(91, 0, 1, 2)
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, tmp_path / "avg_model.pt")
    with open(tmp_path / "config.yaml", "w") as f:
        yaml.safe_dump({"model": ARCH,
                        "model_args": {"feat_dim": 72, "embed_dim": 192, "pooling_func": "ASTP", "two_emb_layer": False},
                        "dataset_args": {"frontend": "fbank", "resample_rate": 16000, "num_frms": 200,
                                         "fbank_args": {"num_mel_bins": 72, "frame_shift": 10, "frame_length": 25}}}, f)
    pcms = {f"u{i}": synth_audio(56 + i, 1, n)[0] for i, n in enumerate((8801, 12000, 16160))}
    refs = {k: redimnet_ref.forward(fbank_ref.fbank(p, num_mel_bins=72, cmn=True)[None], sd)[0].numpy()
            for k, p in pcms.items()}
    for k, p in pcms.items():
        write_wav(str(tmp_path / f"{k}.wav"), p)
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
