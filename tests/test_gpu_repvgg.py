"""RepVGG (the REPVGG_* names) on the HIP path against the reference fixtures and tests/repvgg_ref.py, in
both checkpoint forms (training form folded on the host when the model goes to the device; deploy form as the
converter wrote it) and, for the RepSPK models, on the 17-tap kernel (option rsbb_taps 2, and the default 1)
and on the dense 25-tap path (0): every fixture, tile-tail shapes, batch invariance, run-to-run bit identity,
the refusal of T = 8, a poked dead tap, the profile classes and the front door (config.yaml + avg_model.pt ->
load_model -> wav, bin/extract; the same after bin/convert_repvgg)."""
import json
import os
import sys

import numpy as np
import pytest
import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import repvgg_ref  # noqa: E402
from oracle import fbank_ref  # noqa: E402
from repvgg_cases import FIXTURES, IDS, load_case, synth_case  # noqa: E402
from wespeaker_hubert_amd import arch as A  # noqa: E402
from wespeaker_hubert_amd.audio import write_wav  # noqa: E402
from wespeaker_hubert_amd.kaldi_io import load_scp_sequential  # noqa: E402
from wespeaker_hubert_amd.speaker_model import HipSpeakerModel  # noqa: E402
from wespeaker_hubert_amd.synthetic import synth_audio, synth_feats  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EMB_ATOL, EMB_COS = 1e-4, 0.9999
RSBB_IDS = [i for i in IDS if "rsbb" in i]


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


def _model(arch, seed, feat_dim=80, embed_dim=256, deploy=False):
    """One device handle per (arch, seed, dims, form), shared by the tests (weights are never changed; a test
    that sets rsbb_taps puts the default back).  Returns (model, training-form dict, deploy-form dict)."""
    key = (arch, seed, feat_dim, embed_dim, deploy)
    if key not in _MODELS:
        spec, _, sd, _ = synth_case(arch, seed, 0, 1, 9, feat_dim, embed_dim)
        folded = A.repvgg_fold(spec, sd)
        m = HipSpeakerModel(arch, feat_dim=feat_dim, embed_dim=embed_dim, deploy=deploy)
        assert m.load_state_dict(folded if deploy else sd, strict=True) == ([], [])
        m.to(DEV)
        assert m.get_option("rsbb_taps") == 1
        _MODELS[key] = (m, sd, folded)
    return _MODELS[key]


def _embed(m, x, taps=None):
    if taps is not None:
        m.set_option("rsbb_taps", taps)
    try:
        out = m(torch.from_numpy(x).to(DEV))
    finally:
        if taps is not None:
            m.set_option("rsbb_taps", 1)
    assert isinstance(out, torch.Tensor)  # RepVGG.forward returns the embedding itself
    return out.cpu().numpy()


@pytest.mark.parametrize("deploy", (False, True), ids=["train_form", "deploy_form"])
@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_fixture(path, deploy):
    z, spec, _, _, x = load_case(path)
    m, _, _ = _model(spec.arch, int(z["weight_seed"]), spec.feat_dim, spec.embed_dim, deploy)
    _assert_emb(_embed(m, x), z["embed_deploy" if deploy else "embed"])


@pytest.mark.parametrize("taps", (0, 2), ids=["dense25", "live17"])
@pytest.mark.parametrize("path", [FIXTURES[IDS.index(i)] for i in RSBB_IDS], ids=RSBB_IDS)
def test_rsbb_fixture_on_both_paths(path, taps):
    z, spec, _, _, x = load_case(path)
    m, _, _ = _model(spec.arch, int(z["weight_seed"]), spec.feat_dim, spec.embed_dim, True)
    _assert_emb(_embed(m, x, taps), z["embed_deploy"])


# TINY_A0 (weights of its first fixture): T' = 2 with a 3-utterance batch, T odd at every level, T even then
# odd, the recipe length; TINY_RSBB_A0 (weights of its fixture): the shortest input and T = 75
SHAPES = [("REPVGG_TINY_A0", 191, 3, 9), ("REPVGG_TINY_A0", 191, 2, 37), ("REPVGG_TINY_A0", 191, 4, 10),
          ("REPVGG_TINY_A0", 191, 1, 200), ("REPVGG_TINY_RSBB_A0", 194, 2, 9), ("REPVGG_TINY_RSBB_A0", 194, 1, 75)]
SHAPE_IDS = [f"{a[7:]}-b{b}-t{t}" for a, _, b, t in SHAPES]
_REF = {}


def _shape_case(arch, seed, B, T):
    key = (arch, B, T)
    if key not in _REF:
        _, sd, _ = _model(arch, seed)
        x = synth_feats(2300 + T, B, T, 80)
        _REF[key] = (x, repvgg_ref.forward(x, sd, arch).numpy())
    return _REF[key]


def _paths(arch):
    return (0, 2) if "RSBB" in arch else (None,)


@pytest.mark.parametrize("arch,seed,B,T", SHAPES, ids=SHAPE_IDS)
def test_against_ref(arch, seed, B, T):
    m, _, _ = _model(arch, seed)
    x, ref = _shape_case(arch, seed, B, T)
    for taps in _paths(arch):
        _assert_emb(_embed(m, x, taps), ref)


@pytest.mark.parametrize("arch,seed,B,T", [s for s in SHAPES if s[2] > 1],
                         ids=[i for s, i in zip(SHAPES, SHAPE_IDS) if s[2] > 1])
def test_each_utterance_alone_equals_its_batch_row(arch, seed, B, T):
    m, _, _ = _model(arch, seed)
    x, _ = _shape_case(arch, seed, B, T)
    for taps in _paths(arch):
        full = _embed(m, x, taps)
        for b in range(B):
            assert _embed(m, x[b:b + 1], taps)[0].tobytes() == full[b].tobytes(), (taps, b)


@pytest.mark.parametrize("arch,seed", [("REPVGG_TINY_A0", 191), ("REPVGG_TINY_RSBB_A0", 194)], ids=["A0", "RSBB_A0"])
def test_two_runs_are_bit_identical(arch, seed):
    m, _, _ = _model(arch, seed)
    x, _ = _shape_case(arch, seed, 2, 37 if arch == "REPVGG_TINY_A0" else 9)
    for taps in _paths(arch):
        assert _embed(m, x, taps).tobytes() == _embed(m, x, taps).tobytes()


def test_too_short_input_is_refused():
    m, _, _ = _model("REPVGG_TINY_A0", 191)
    with pytest.raises(RuntimeError, match="9 frames"):
        m.embed(torch.zeros(1, 8, 80, device=DEV))


TAGS = ("stem", "rep_conv3x3", "rsbb_sparse", "rsbb_dense", "rsbb_dense.L2", "rsbb_sparse.L2", "tstp_head")


def _launches(m, x, taps):
    m.set_option("rsbb_taps", taps)
    m.profile(True)
    try:
        m(torch.from_numpy(x).to(DEV))
    finally:
        m.profile(False)
        m.set_option("rsbb_taps", 1)
    return {k: m.profile_query(k)[0] for k in TAGS}


def test_profile_classes_and_a_poked_dead_tap():
    """33 blocks behind the stem.  RepVGG: all on the 3x3 classes.  RepSPK: all on the 17-tap kernel
    (rsbb_taps 2) or all dense (0); with one dead tap of stage2.1 poked non-zero that layer, and only that
    layer, runs dense whatever the option says, and the result is the dense path's within the bars."""
    m, _, _ = _model("REPVGG_TINY_A0", 191)
    x, _ = _shape_case("REPVGG_TINY_A0", 191, 2, 37)
    assert _launches(m, x, 1) == {"stem": 1, "rep_conv3x3": 33, "rsbb_sparse": 0, "rsbb_dense": 0, "rsbb_dense.L2": 0,
                                  "rsbb_sparse.L2": 0, "tstp_head": 1}
    m, _, folded = _model("REPVGG_TINY_RSBB_A0", 194)
    x, _ = _shape_case("REPVGG_TINY_RSBB_A0", 194, 2, 9)
    assert _launches(m, x, 2) == {"stem": 1, "rep_conv3x3": 0, "rsbb_sparse": 33, "rsbb_dense": 0, "rsbb_dense.L2": 0,
                                  "rsbb_sparse.L2": 4, "tstp_head": 1}
    assert _launches(m, x, 0) == {"stem": 1, "rep_conv3x3": 0, "rsbb_sparse": 0, "rsbb_dense": 33, "rsbb_dense.L2": 4,
                                  "rsbb_sparse.L2": 0, "tstp_head": 1}
    poked = dict(folded)
    w = poked["stage2.1.rbr_reparam.weight"].copy()
    w[:, :, 0, 1] = 0.01  # the whole tap, so that the embedding moves by far more than the bars
    poked["stage2.1.rbr_reparam.weight"] = w
    assert A.repvgg_dense_blocks(m.spec, poked) == ("stage2.1",)
    pm = HipSpeakerModel("REPVGG_TINY_RSBB_A0", feat_dim=80, embed_dim=256, deploy=True)
    pm.load_state_dict(poked, strict=True)
    pm.to(DEV)
    assert _launches(pm, x, 2) == {"stem": 1, "rep_conv3x3": 0, "rsbb_sparse": 32, "rsbb_dense": 1, "rsbb_dense.L2": 1,
                                   "rsbb_sparse.L2": 3, "tstp_head": 1}
    ref = repvgg_ref.forward(x, poked, "REPVGG_TINY_RSBB_A0").numpy()
    assert np.abs(ref - _shape_case("REPVGG_TINY_RSBB_A0", 194, 2, 9)[1]).max() > 10 * EMB_ATOL  # the poke is felt
    _assert_emb(_embed(pm, x, 2), ref)
    _assert_emb(_embed(pm, x, 0), ref)


def test_front_door_model_dir_to_embedding_in_either_order(tmp_path):
    """config.yaml with the recipe's model_args (repvgg.yaml) + avg_model.pt -> load_model ->
    extract_embedding(wav), and bin/extract.py on three short wavs, against fbank_ref + repvgg_ref; then the
    project's convert tool and the same extraction from convert_model.pt + the rewritten config."""
    import wespeaker_hubert_amd as wespeaker
    from wespeaker_hubert_amd.bin.convert_repvgg import convert
    from wespeaker_hubert_amd.bin.extract import extract
    from wespeaker_hubert_amd.cli.speaker import load_model_pt
    _, _, sd, _ = synth_case("REPVGG_TINY_A0", 199, 0, 1, 9, 80, 256)
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, tmp_path / "avg_model.pt")
    with open(tmp_path / "config.yaml", "w") as f:
        yaml.safe_dump({"model": "REPVGG_TINY_A0", "exp_dir": str(tmp_path),
                        "model_args": {"feat_dim": 80, "embed_dim": 256, "pooling_func": "TSTP", "deploy": False,
                                       "use_se": False},
                        "dataset_args": {"frontend": "fbank", "resample_rate": 16000, "num_frms": 200,
                                         "fbank_args": {"num_mel_bins": 80, "frame_shift": 10, "frame_length": 25}}}, f)
    m = load_model_pt(str(tmp_path))
    assert isinstance(m, HipSpeakerModel) and m.spec.family == "repvgg" and not m.spec.deploy
    pcms = {f"u{i}": synth_audio(246 + i, 1, n)[0] for i, n in enumerate((8801, 12000, 16160))}
    refs = {k: repvgg_ref.forward(fbank_ref.fbank(p, cmn=True)[None], sd)[0].numpy() for k, p in pcms.items()}
    for k, p in pcms.items():
        write_wav(str(tmp_path / f"{k}.wav"), p)
    spk = wespeaker.load_model(str(tmp_path))
    _assert_emb(spk.extract_embedding(str(tmp_path / "u1.wav")).numpy()[None], refs["u1"][None])
    with open(tmp_path / "raw.list", "w") as f:
        for k in pcms:
            f.write(json.dumps({"key": k, "wav": str(tmp_path / f"{k}.wav"), "spk": "s0"}) + "\n")

    def run(model_path, tag):
        scp = extract(config=str(tmp_path / "config.yaml"), model_path=str(model_path), data_type="raw",
                      data_list=str(tmp_path / "raw.list"), embed_ark=str(tmp_path / f"{tag}.ark"), batch_size=1,
                      num_workers=1)
        rows = dict(load_scp_sequential(scp))
        assert sorted(rows) == sorted(pcms)
        return rows
    first = run(tmp_path / "avg_model.pt", "xvector")
    for k, e in first.items():
        _assert_emb(e[None], refs[k][None])
    convert(str(tmp_path / "config.yaml"), str(tmp_path / "avg_model.pt"), str(tmp_path / "convert_model.pt"))
    with open(tmp_path / "config.yaml") as f:
        assert yaml.safe_load(f)["model_args"]["deploy"] is True
    second = run(tmp_path / "convert_model.pt", "xvector_deploy")
    for k, e in second.items():
        _assert_emb(e[None], first[k][None])
        _assert_emb(e[None], refs[k][None])
