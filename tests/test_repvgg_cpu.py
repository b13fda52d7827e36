"""RepVGG (the REPVGG_* names) without a GPU: the parameter tables in both checkpoint forms (arch.py and the
library's), every refusal, the host fold against the checksums of the tensors the reference's own converter
made, the dead taps of a folded RepSPK kernel, the torch-CPU restatement tests/repvgg_ref.py against the
fixtures (tests/golden/make_repvgg_golden.py), the convert tool, the FLOP count and the workspace query."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import repvgg_ref  # noqa: E402
from repvgg_cases import CHECKED_BLOCKS, FIXTURES, IDS, last_block, load_case, synth_case  # noqa: E402
from wespeaker_hubert_amd import _lib  # noqa: E402
from wespeaker_hubert_amd import arch as A  # noqa: E402
from wespeaker_hubert_amd.bin.convert_repvgg import convert  # noqa: E402
from wespeaker_hubert_amd.speaker_model import HipSpeakerModel, get_speaker_model  # noqa: E402

EMB_ATOL, EMB_COS = 1e-4, 0.9999  # the project's bars
RSBB = [p for p in FIXTURES if "rsbb" in p]
SHORT = [p for p in FIXTURES if "_t37" in p or "_t9" in p or "_t50" in p]

_FOLDS = {}


def folded(path):
    """The fixture's training-form weights through arch.repvgg_fold, computed once."""
    if path not in _FOLDS:
        _, spec, _, sd, _ = load_case(path)
        _FOLDS[path] = A.repvgg_fold(spec, sd)
    return _FOLDS[path]


def _assert_emb(got, ref, atol=EMB_ATOL):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    assert np.abs(got - ref).max() < atol, np.abs(got - ref).max()
    cos = (got * ref).sum(1) / np.linalg.norm(got, axis=1) / np.linalg.norm(ref, axis=1)
    assert cos.min() >= EMB_COS, cos.min()


def test_the_eight_fixtures_exist():
    assert len(FIXTURES) == 8 and len(RSBB) == 4, FIXTURES
    for p in FIXTURES:
        assert os.path.getsize(p) < (1 << 20)
        z = np.load(p)
        assert all(0.1 <= float(z[f"rms_stage{li}"]) <= 10.0 for li in range(5))


def _shapes(v):
    return [tuple(int(s) for s in str(x).split(",") if s) for x in v]


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_param_layout_matches_reference_in_both_forms(path):
    z, spec, plist, _, _ = load_case(path)
    assert A.param_list(spec) == plist and spec.family == "repvgg" and not spec.deploy
    assert [n for n, _ in plist] == [str(n) for n in z["param_names"]]
    assert [tuple(s) for _, s in plist] == _shapes(z["param_shapes"])
    dep = A.repvgg_params(A.make_spec(spec.arch, feat_dim=spec.feat_dim, embed_dim=spec.embed_dim, deploy=True))
    assert [n for n, _ in dep] == [str(n) for n in z["param_names_deploy"]]
    assert [tuple(s) for _, s in dep] == _shapes(z["param_shapes_deploy"])
    assert list(folded(path)) == [n for n, _ in dep]
    assert [tuple(v.shape) for v in folded(path).values()] == [tuple(s) for _, s in dep]


def test_entry_counts():
    def n(arch, deploy):
        return len(A.repvgg_params(A.make_spec(arch, deploy=deploy)))
    assert (n("REPVGG_TINY_A0", False), n("REPVGG_TINY_A0", True)) == (560, 70)
    assert n("REPVGG_TINY_RSBB_A0", False) == 560
    assert (n("REPVGG_A0", False), n("REPVGG_A0", True)) == (356, 46)
    assert n("REPVGG_RSBB_A2", False) == 351
    assert len(A.REPVGG_ARCHS) == 9
    # seg is sized for int(feat_dim / 8) rows of the last width, mean and std
    assert dict(A.repvgg_params(A.make_spec("REPVGG_A2", feat_dim=40, embed_dim=7)))["seg.weight"] == (7, 2 * 5 * 1408)
    assert dict(A.repvgg_params(A.make_spec("REPVGG_RSBB_A0", deploy=True)))["stage2.0.rbr_reparam.weight"] == (96, 48, 5, 5)


def test_make_spec_defaults_and_refusals():
    s = A.make_spec("REPVGG_TINY_A0")
    assert (s.feat_dim, s.embed_dim, s.pooling_func, s.deploy, s.family) == (80, 256, "TSTP", False, "repvgg")
    assert A.make_spec("REPVGG_B0", deploy=True, use_se=False).deploy
    for name in ("REPVGG_B1", "REPVGG_B2", "REPVGG_B3", "REPVGG_B1g2", "REPVGG_B2g4", "REPVGG_B3g2", "REPVGG_D2SE"):
        with pytest.raises(NotImplementedError, match=name):
            A.make_spec(name)
        with pytest.raises(NotImplementedError):
            get_speaker_model(name)
    with pytest.raises(NotImplementedError, match="use_se"):
        A.make_spec("REPVGG_TINY_A0", use_se=True)
    with pytest.raises(NotImplementedError, match="TSTP"):
        A.make_spec("REPVGG_TINY_A0", pooling_func="ASTP")
    with pytest.raises(TypeError):
        A.make_spec("REPVGG_A0", emb_bn=True)
    with pytest.raises(TypeError):
        A.make_spec("REPVGG_A0", two_emb_layer=False)
    for fd in (0, 4, 84):
        with pytest.raises(ValueError, match="multiple of 8"):
            A.make_spec("REPVGG_A1", feat_dim=fd)
    with pytest.raises(KeyError):
        A.make_spec("REPVGG_X")


def _create(arch, feat_dim, embed_dim, emb_bn=0, two_emb=0):
    lib = _lib.load()
    h = ctypes.c_void_p()
    rc = lib.wsp_model_create(arch.encode(), feat_dim, embed_dim, emb_bn, int(two_emb), ctypes.byref(h))
    return lib, h, rc


@pytest.mark.parametrize("arch,feat_dim,embed_dim", [("REPVGG_TINY_A0", 80, 256), ("REPVGG_RSBB_A2", 40, 192),
                                                     ("REPVGG_A0", 8, 64), ("REPVGG_RSBB_B0", 80, 256)])
def test_library_table_is_the_deploy_layout(arch, feat_dim, embed_dim):
    lib, h, rc = _create(arch, feat_dim, embed_dim)
    assert rc == 0, lib.wsp_last_error()
    try:
        name, ndim, shape = ctypes.c_char_p(), ctypes.c_int(), (ctypes.c_int64 * 4)()
        out = []
        for i in range(lib.wsp_model_num_params(h)):
            assert lib.wsp_model_param_info(h, i, ctypes.byref(name), ctypes.byref(ndim), shape) == 0
            out.append((name.value.decode(), tuple(shape[d] for d in range(ndim.value))))
    finally:
        lib.wsp_model_destroy(h)
    want = A.repvgg_params(A.make_spec(arch, feat_dim=feat_dim, embed_dim=embed_dim, deploy=True))
    assert out == [(n, tuple(s)) for n, s in want]


def test_library_refusals_and_rsbb_taps():
    for name in ("REPVGG_B1", "REPVGG_B3g4", "REPVGG_D2SE", "REPVGG_X"):
        lib, h, rc = _create(name, 80, 256)
        assert rc != 0 and b"unsupported arch" in lib.wsp_last_error()
    lib, h, rc = _create("REPVGG_TINY_A0", 84, 256)
    assert rc != 0 and b"multiple of 8" in lib.wsp_last_error()
    assert _create("REPVGG_TINY_A0", 80, 0)[2] != 0
    lib, h, rc = _create("REPVGG_TINY_A0", 80, 256, emb_bn=1)
    assert rc != 0 and b"emb_bn" in lib.wsp_last_error()
    assert _create("REPVGG_TINY_A0", 80, 256, two_emb=1)[2] != 0
    lib, h, rc = _create("REPVGG_TINY_RSBB_A0", 80, 256)
    assert rc == 0
    try:
        v = ctypes.c_int(-1)
        assert lib.wsp_model_get_option(h, b"rsbb_taps", ctypes.byref(v)) == 0 and v.value == 1
        assert lib.wsp_model_set_option(h, b"rsbb_taps", 3) != 0 and b"rsbb_taps must be 0" in lib.wsp_last_error()
        assert lib.wsp_model_set_option(h, b"rsbb_taps", -1) != 0
        for val in (0, 2, 1):
            assert lib.wsp_model_set_option(h, b"rsbb_taps", val) == 0
            assert lib.wsp_model_get_option(h, b"rsbb_taps", ctypes.byref(v)) == 0 and v.value == val
    finally:
        lib.wsp_model_destroy(h)
    lib, h, rc = _create("ResNet34", 80, 256)  # the key is refused on handles that do not own it
    assert rc == 0
    try:
        assert lib.wsp_model_set_option(h, b"rsbb_taps", 0) != 0 and b"RepVGG handles" in lib.wsp_last_error()
    finally:
        lib.wsp_model_destroy(h)


def test_workspace_query_answers_without_a_device():
    """B = 128 x T = 1000: two ping-pong activations of the widest operand (stage 1: 80 x 1000 x 32 floats =
    10.24 MB per utterance for TINY; 64 padded channels for A0), chunked under the 2 GiB operand cap."""
    for arch, width in (("REPVGG_TINY_RSBB_A0", 32), ("REPVGG_A0", 64)):
        lib, h, rc = _create(arch, 80, 256)
        assert rc == 0
        try:
            def ws(B):
                b = ctypes.c_size_t()
                assert lib.wsp_model_workspace_bytes(h, B, 1000, ctypes.byref(b)) == 0, lib.wsp_last_error()
                return b.value
            per_utt = 80 * 1000 * width * 4
            assert 2 * 128 * per_utt <= ws(128) < 2.1 * 128 * per_utt if width == 32 else ws(128) < 2.1 * 128 * per_utt
            assert ws(1) < ws(2) < ws(64)
        finally:
            lib.wsp_model_destroy(h)


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_fold_reproduces_the_reference_converter(path):
    """The stored figures are float64 sums of the float32 tensors the reference's converter made (its fold
    runs in float32); ours runs in float64 and rounds once.  Relative 1e-6: of the abs-sum for both figures
    (a plain sum can cancel to nothing)."""
    z, spec, _, _, _ = load_case(path)
    f = folded(path)
    for tag in CHECKED_BLOCKS:
        p = last_block(spec) if tag == "last" else tag
        for leaf, key in ((".rbr_reparam.weight", "w"), (".rbr_reparam.bias", "b")):
            t = f[p + leaf].astype(np.float64)
            assert f[p + leaf].dtype == np.float32
            a = float(z[f"wabs_{tag}_{key}"])
            assert abs(np.abs(t).sum() - a) <= 1e-6 * a, (tag, leaf)
            assert abs(t.sum() - float(z[f"wsum_{tag}_{key}"])) <= 1e-6 * a, (tag, leaf)
    np.testing.assert_array_equal(f["seg.weight"], load_case(path)[3]["seg.weight"])


def test_fold_by_hand_on_one_block():
    """One RepVGG and one RepSPK block against the formulas written out per element."""
    for arch, k in (("REPVGG_TINY_A0", 3), ("REPVGG_TINY_RSBB_A0", 5)):
        spec, _, sd, _ = synth_case(arch, 7, 8, 1, 9, 8, 16)
        f = A.repvgg_fold(spec, sd)
        p, n, c = "stage1.1", 5, 9  # an identity block; output channel n, input channel c (and the diagonal n, n)

        def aff(q):
            t = sd[q + ".weight"].astype(np.float64) / np.sqrt(sd[q + ".running_var"].astype(np.float64) + 1e-5)
            return t, sd[q + ".bias"].astype(np.float64) - sd[q + ".running_mean"].astype(np.float64) * t
        t3, b3 = aff(p + ".rbr_dense.bn")
        br = ".rbr_dense_dilation" if k == 5 else ".rbr_1x1"
        t2, b2 = aff(p + br + ".bn")
        ti, bi = aff(p + ".rbr_identity")
        for cc in (c, n):
            want = np.zeros((k, k))
            want[k // 2 - 1:k // 2 + 2, k // 2 - 1:k // 2 + 2] += sd[p + ".rbr_dense.conv.weight"][n, cc].astype(np.float64) * t3[n]
            w2 = sd[p + br + ".conv.weight"][n, cc].astype(np.float64) * t2[n]
            if k == 5:
                want[::2, ::2] += w2
            else:
                want[1, 1] += w2[0, 0]
            if cc == n:
                want[k // 2, k // 2] += ti[n]
            np.testing.assert_array_equal(f[p + ".rbr_reparam.weight"][n, cc], want.astype(np.float32))
        assert f[p + ".rbr_reparam.bias"][n] == np.float32(b3[n] + b2[n] + bi[n])


@pytest.mark.parametrize("path", RSBB, ids=[i for i in IDS if "rsbb" in i])
def test_folded_repspk_kernels_are_zero_at_the_dead_taps(path):
    _, spec, _, _, _ = load_case(path)
    assert len(A.RSBB_LIVE_TAPS) == 17 and len(A.RSBB_DEAD_TAPS) == 8 and (2, 2) in A.RSBB_LIVE_TAPS
    f = folded(path)
    for p, *_ in A.repvgg_blocks(spec):
        w = f[p + ".rbr_reparam.weight"]
        assert w.shape[2:] == (5, 5)
        for kf, kt in A.RSBB_DEAD_TAPS:
            assert not w[:, :, kf, kt].any(), (p, kf, kt)
        for kf, kt in A.RSBB_LIVE_TAPS:
            assert w[:, :, kf, kt].any(), (p, kf, kt)
    assert A.repvgg_dense_blocks(spec, f) == ()


def test_a_poked_dead_tap_flips_that_layer_only():
    path = FIXTURES[IDS.index("repvgg_tiny_rsbb_a0_f8_e64_b3_t9")]
    _, spec, _, _, _ = load_case(path)
    f = dict(folded(path))
    w = f["stage2.1.rbr_reparam.weight"].copy()
    w[3, 7, 0, 1] = 1e-3
    f["stage2.1.rbr_reparam.weight"] = w
    assert A.repvgg_dense_blocks(spec, f) == ("stage2.1",)
    T = 50
    sparse, poked, dense = (A.repvgg_gflop_per_utt(spec, T), A.repvgg_gflop_per_utt(spec, T, 1, ("stage2.1",)),
                            A.repvgg_gflop_per_utt(spec, T, 0))
    # stage 2 at T = 50: F x T = 4 x 25 positions, 64 -> 64 channels, 8 more taps
    assert poked - sparse == pytest.approx(2.0 * 4 * 25 * 64 * 64 * 8 / 1e9, rel=1e-9)
    assert sparse < poked < dense
    # a RepVGG model has no such layers
    spec3 = A.make_spec("REPVGG_TINY_A0", feat_dim=8, embed_dim=64)
    assert A.repvgg_dense_blocks(spec3, {}) == ()


_REF = {}


def ref_runs(path):
    """f32 restatement in both forms (training form with its stage outputs), computed once."""
    if path not in _REF:
        _, spec, _, sd, x = load_case(path)
        emb, inter = repvgg_ref.forward(x, sd, spec.arch, taps=True)
        _REF[path] = (emb, inter, repvgg_ref.forward(x, folded(path), spec.arch))
    return _REF[path]


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_ref_matches_reference_forward_in_both_forms(path):
    z, _, _, _, x = load_case(path)
    assert abs(x.astype(np.float64).sum() - float(z["input_sum"])) < 1e-6 * max(1.0, abs(float(z["input_sum"])))
    np.testing.assert_array_equal(x.reshape(-1)[:16], z["input_head"])
    emb, inter, emb_d = ref_runs(path)
    _assert_emb(emb.numpy(), z["embed"])
    _assert_emb(emb_d.numpy(), z["embed_deploy"])
    _assert_emb(emb_d.numpy(), z["embed"])  # the two forms are one model
    # recorded sums of the stage outputs: f32 tensors summed in f64: 1e-5 of the abs-sum (+ 1e-4 absolute)
    for tag in repvgg_ref.TAPS:
        t = inter[tag].double()
        a = float(z["abs_" + tag])
        assert abs(float(t.abs().sum()) - a) <= 1e-5 * a + 1e-4, tag
        assert abs(float(t.sum()) - float(z["sum_" + tag])) <= 1e-5 * a + 1e-4, tag


@pytest.mark.parametrize("path", SHORT, ids=[os.path.basename(p)[:-4] for p in SHORT])
def test_ref_in_float64_matches_both_fixture_embeddings(path):
    """The float64 evaluation of either form against the reference's float32 embeddings, and the two forms
    against each other: they differ only by the float32 rounding of the folded weights."""
    z, spec, _, sd, x = load_case(path)
    e64 = repvgg_ref.forward(x, sd, spec.arch, dtype=torch.float64).numpy()
    d64 = repvgg_ref.forward(x, folded(path), spec.arch, dtype=torch.float64).numpy()
    _assert_emb(z["embed"], e64)
    _assert_emb(z["embed_deploy"], d64)
    assert np.abs(e64 - d64).max() < 2e-5
    assert np.abs(z["embed"].astype(np.float64) - z["embed_deploy"]).max() < 2e-5


def test_gflop_against_a_direct_mac_count():
    """repvgg_gflop_per_utt against the multiply-accumulates of every conv / linear call the restatement
    makes (deploy form: one conv per block, all k x k taps), and the sparse figure: lower by exactly 8 / 25 of
    the RepSPK convs' MACs."""
    for arch in ("REPVGG_A0", "REPVGG_RSBB_A2"):
        spec, _, sd, x = synth_case(arch, 5, 6, 1, 37, 40, 96)
        _, macs = repvgg_ref.forward(x, A.repvgg_fold(spec, sd), arch, macs=True)
        assert A.repvgg_gflop_per_utt(spec, 37, 0) == pytest.approx(2.0 * macs / 1e9, rel=1e-12)
        seg = 2 * 1408 * 5 * 96 if arch == "REPVGG_RSBB_A2" else 0
        if arch == "REPVGG_RSBB_A2":
            conv = macs - seg
            assert A.repvgg_gflop_per_utt(spec, 37, 1) == pytest.approx(2.0 * (macs - conv * 8 / 25) / 1e9, rel=1e-12)
        else:
            assert A.repvgg_gflop_per_utt(spec, 37, 1) == A.repvgg_gflop_per_utt(spec, 37, 0)


def test_registry_and_load_state_dict_report_against_the_selected_layout():
    for arch in A.REPVGG_ARCHS:
        m = get_speaker_model(arch)(feat_dim=80, embed_dim=256)
        assert isinstance(m, HipSpeakerModel) and m.spec.family == "repvgg" and not m.supports_segments
        assert m.state_dict_layout() == A.repvgg_params(m.spec)
    path = FIXTURES[IDS.index("repvgg_tiny_a0_f8_e64_b3_t9")]
    _, spec, _, sd, _ = load_case(path)
    f = folded(path)
    train = HipSpeakerModel(spec.arch, feat_dim=8, embed_dim=64)
    assert train.load_state_dict(sd) == ([], [])
    miss, unexp = train.load_state_dict(f)  # a deploy checkpoint into a training-form model
    assert "stage0.rbr_reparam.weight" in unexp and "seg.weight" not in unexp
    dep = HipSpeakerModel(spec.arch, feat_dim=8, embed_dim=64, deploy=True)
    assert len(dep.state_dict_layout()) == 70 and dep.load_state_dict(f) == ([], [])
    fresh = HipSpeakerModel(spec.arch, feat_dim=8, embed_dim=64, deploy=True)
    miss, unexp = fresh.load_state_dict(sd)  # and the reverse
    assert "stage0.rbr_reparam.weight" in miss and "stage0.rbr_dense.conv.weight" in unexp and "seg.weight" not in miss
    with pytest.raises(RuntimeError):
        fresh.load_state_dict(sd, strict=True)
    with pytest.raises(ValueError, match="size mismatch"):
        dep.load_state_dict({"stage0.rbr_reparam.weight": np.zeros((32, 1, 5, 5), np.float32)})


def test_convert_tool_round_trip(tmp_path):
    path = FIXTURES[IDS.index("repvgg_tiny_rsbb_a0_f8_e64_b3_t9")]
    _, spec, _, sd, _ = load_case(path)
    torch.save({"model": {"module." + k: torch.from_numpy(v) for k, v in sd.items()}}, tmp_path / "avg_model.pt")
    cfg = {"model": spec.arch, "exp_dir": str(tmp_path),
           "model_args": {"feat_dim": 8, "embed_dim": 64, "pooling_func": "TSTP", "deploy": False, "use_se": False},
           "dataset_args": {"num_frms": 200}}
    with open(tmp_path / "config.yaml", "w") as fh:
        yaml.safe_dump(cfg, fh)
    out = convert(str(tmp_path / "config.yaml"), str(tmp_path / "avg_model.pt"), str(tmp_path / "models" / "convert_model.pt"))
    assert out == str(tmp_path / "config.yaml")
    with open(out) as fh:
        new = yaml.safe_load(fh)
    assert new["model_args"] == dict(cfg["model_args"], deploy=True) and new["dataset_args"] == cfg["dataset_args"]
    state = torch.load(tmp_path / "models" / "convert_model.pt", weights_only=True)
    m = get_speaker_model(new["model"])(**new["model_args"])
    assert m.spec.family == "repvgg" and m.spec.deploy
    assert [(k, tuple(v.shape)) for k, v in state.items()] == [(n, tuple(s)) for n, s in m.state_dict_layout()]
    assert m.load_state_dict(state, strict=True) == ([], [])
    for k, v in folded(path).items():
        np.testing.assert_array_equal(state[k].numpy(), v)
    # a deploy checkpoint is not something to convert
    with pytest.raises(KeyError, match="training-form"):
        convert(out, str(tmp_path / "models" / "convert_model.pt"), str(tmp_path / "again.pt"))
