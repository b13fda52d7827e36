"""Res2Net (Res2Net34_Base, Res2Net34_Large) without a GPU: the parameter table (arch.py and the
library's), the torch-CPU restatement tests/res2net_ref.py against the fixtures made from the
reference module (tests/golden/make_res2net_golden.py), that the two x 8 fixtures exercise the clamp,
the host-side surface (registry, defaults, refusals, option res2_tail) and the operand-chunk rule
through the workspace query."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import res2net_ref  # noqa: E402
from res2net_cases import FIXTURES, IDS, load_case  # noqa: E402
from wespeaker_hubert_amd import _lib  # noqa: E402
from wespeaker_hubert_amd import arch as A  # noqa: E402
from wespeaker_hubert_amd.speaker_model import HipSpeakerModel, get_speaker_model  # noqa: E402

X8 = [p for p in FIXTURES if p.endswith("_x8.npz")]

_RUNS = {}


def ref_runs(path):
    """(f32 embedding, its intermediates) of one fixture, computed once."""
    if path not in _RUNS:
        _, spec, _, sd, x = load_case(path)
        _RUNS[path] = res2net_ref.forward(x, sd, spec.arch, spec.two_emb_layer, taps=True)
    return _RUNS[path]


def test_the_seven_fixtures_exist():
    assert len(FIXTURES) == 7 and len(X8) == 2, FIXTURES
    for p in FIXTURES:
        assert os.path.getsize(p) < (1 << 20)
    for p in X8:  # the generator's own count: the ceiling is reached at the output of at least two stages
        assert int((np.load(p)["at20"] > 0).sum()) >= 2


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_param_layout_matches_reference(path):
    z, spec, plist, _, _ = load_case(path)
    assert A.param_list(spec) == plist and spec.family == "res2net"
    assert [n for n, _ in plist] == [str(n) for n in z["param_names"]]
    assert [tuple(s) for _, s in plist] == [tuple(int(s) for s in str(v).split(",") if s) for v in z["param_shapes"]]


def test_tensor_counts_and_disjoint_names():
    n = {(a, t): len(A.res2net_params(A.make_spec(a, two_emb_layer=t))) for a in A.RES2NET_ARCHS for t in (False, True)}
    assert n[("Res2Net34_Base", False)] == n[("Res2Net34_Large", False)] == 320
    assert n[("Res2Net34_Base", True)] == n[("Res2Net34_Large", True)] == 325
    assert not set(A.RES2NET_ARCHS) & set(A.ERES2NET_ARCHS)
    assert A.make_spec("ERes2Net34_Base").family == "eres2net" and A.make_spec("ResNet34").family == "resnet"
    # seg_1 is sized for int(feat_dim / 8) rows of 2 * 8 m channels, mean and std
    assert dict(A.res2net_params(A.make_spec("Res2Net34_Large", feat_dim=40, embed_dim=7)))["seg_1.weight"] == (
        7, 2 * 5 * 64 * 8 * 2)


def _create(arch, feat_dim, embed_dim, emb_bn=0, two_emb=0):
    lib = _lib.load()
    h = ctypes.c_void_p()
    rc = lib.wsp_model_create(arch.encode(), feat_dim, embed_dim, emb_bn, int(two_emb), ctypes.byref(h))
    return lib, h, rc


def _library_table(arch, feat_dim, embed_dim, two_emb):
    lib, h, rc = _create(arch, feat_dim, embed_dim, 0, two_emb)
    assert rc == 0, lib.wsp_last_error()
    try:
        name, ndim, shape = ctypes.c_char_p(), ctypes.c_int(), (ctypes.c_int64 * 4)()
        out = []
        for i in range(lib.wsp_model_num_params(h)):
            assert lib.wsp_model_param_info(h, i, ctypes.byref(name), ctypes.byref(ndim), shape) == 0
            out.append((name.value.decode(), tuple(shape[d] for d in range(ndim.value))))
        return out
    finally:
        lib.wsp_model_destroy(h)


@pytest.mark.parametrize("arch,feat_dim,embed_dim,two_emb", [
    ("Res2Net34_Base", 80, 256, False), ("Res2Net34_Base", 40, 256, True), ("Res2Net34_Large", 80, 192, False)])
def test_library_table_matches_arch(arch, feat_dim, embed_dim, two_emb):
    want = A.res2net_params(A.make_spec(arch, feat_dim=feat_dim, embed_dim=embed_dim, two_emb_layer=two_emb))
    assert _library_table(arch, feat_dim, embed_dim, two_emb) == [(n, tuple(s)) for n, s in want]


def test_library_refusals_and_res2_tail():
    lib, h, rc = _create("Res2Net34_X", 80, 256)
    assert rc != 0 and b"unsupported arch" in lib.wsp_last_error()
    lib, h, rc = _create("Res2Net34_Base", 84, 256)
    assert rc != 0 and b"multiple of 8" in lib.wsp_last_error()
    assert _create("Res2Net34_Base", 80, 0)[2] != 0
    assert _create("Res2Net34_Base", 80, 256, emb_bn=1)[2] != 0
    lib, h, rc = _create("Res2Net34_Base", 80, 256)
    assert rc == 0
    try:
        v = ctypes.c_int(-1)
        assert lib.wsp_model_get_option(h, b"res2_tail", ctypes.byref(v)) == 0 and v.value == 1
        assert lib.wsp_model_set_option(h, b"res2_tail", 3) != 0
        assert b"res2_tail must be 0" in lib.wsp_last_error()
        assert lib.wsp_model_set_option(h, b"res2_tail", -1) != 0
        for val in (0, 2, 1):
            assert lib.wsp_model_set_option(h, b"res2_tail", val) == 0
            assert lib.wsp_model_get_option(h, b"res2_tail", ctypes.byref(v)) == 0 and v.value == val
    finally:
        lib.wsp_model_destroy(h)
    lib, h, rc = _create("ERes2Net34_Base", 80, 256)  # the key is refused on handles that do not own it
    assert rc == 0
    try:
        assert lib.wsp_model_set_option(h, b"res2_tail", 0) != 0
        assert b"Res2Net handles" in lib.wsp_last_error()
    finally:
        lib.wsp_model_destroy(h)


def test_operand_chunks_through_the_workspace_query():
    """Base at T = 1000: a stage-1 block output is 80 x 1000 x 64 floats = 20.48 MB per utterance and the
    operand cap is 7/8 of 2 GiB, so 91 utterances are one chunk, 92 two chunks of 46 and 128 two of 64.
    The workspace depends on the chunk size alone, which the query shows without a device."""
    lib, h, rc = _create("Res2Net34_Base", 80, 256)
    assert rc == 0
    try:
        def ws(B):
            b = ctypes.c_size_t()
            assert lib.wsp_model_workspace_bytes(h, B, 1000, ctypes.byref(b)) == 0, lib.wsp_last_error()
            return b.value
        assert ws(128) == ws(64) and ws(92) == ws(46) and ws(46) < ws(64) < ws(91)
        assert (1 << 32) < ws(128) < 128 * 1000 * 80 * 64 * 4 * 3  # no 32-bit wrap, far below whole-batch buffers
        per_utt = (ws(64) - ws(46)) / 18.0
        assert 3 * 20.48e6 < per_utt < 5 * 20.48e6  # X, O, SC + Y1 (1/2) + S (1/4) of 20.48 MB
    finally:
        lib.wsp_model_destroy(h)


def test_make_spec_defaults_and_refusals():
    s = A.make_spec("Res2Net34_Base")
    assert (s.feat_dim, s.embed_dim, s.pooling_func, s.two_emb_layer, s.family, s.m_channels) == (
        80, 192, "TSTP", False, "res2net", 32)
    assert A.make_spec("Res2Net34_Large", embed_dim=256, two_emb_layer=True).two_emb_layer
    assert A.make_spec("Res2Net34_Large").m_channels == 64
    with pytest.raises(NotImplementedError):
        A.make_spec("Res2Net34_Base", pooling_func="ASTP")
    with pytest.raises(ValueError, match="multiple of 8"):
        A.make_spec("Res2Net34_Large", feat_dim=84)
    with pytest.raises(TypeError):
        A.make_spec("Res2Net34_Base", emb_bn=True)
    with pytest.raises(KeyError):
        A.make_spec("Res2Net34_X")


def test_registry_round_trip():
    for arch in A.RES2NET_ARCHS:
        m = get_speaker_model(arch)(feat_dim=80, embed_dim=256)
        assert isinstance(m, HipSpeakerModel) and m.spec.family == "res2net" and not m.supports_segments
        assert m.spec.arch == arch and m.state_dict_layout() == A.res2net_params(m.spec)
    assert len(get_speaker_model("Res2Net34_Base")().state_dict_layout()) == 320
    with pytest.raises(KeyError):
        get_speaker_model("Res2Net34_X")


def test_gflop_against_a_direct_mac_count():
    """res2net_gflop_per_utt against the multiply-accumulates of every conv / linear call the functional
    restatement makes at one shape (Large, two_emb_layer, feat 40, T = 37: odd planes at every level)."""
    spec = A.make_spec("Res2Net34_Large", feat_dim=40, embed_dim=96, two_emb_layer=True)
    from wespeaker_hubert_amd.synthetic import synth_feats, synth_state_dict
    sd = synth_state_dict(5, A.res2net_params(spec), residual_tame=True)
    _, macs = res2net_ref.forward(synth_feats(6, 1, 37, 40), sd, spec.arch, True, macs=True)
    assert A.res2net_gflop_per_utt(spec, 37) == pytest.approx(2.0 * macs / 1e9, rel=1e-12)


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_ref_matches_reference_forward(path):
    z, _, _, _, x = load_case(path)
    assert abs(x.astype(np.float64).sum() - float(z["input_sum"])) < 1e-6 * max(1.0, abs(float(z["input_sum"])))
    np.testing.assert_array_equal(x.reshape(-1)[:16], z["input_head"])
    emb, inter = ref_runs(path)
    assert emb.shape == z["embed"].shape and torch.isfinite(emb).all()
    # the bars of test_eres2net_cpu.py for the same comparison
    np.testing.assert_allclose(emb.numpy(), z["embed"], atol=2e-5, rtol=0)
    # recorded sums of the intermediates: f32 tensors summed in f64, so the two f32 evaluations
    # may differ by a few ulps per element: 1e-5 of the abs-sum (+ 1e-4 absolute)
    for tag in res2net_ref.TAPS:
        t = inter[tag].double()
        a = float(z["abs_" + tag])
        assert abs(float(t.abs().sum()) - a) <= 1e-5 * a + 1e-4, tag
        assert abs(float(t.sum()) - float(z["sum_" + tag])) <= 1e-5 * a + 1e-4, tag


@pytest.mark.parametrize("path", [p for p in FIXTURES if "_t37" in p or "_t9" in p or "_t50" in p],
                         ids=[i for i in IDS if "_t37" in i or "_t9" in i or "_t50" in i])
def test_ref_in_float64_matches_reference_forward(path):
    """The float64 evaluation of the restatement against the (f32) fixture embedding, same bar."""
    z, spec, _, sd, x = load_case(path)
    emb = res2net_ref.forward(x, sd, spec.arch, spec.two_emb_layer, dtype=torch.float64)
    np.testing.assert_allclose(emb.numpy(), z["embed"].astype(np.float64), atol=2e-5, rtol=0)


@pytest.mark.parametrize("path", X8, ids=[os.path.basename(p)[:-4] for p in X8])
def test_x8_inputs_exercise_the_clamp(path):
    """Without the ceiling at 20 the embedding moves by more than 100 x the GPU test's tolerance
    (1e-4 x rms of the reference embedding): the x 8 cases test the clamp."""
    z, spec, _, sd, x = load_case(path)
    emb, inter = ref_runs(path)
    assert sum(int((inter[f"layer{li}"] == 20.0).any()) for li in (1, 2, 3, 4)) >= 2
    relu = res2net_ref.forward(x, sd, spec.arch, spec.two_emb_layer, clamp=False)
    rms = float(np.sqrt((z["embed"].astype(np.float64) ** 2).mean()))
    assert float((emb - relu).abs().max()) > 100 * 1e-4 * rms
