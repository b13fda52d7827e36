"""ERes2Net (Base, Large, aug) without a GPU: the parameter table (arch.py and the library's), the
torch-CPU restatement tests/eres2net_ref.py against the fixtures made from the reference module
(tests/golden/make_eres2net_golden.py), that the two x 8 fixtures exercise the clamp, and the
host-side surface (registry, defaults, refusals)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import eres2net_ref  # noqa: E402
from eres2net_cases import FIXTURES, IDS, load_case  # noqa: E402
from wespeaker_hubert_amd import _lib  # noqa: E402
from wespeaker_hubert_amd import arch as A  # noqa: E402
from wespeaker_hubert_amd.speaker_model import HipSpeakerModel, get_speaker_model  # noqa: E402

X8 = [p for p in FIXTURES if p.endswith("_x8.npz")]

_RUNS = {}


def ref_runs(path):
    """(f32 embedding, its intermediates) of one fixture, computed once."""
    if path not in _RUNS:
        _, spec, _, sd, x = load_case(path)
        _RUNS[path] = eres2net_ref.forward(x, sd, spec.arch, spec.two_emb_layer, taps=True)
    return _RUNS[path]


def test_the_eight_fixtures_exist():
    assert len(FIXTURES) == 8 and len(X8) == 2, FIXTURES


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_param_layout_matches_reference(path):
    z, spec, plist, _, _ = load_case(path)
    assert A.param_list(spec) == plist and spec.family == "eres2net"
    assert [n for n, _ in plist] == [str(n) for n in z["param_names"]]
    assert [tuple(s) for _, s in plist] == [tuple(int(s) for s in str(v).split(",") if s) for v in z["param_shapes"]]


def test_tensor_counts():
    n = {(a, t): len(A.eres2net_params(A.make_spec(a, two_emb_layer=t)))
         for a in A.ERES2NET_ARCHS for t in (False, True)}
    assert n[("ERes2Net34_Base", False)] == n[("ERes2Net34_Large", False)] == 587
    assert n[("ERes2Net34_Base", True)] == 592
    assert n[("ERes2Net34_aug", False)] == 809


def _library_table(arch, feat_dim, embed_dim, two_emb):
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.wsp_model_create(arch.encode(), feat_dim, embed_dim, 0, int(two_emb), ctypes.byref(h)) == 0, \
        lib.wsp_last_error()
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
    ("ERes2Net34_Base", 80, 512, False), ("ERes2Net34_Base", 40, 256, True), ("ERes2Net34_Large", 80, 512, False),
    ("ERes2Net34_aug", 80, 192, False)])
def test_library_table_matches_arch(arch, feat_dim, embed_dim, two_emb):
    want = A.eres2net_params(A.make_spec(arch, feat_dim=feat_dim, embed_dim=embed_dim, two_emb_layer=two_emb))
    assert _library_table(arch, feat_dim, embed_dim, two_emb) == [(n, tuple(s)) for n, s in want]


def test_library_refusals():
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.wsp_model_create(b"ERes2Net34_X", 80, 512, 0, 0, ctypes.byref(h)) != 0
    assert b"unsupported arch" in lib.wsp_last_error()
    assert lib.wsp_model_create(b"ERes2Net34_Base", 60, 512, 0, 0, ctypes.byref(h)) != 0
    assert b"multiple of 8" in lib.wsp_last_error()
    assert lib.wsp_model_create(b"ERes2Net34_Base", 80, 0, 0, 0, ctypes.byref(h)) != 0
    assert lib.wsp_model_create(b"ERes2Net34_Base", 80, 512, 1, 0, ctypes.byref(h)) != 0
    assert lib.wsp_model_create(b"ERes2Net34_Base", 80, 512, 0, 0, ctypes.byref(h)) == 0
    try:
        # B = 128 x T = 1000 is chunked: far below whole-batch buffers, and no 32-bit wrap
        b = ctypes.c_size_t()
        assert lib.wsp_model_workspace_bytes(h, 128, 1000, ctypes.byref(b)) == 0, lib.wsp_last_error()
        assert (1 << 32) < b.value < 128 * 1000 * 80 * 64 * 4 * 3
    finally:
        lib.wsp_model_destroy(h)


def test_make_spec_defaults_and_refusals():
    s = A.make_spec("ERes2Net34_Base")
    assert (s.feat_dim, s.embed_dim, s.pooling_func, s.two_emb_layer, s.family) == (80, 192, "TSTP", False, "eres2net")
    assert A.make_spec("ERes2Net34_aug", embed_dim=512, two_emb_layer=True).two_emb_layer
    with pytest.raises(NotImplementedError):
        A.make_spec("ERes2Net34_Base", pooling_func="ASTP")
    with pytest.raises(ValueError, match="multiple of 8"):
        A.make_spec("ERes2Net34_Large", feat_dim=60)
    with pytest.raises(KeyError):
        A.make_spec("ERes2Net34_X")


def test_registry():
    for arch in A.ERES2NET_ARCHS:
        m = get_speaker_model(arch)(feat_dim=80, embed_dim=512)
        assert isinstance(m, HipSpeakerModel) and m.spec.family == "eres2net" and not m.supports_segments
    assert len(get_speaker_model("ERes2Net34_Base")().state_dict_layout()) == 587
    # 2 x MACs of the recipe shape: 6.72 GFLOP per 200-frame utterance (Base), 62.5 (aug)
    assert A.eres2net_gflop_per_utt(A.make_spec("ERes2Net34_Base", embed_dim=512), 200) == pytest.approx(6.72, abs=0.01)
    assert A.eres2net_gflop_per_utt(A.make_spec("ERes2Net34_aug"), 200) == pytest.approx(62.49, abs=0.01)


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_ref_matches_reference_forward(path):
    z, _, _, _, x = load_case(path)
    assert abs(x.astype(np.float64).sum() - float(z["input_sum"])) < 1e-6 * max(1.0, abs(float(z["input_sum"])))
    np.testing.assert_array_equal(x.reshape(-1)[:16], z["input_head"])
    emb, inter = ref_runs(path)
    assert emb.shape == z["embed"].shape and torch.isfinite(emb).all()
    # the tolerance of test_campplus_cpu.py for the same comparison (the x 8 embeddings are 11 x
    # larger and still meet it)
    np.testing.assert_allclose(emb.numpy(), z["embed"], atol=2e-5, rtol=0)
    # recorded sums of the intermediates: f32 tensors summed in f64, so the two f32 evaluations
    # may differ by a few ulps per element: 1e-5 of the abs-sum (+ 1e-4 absolute)
    for tag in eres2net_ref.TAPS:
        t = inter[tag].double()
        a = float(z["abs_" + tag])
        assert abs(float(t.abs().sum()) - a) <= 1e-5 * a + 1e-4, tag
        assert abs(float(t.sum()) - float(z["sum_" + tag])) <= 1e-5 * a + 1e-4, tag


@pytest.mark.parametrize("path", X8, ids=[os.path.basename(p)[:-4] for p in X8])
def test_x8_inputs_exercise_the_clamp(path):
    """Without the ceiling at 20 the embedding moves by more than 100 x the GPU test's tolerance
    (1e-4 x rms of the reference embedding): the x 8 cases test the clamp."""
    z, spec, _, sd, x = load_case(path)
    emb, _ = ref_runs(path)
    relu = eres2net_ref.forward(x, sd, spec.arch, spec.two_emb_layer, clamp=False)
    rms = float(np.sqrt((z["embed"].astype(np.float64) ** 2).mean()))
    assert float((emb - relu).abs().max()) > 100 * 1e-4 * rms
