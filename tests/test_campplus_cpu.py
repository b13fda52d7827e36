"""CAM++ (CAMPPlus) without a GPU: the parameter table (arch.py and the library's), the torch-CPU
restatement tests/campplus_ref.py against the fixtures made from the reference module
(tests/golden/make_campplus_golden.py), and the host-side surface (registry, refusals, workspace
query)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import campplus_ref  # noqa: E402
from campplus_cases import FIXTURES, IDS, load_case  # noqa: E402
from wespeaker_hubert_amd import _lib  # noqa: E402
from wespeaker_hubert_amd import arch as A  # noqa: E402
from wespeaker_hubert_amd.speaker_model import HipSpeakerModel, get_speaker_model  # noqa: E402

TAPS = ("head", "tdnn", "block1", "transit1", "block2", "transit2", "block3", "transit3")


_RUNS = {}


def ref_runs(path):
    """(f32 embedding, its intermediates, f64 embedding) of one fixture, computed once."""
    if path not in _RUNS:
        _, _, _, sd, x = load_case(path)
        e32, inter = campplus_ref.forward(x, sd, taps=True)
        e64 = campplus_ref.forward(x, sd, dtype=torch.float64)
        _RUNS[path] = (e32, inter, e64)
    return _RUNS[path]


def test_the_five_fixtures_exist():
    assert len(FIXTURES) == 5, FIXTURES


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_param_layout_matches_reference(path):
    z, spec, plist, _, _ = load_case(path)
    assert A.param_list(spec) == plist and spec.family == "campplus"
    assert len(plist) == 937
    assert [n for n, _ in plist] == [str(n) for n in z["param_names"]]
    assert [tuple(s) for _, s in plist] == [tuple(int(s) for s in str(v).split(",") if s) for v in z["param_shapes"]]


def test_parameter_count_of_the_hub_model():
    plist = A.campplus_params(A.make_spec("CAMPPlus"))
    assert sum(int(np.prod(s)) for _, s in plist) == 7259162


@pytest.mark.parametrize("feat_dim", [80, 40, 8])
def test_library_table_matches_arch(feat_dim):
    lib = _lib.load()
    want = A.campplus_params(A.make_spec("CAMPPlus", feat_dim=feat_dim, embed_dim=192))
    h = ctypes.c_void_p()
    assert lib.wsp_model_create(b"CAMPPlus", feat_dim, 192, 0, 0, ctypes.byref(h)) == 0, lib.wsp_last_error()
    try:
        assert lib.wsp_model_num_params(h) == len(want)
        name, ndim, shape = ctypes.c_char_p(), ctypes.c_int(), (ctypes.c_int64 * 4)()
        for i, (n, s) in enumerate(want):
            assert lib.wsp_model_param_info(h, i, ctypes.byref(name), ctypes.byref(ndim), shape) == 0
            assert name.value.decode() == n
            assert tuple(shape[d] for d in range(ndim.value)) == tuple(s), n
    finally:
        lib.wsp_model_destroy(h)


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_ref_matches_reference_forward(path):
    z, _, _, _, x = load_case(path)
    assert abs(x.astype(np.float64).sum() - float(z["input_sum"])) < 1e-6 * max(1.0, abs(float(z["input_sum"])))
    np.testing.assert_array_equal(x.reshape(-1)[:16], z["input_head"])
    emb, inter, _ = ref_runs(path)
    assert emb.shape == z["embed"].shape and torch.isfinite(emb).all()
    np.testing.assert_allclose(emb.numpy(), z["embed"], atol=2e-5, rtol=0)
    # recorded sums of the intermediates: f32 tensors summed in f64, so the two f32 evaluations
    # may differ by a few ulps per element: 1e-5 of the abs-sum (+ 1e-4 absolute)
    for tag in TAPS:
        t = inter[tag].double()
        a = float(z["abs_" + tag])
        assert abs(float(t.abs().sum()) - a) <= 1e-5 * a + 1e-4, tag
        assert abs(float(t.sum()) - float(z["sum_" + tag])) <= 1e-5 * a + 1e-4, tag
    fl = inter["frame_level"]
    np.testing.assert_allclose(fl[:, 0].numpy(), z["frame_first"], atol=2e-5, rtol=1e-5)
    np.testing.assert_allclose(fl[:, -1].numpy(), z["frame_last"], atol=2e-5, rtol=1e-5)


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_float64_run_guards_the_seeds(path):
    e32, _, e64 = ref_runs(path)
    assert e64.dtype == torch.float64
    assert float((e32.double() - e64).abs().max()) < 1e-5


def test_registry_and_refusals():
    m = get_speaker_model("CAMPPlus")()
    assert isinstance(m, HipSpeakerModel)
    assert (m.spec.feat_dim, m.spec.embed_dim, m.spec.pooling_func, m.spec.family) == (80, 512, "TSTP", "campplus")
    assert not m.supports_segments
    assert len(m.state_dict_layout()) == 937
    hub = get_speaker_model("CAMPPlus")(feat_dim=80, embed_dim=192, pooling_func="TSTP")
    assert hub.spec.embed_dim == 192
    with pytest.raises(NotImplementedError):
        get_speaker_model("CAMPPlus")(pooling_func="ASTP")
    with pytest.raises(ValueError, match="multiple of 8"):
        get_speaker_model("CAMPPlus")(feat_dim=60)
    assert A.campplus_gflop_per_utt(A.make_spec("CAMPPlus"), 498) == pytest.approx(5.345, abs=0.01)


def test_library_refusals_and_workspace_query():
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.wsp_model_create(b"CAMPPlus", 60, 512, 0, 0, ctypes.byref(h)) != 0
    assert b"multiple of 8" in lib.wsp_last_error()
    assert lib.wsp_model_create(b"CAMPPlus", 0, 512, 0, 0, ctypes.byref(h)) != 0
    assert lib.wsp_model_create(b"CAMPPlus", 80, 0, 0, 0, ctypes.byref(h)) != 0
    assert lib.wsp_model_create(b"CAMPPlus", 80, 512, 1, 0, ctypes.byref(h)) != 0
    assert lib.wsp_model_create(b"CAMPPlus", 80, 512, 0, 1, ctypes.byref(h)) != 0
    assert lib.wsp_model_create(b"CAMPPlus", 80, 512, 0, 0, ctypes.byref(h)) == 0
    try:
        b = ctypes.c_size_t()
        assert lib.wsp_model_workspace_bytes(h, 1024, 1000, ctypes.byref(b)) == 0, lib.wsp_last_error()
        # at least the stem's output of one 2 GiB-capped chunk, and no 32-bit wrap
        small = ctypes.c_size_t()
        assert lib.wsp_model_workspace_bytes(h, 2, 200, ctypes.byref(small)) == 0
        assert b.value > (1 << 32) and b.value > 100 * small.value
        assert b.value < 1024 * 1000 * 80 * 32 * 4 * 4  # chunked: far below four whole-batch stem images
        v = ctypes.c_int(-1)
        assert lib.wsp_model_get_option(h, b"streams", ctypes.byref(v)) == 0 and v.value == 1
        assert lib.wsp_model_get_option(h, b"cam_fused", ctypes.byref(v)) == 0 and v.value == 1
        assert lib.wsp_model_set_option(h, b"cam_fused", 2) != 0
    finally:
        lib.wsp_model_destroy(h)
