"""Gemini DF-ResNet (60 / 114 / 183 / 237) without a GPU: the parameter table (arch.py and the
library's), the host-side surface (registry, defaults, refusals, option ib_fused), the
multiply-accumulate count, the torch-CPU restatement tests/gemini_ref.py against the fixtures made
from the reference module (tests/golden/make_gemini_golden.py), and the op test's tail allowance
against an f32 emulation of the kernel's arithmetic and against wrong variants of it."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import conv_gemm_ref as ref  # noqa: E402
import gemini_ref  # noqa: E402
import test_gpu_gemini_op as op  # noqa: E402  (cases, float64 references and allowances; nothing runs on import)
from gemini_cases import FIXTURES, IDS, load_case  # noqa: E402
from wespeaker_hubert_amd import _lib  # noqa: E402
from wespeaker_hubert_amd import arch as A  # noqa: E402
from wespeaker_hubert_amd.speaker_model import HipSpeakerModel, get_speaker_model  # noqa: E402

COUNTS = {"Gemini_DF_ResNet60": 356, "Gemini_DF_ResNet114": 680, "Gemini_DF_ResNet183": 1094, "Gemini_DF_ResNet237": 1418}
IB_FUSED_DEFAULT = 0  # the three-launch route is the faster one


def test_the_six_fixtures_exist():
    assert len(FIXTURES) == 6, FIXTURES
    assert {str(np.load(p)["arch"]) for p in FIXTURES} == set(COUNTS)


def test_make_spec_defaults_and_refusals():
    s = A.make_spec("Gemini_DF_ResNet114", feat_dim=80)
    assert (s.feat_dim, s.embed_dim, s.pooling_func, s.two_emb_layer, s.family) == (80, 128, "TSTP", False, "gemini")
    assert A.make_spec("Gemini_DF_ResNet60", feat_dim=16, embed_dim=64, two_emb_layer=True).two_emb_layer
    with pytest.raises(NotImplementedError):
        A.make_spec("Gemini_DF_ResNet114", feat_dim=80, pooling_func="ASTP")
    with pytest.raises(ValueError, match="multiple of 16"):
        A.make_spec("Gemini_DF_ResNet114", feat_dim=40)
    with pytest.raises(ValueError, match="multiple of 16"):
        A.make_spec("Gemini_DF_ResNet114")  # the reference's class default, feat_dim 40, is one of them
    with pytest.raises(KeyError):
        A.make_spec("Gemini_DF_ResNet99")
    assert set(A.GEMINI_ARCHS).isdisjoint(A.RESNET_ARCHS)


def test_registry():
    for arch, n in COUNTS.items():
        m = get_speaker_model(arch)(feat_dim=80, embed_dim=256)
        assert isinstance(m, HipSpeakerModel) and m.spec.family == "gemini" and not m.supports_segments
        assert len(m.state_dict_layout()) == n
        assert len(get_speaker_model(arch)(feat_dim=80, embed_dim=256, two_emb_layer=True).state_dict_layout()) == n + 5
    with pytest.raises(KeyError):
        get_speaker_model("Gemini_DF_ResNet99")


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_param_layout_matches_reference(path):
    z, spec, plist, _, _ = load_case(path)
    assert A.param_list(spec) == plist and spec.family == "gemini"
    assert [n for n, _ in plist] == [str(n) for n in z["param_names"]]
    assert [tuple(s) for _, s in plist] == [tuple(int(s) for s in str(v).split(",") if s) for v in z["param_shapes"]]
    assert len(plist) == COUNTS[spec.arch] + 5 * spec.two_emb_layer


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


@pytest.mark.parametrize("two_emb", (False, True))
@pytest.mark.parametrize("arch", sorted(COUNTS))
def test_library_table_matches_arch(arch, two_emb):
    want = A.param_list(A.make_spec(arch, feat_dim=80, embed_dim=192, two_emb_layer=two_emb))
    assert _library_table(arch, 80, 192, two_emb) == [(n, tuple(s)) for n, s in want]


def test_library_refusals_and_ib_fused():
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.wsp_model_create(b"Gemini_DF_ResNet99", 80, 256, 0, 0, ctypes.byref(h)) != 0
    assert b"unsupported arch" in lib.wsp_last_error()
    assert lib.wsp_model_create(b"Gemini_DF_ResNet114", 40, 256, 0, 0, ctypes.byref(h)) != 0
    assert b"multiple of 16" in lib.wsp_last_error()
    assert lib.wsp_model_create(b"Gemini_DF_ResNet114", 80, 0, 0, 0, ctypes.byref(h)) != 0
    assert lib.wsp_model_create(b"Gemini_DF_ResNet114", 80, 256, 1, 0, ctypes.byref(h)) != 0  # emb_bn
    assert lib.wsp_model_create(b"Gemini_DF_ResNet60", 80, 256, 0, 0, ctypes.byref(h)) == 0
    try:
        v, b = ctypes.c_int(), ctypes.c_size_t()
        assert lib.wsp_model_get_option(h, b"ib_fused", ctypes.byref(v)) == 0 and v.value == IB_FUSED_DEFAULT
        assert lib.wsp_model_set_option(h, b"ib_fused", 2) != 0
        assert b"ib_fused must be 0" in lib.wsp_last_error()
        assert lib.wsp_model_set_option(h, b"ib_fused", -1) != 0
        # the workspace follows the option: the three-launch route holds a second 4d-wide buffer
        # (128 channels x 40 rows x T floats per utterance at level 1)
        size = {}
        for fused in (0, 1):
            assert lib.wsp_model_set_option(h, b"ib_fused", fused) == 0
            assert lib.wsp_model_get_option(h, b"ib_fused", ctypes.byref(v)) == 0 and v.value == fused
            assert lib.wsp_model_workspace_bytes(h, 2, 200, ctypes.byref(b)) == 0, lib.wsp_last_error()
            size[fused] = b.value
        assert size[0] - size[1] == 2 * 128 * 40 * 200 * 4
        # B = 128 x T = 1000 is chunked (two chunks of 64): half of the whole-batch buffers (two d-wide
        # of 80 x T x 32 and one 4d-wide of 40 x T x 128 floats per utterance), no 32-bit wrap
        assert lib.wsp_model_workspace_bytes(h, 128, 1000, ctypes.byref(b)) == 0, lib.wsp_last_error()
        assert (1 << 31) < b.value < 128 * 1000 * (2 * 80 * 32 + 40 * 128) * 4 * 3 // 4
    finally:
        lib.wsp_model_destroy(h)


def _naive_gflop(spec, T):
    """2 x MACs from the parameter table alone: every conv weight's element count times the
    positions it is applied at, plus seg_1."""
    F, t = spec.feat_dim, T
    pos = {0: F * t}
    for li in range(4):
        F, t = (F - 1) // 2 + 1, (t - 1) // A.GEMINI_STRIDE_T[li] + 1
        pos[li + 1] = F * t
    macs = 0
    for name, shape in A.gemini_params(spec):
        if len(shape) != 4:
            continue
        part = name.split(".")
        level = int(part[1]) if part[0] == "downsample_layers" else int(part[1]) + 1
        macs += pos[level] * int(np.prod(shape))
    macs += 2 * F * 256 * spec.embed_dim
    return 2.0 * macs / 1e9


@pytest.mark.parametrize("arch", sorted(COUNTS))
def test_gflop_equals_a_naive_per_layer_count(arch):
    for feat_dim, embed_dim, T in ((80, 256, 200), (16, 64, 3), (32, 128, 37)):
        spec = A.make_spec(arch, feat_dim=feat_dim, embed_dim=embed_dim)
        assert A.gemini_gflop_per_utt(spec, T) == pytest.approx(_naive_gflop(spec, T), rel=1e-12)


def test_gflop_of_the_recipe_shape():
    spec = A.make_spec("Gemini_DF_ResNet114", feat_dim=80, embed_dim=256)
    assert A.gemini_gflop_per_utt(spec, 200) == pytest.approx(10.47, abs=0.01)


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_ref_matches_reference_forward(path):
    """gemini_ref against the fixture's embedding (<= 1e-6) and recorded sums.  Measured: 0 .. 7.5e-8
    on the host that made the fixtures; on a host whose torch takes other CPU convolution kernels
    (another summation order) 114 / 183 / 237 came out at 1.4e-6 / 1.2e-6 / 1.9e-6, the three
    Gemini60 fixtures inside the bound."""
    z, spec, _, sd, x = load_case(path)
    assert abs(x.astype(np.float64).sum() - float(z["input_sum"])) < 1e-6 * max(1.0, abs(float(z["input_sum"])))
    np.testing.assert_array_equal(x.reshape(-1)[:16], z["input_head"])
    emb, inter = gemini_ref.forward(x, sd, spec.arch, spec.two_emb_layer, taps=True)
    assert emb.shape == z["embed"].shape and torch.isfinite(emb).all()
    # the same ops in the same order: a few f32 ulps of O(1) embeddings
    np.testing.assert_allclose(emb.numpy(), z["embed"], atol=1e-6, rtol=0)
    # recorded sums of the intermediates: f32 tensors summed in f64, so the two f32 evaluations
    # may differ by a few ulps per element: 1e-5 of the abs-sum (+ 1e-4 absolute)
    for tag in gemini_ref.TAPS:
        t = inter[tag].double()
        a = float(z["abs_" + tag])
        assert abs(float(t.abs().sum()) - a) <= 1e-5 * a + 1e-4, tag
        assert abs(float(t.sum()) - float(z["sum_" + tag])) <= 1e-5 * a + 1e-4, tag


# ------------------------------------------------------------- the tail's op allowance --
def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32)


def emulate_tail(c, transpose_taps=False, neighbour_halo=False, drop_shift=False, drop_inner_relu=False,
                 res_after_relu=False):
    """The tail kernel's arithmetic in numpy: the depthwise conv as a chain of f32 fma over taps
    0..8 (each the f32 rounding of the exact w y + acc), the bias added last, ReLU; h split into
    bf16 hi / lo; per 32-long k-step the three products lo hi, hi lo, hi hi accumulated into an f32
    register one after the other; bias, residual and ReLU in f32.  The flags build wrong variants."""
    B, Fq, T, d, K, M = c["B"], c["F"], c["T"], c["d"], c["K"], c["M"]
    y = c["y"][:, c["yoff"]:c["yoff"] + K].astype(np.float64)
    if neighbour_halo:  # one tall plane: a row above / below an utterance is its neighbour's
        pad = np.zeros((1, B * Fq + 2, T + 2, K))
        pad[0, 1:-1, 1:-1] = y.reshape(B * Fq, T, K)
        window = lambda kf, kt: pad[0, kf:kf + B * Fq, kt:kt + T].reshape(M, K)  # noqa: E731
    else:
        pad = np.zeros((B, Fq + 2, T + 2, K))
        pad[:, 1:-1, 1:-1] = y.reshape(B, Fq, T, K)
        window = lambda kf, kt: pad[:, kf:kf + Fq, kt:kt + T].reshape(M, K)  # noqa: E731
    acc = np.zeros((M, K), np.float32)
    for tap in range(9):
        kf, kt = (tap % 3, tap // 3) if transpose_taps else (tap // 3, tap % 3)
        acc = _f32(c["w2"][tap].astype(np.float64) * window(kf, kt) + acc)
    h = acc if drop_shift else (acc + c["b2"]).astype(np.float32)
    if not drop_inner_relu:
        h = np.maximum(h, np.float32(0))
    hi = ref.to_bf16(h)
    lo = ref.to_bf16(h - hi)
    whi = ref.to_bf16(c["w3"])
    wlo = ref.to_bf16(c["w3"] - whi)
    out = np.zeros((M, d), np.float32)
    for k0 in range(0, K, 32):
        ks = slice(k0, k0 + 32)
        for a, w in ((hi, wlo), (lo, whi), (hi, whi)):  # mma3: w_lo h_hi, w_hi h_lo, w_hi h_hi
            out = _f32(a[:, ks].astype(np.float64) @ w[:, ks].astype(np.float64).T + out)
    resid = c["res"][:, c["roff"]:c["roff"] + d]
    out = (out + c["b3"]).astype(np.float32)
    if res_after_relu:
        return np.maximum(out, np.float32(0)) + resid
    return np.maximum((out + resid).astype(np.float32), np.float32(0))


_TAIL_CASES = [c for c in op.CASES if c["op"] == op.TAIL]
_TAIL_IDS = ["-".join(map(str, c["hdr"][:4])) + ("-strided" if c["ldy"] != c["K"] else "") for c in _TAIL_CASES]


@pytest.mark.parametrize("c", _TAIL_CASES, ids=_TAIL_IDS)
def test_emulated_tail_stays_inside_the_allowance(c):
    want, allow = op.tail_reference(c)
    err = (torch.from_numpy(emulate_tail(c)).double() - want).abs()
    ratio = float((err / allow).max())
    print(f"emulation: max |err| / allowance {ratio:.3f}")
    assert 0.0 < ratio <= 1.0


@pytest.mark.parametrize("variant", ("transpose_taps", "neighbour_halo", "drop_shift", "drop_inner_relu",
                                     "res_after_relu"))
def test_wrong_tails_exceed_the_allowance(variant):
    """Every wrong variant of the tail must fall outside the allowance, on the case with utterance
    and plane edges (B = 2, F = 3, T = 7, d = 32) and on its strided twin."""
    for c in (c for c in _TAIL_CASES if c["hdr"][:4] == [2, 3, 7, 32]):
        want, allow = op.tail_reference(c)
        err = (torch.from_numpy(emulate_tail(c, **{variant: True})).double() - want).abs()
        assert float((err / allow).max()) > 10.0, variant


def test_emulated_depthwise_conv_stays_inside_its_allowance():
    for c in (c for c in op.CASES if c["op"] == op.DW):
        want, delta = op.dw_reference(c)
        # the fma chain alone, as emulate_tail forms it
        B, Fq, T, K, M = c["B"], c["F"], c["T"], c["K"], c["M"]
        pad = np.zeros((B, Fq + 2, T + 2, K))
        pad[:, 1:-1, 1:-1] = c["y"][:, c["yoff"]:c["yoff"] + K].astype(np.float64).reshape(B, Fq, T, K)
        acc = np.zeros((M, K), np.float32)
        for tap in range(9):
            acc = _f32(c["w2"][tap].astype(np.float64) * pad[:, tap // 3:tap // 3 + Fq, tap % 3:tap % 3 + T].reshape(M, K) + acc)
        h = np.maximum((acc + c["b2"]).astype(np.float32), np.float32(0))
        assert float(((torch.from_numpy(h).double() - want).abs() / delta).max()) <= 1.0
