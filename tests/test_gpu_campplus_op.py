"""Op-level conformance of the four CAM++ kernels against float64 (tools/cam_dense_run).

The runner launches the shipped launchers of libwsp_hip.so (launch_cam_gemm, launch_cam_mask,
launch_cam_local, launch_fcm_conv) and holds no reference arithmetic; one run serves all tests.
Every output element of the three GEMM-like kernels is held to the bound tests/conv_gemm_ref.py
derives for bf16x3 products with f32 accumulation (imported, not restated):
    |y - ref| <= (2^-16 + (K + 8) 2^-24) S + 4 * 2^-24 (|y| + |y|)          S = sum |a| |w|
through each kernel's own f32 epilogue (1-Lipschitz ReLU, |scale|, 4 * 2^-24 of the magnitudes it
adds).  The GEMM's A operand is relu(fma(a, s1, t1)) rounded to f32 — what the prologue feeds the
hi / lo split — so the reference takes that f32 tensor as its operand.  Guard rows, guard columns
(the 32-column slice the local conv writes between live channels of the dense buffer) and guard
tails must come back bit-untouched.  The segment sums are held to the summed element bounds plus
16 * 2^-24 sum |y| for the f32 tree (depth 8 in a lane + 2 shuffles + 3 waves = 13 adds).

Context mask: float64 of the same path from the f32 segment sums, weights scaled so that the
sigmoid's argument stays within a few units of 0 (asserted: 1 < max |z| < 4).  Allowed: 4 f32 ulps
of the mask plus DEVICE_ERR = 4 x the largest excess over those 4 ulps measured on an MI355X
(ceiling 1e-6); the f32 arithmetic of the two small linears is part of what is measured.
Measured (MI355X, these seeds): max |device - float64| 1.275e-7 over the four mask cases (max |z| 2.53),
0.806 of the 4 ulps, excess over them 0 -> DEVICE_ERR 0.
max |err| / bound: cam_gemm .160 (segment sums .101), cam_local .061, fcm_conv .472.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import conv_gemm_ref as ref  # noqa: E402
import op_runner  # noqa: E402
from conv_gemm_ref import EPS24  # noqa: E402
from op_runner import untouched as _untouched  # noqa: E402

pytestmark = pytest.mark.gpu

MAGIC, SEG = 0x44505357, 100
MEASURED_MASK_EXCESS = 0.0
DEVICE_ERR = 4.0 * MEASURED_MASK_EXCESS
assert DEVICE_ERR < 1e-6


def nseg_of(T):
    return (T + SEG - 1) // SEG


# ------------------------------------------------------------------------------ cases --
def gemm_case(seed, M, T, K, N, lda, ldo, flags):
    rng = np.random.default_rng(seed)
    c = dict(op=1, hdr=[M, T, K, N, lda, ldo, flags], M=M, T=T, K=K, N=N, lda=lda, ldo=ldo, flags=flags)
    c["a"] = ref.rand_a(rng, M, lda, relu=not flags & 1)
    c["w"] = ref.rand_w(rng, N, K)
    if flags & 1:
        c["s1"] = rng.uniform(0.5, 1.5, K).astype(np.float32) * rng.choice([-1.0, 1.0], K).astype(np.float32)
        c["t1"] = rng.uniform(-0.3, 0.3, K).astype(np.float32)
    if flags & 2:
        c["s2"] = rng.uniform(0.5, 1.5, N).astype(np.float32)
        c["t2"] = rng.uniform(-0.3, 0.3, N).astype(np.float32)
    c["arrays"] = [c["a"], c["w"]] + [c[k] for k in ("s1", "t1", "s2", "t2") if k in c]
    return c


def mask_case(seed, B, T):
    rng = np.random.default_rng(seed)
    n = nseg_of(T)
    lens = np.array([min(SEG, T - SEG * q) for q in range(n)], dtype=np.float64)
    # sums of post-ReLU activations in [0, 1) over each segment's frames
    ss = (rng.uniform(0.0, 1.0, (B, n, 128)) * lens[None, :, None]).astype(np.float32)
    c = dict(op=2, hdr=[B, T], B=B, T=T, segsum=ss, w1=ref.rand_w(rng, 64, 128, amp=0.1), b1=ref.rand_w(rng, 64, amp=0.1),
             w2=ref.rand_w(rng, 32, 64, amp=0.3), b2=ref.rand_w(rng, 32, amp=0.3))
    c["arrays"] = [c[k] for k in ("segsum", "w1", "b1", "w2", "b2")]
    return c


def local_case(seed, M, T, dil, ldh, ldo, ocol):
    rng = np.random.default_rng(seed)
    c = dict(op=3, hdr=[M, T, dil, ldh, ldo, ocol], M=M, T=T, dil=dil, ldh=ldh, ldo=ldo, ocol=ocol)
    c["h"] = ref.rand_a(rng, M, ldh, relu=True)
    c["w"] = ref.rand_w(rng, 32, 128, 3)
    c["mask"] = rng.uniform(0.05, 0.95, ((M // T) * nseg_of(T), 32)).astype(np.float32)
    c["arrays"] = [c["h"], c["w"], c["mask"]]
    return c


def fcm_case(seed, B, Fi, T, relu, tfc, sc):
    rng = np.random.default_rng(seed)
    c = dict(op=4, hdr=[B, Fi, T, relu, tfc, sc], B=B, Fi=Fi, T=T, relu=relu, tfc=tfc, sc=sc)
    c["x"] = ref.rand_a(rng, B * Fi * T, 32, relu=True)
    c["w"] = ref.rand_w(rng, 32, 32, 3, 3)
    c["bias"] = ref.rand_w(rng, 32, amp=0.2)
    c["arrays"] = [c["x"], c["w"], c["bias"]]
    if sc:
        c["wsc"], c["bsc"] = ref.rand_w(rng, 32, 32, amp=0.2), ref.rand_w(rng, 32, amp=0.2)
        c["arrays"] += [c["wsc"], c["bsc"]]
    return c


CASES = [
    # GEMM: K = 128 and 992; M = 1, 101, 303; segment counts 1, 2, 3; wide lda / ldo; the
    # transit forms (N = 256 / 512, no epilogue / epilogue, dense 128-row tiles with a tail) and
    # the unfused form (no prologue)
    gemm_case(1, 1, 1, 128, 128, 160, 136, 7),
    gemm_case(2, 101, 101, 992, 128, 1024, 128, 7),
    gemm_case(3, 303, 101, 128, 128, 512, 128, 7),
    gemm_case(4, 250, 250, 992, 128, 1000, 132, 7),
    gemm_case(5, 4, 2, 160, 128, 512, 128, 7),
    gemm_case(6, 303, 101, 992, 256, 1024, 264, 1),
    gemm_case(7, 101, 101, 128, 512, 128, 512, 3),
    gemm_case(8, 101, 101, 128, 128, 132, 128, 6),
    mask_case(11, 3, 100), mask_case(12, 2, 101), mask_case(13, 1, 250), mask_case(14, 5, 2),
    # local conv: dilation 2 with T' = 2, M = 1 / 101 / 303, the slice between live columns
    local_case(21, 4, 2, 2, 128, 96, 32),
    local_case(22, 1, 1, 1, 128, 32, 0),
    local_case(23, 101, 101, 1, 128, 512, 416),
    local_case(24, 303, 101, 2, 136, 1024, 512),
    local_case(25, 250, 250, 2, 128, 64, 32),
    # strided conv: F = 8 -> 4 with and without the fused shortcut, F = 2 -> 1, frame-row output,
    # more than one block (600 > 512 positions), no ReLU
    fcm_case(31, 2, 8, 5, 1, 0, 1), fcm_case(32, 2, 8, 5, 1, 0, 0), fcm_case(33, 3, 2, 7, 1, 1, 0),
    fcm_case(34, 3, 8, 50, 1, 0, 1), fcm_case(35, 1, 6, 101, 0, 1, 0),
]


@pytest.fixture(scope="module")
def res(tmp_path_factory):
    """One runner process for all cases."""
    return op_runner.run("cam_dense_run", MAGIC, [(c["op"], c["hdr"], c["arrays"]) for c in CASES],
                         tmp_path_factory.mktemp("cam_dense"))


def _of(res, op):
    for c, r in zip(CASES, res):
        if c["op"] == op:
            assert r["status"] == 0, f"case {c['hdr']} refused: {r['message']}"
            yield c, r


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).double()


# ------------------------------------------------------------------------------ tests --
def test_bnrelu_prologue_gemm(res):
    worst = worst_sum = 0.0
    for c, r in _of(res, 1):
        M, T, K, N, lda, ldo, flags = c["hdr"]
        tag = f"gemm {c['hdr']}"
        a = c["a"][:, :K]
        if flags & 1:  # the prologue's f32 fma + max, as the kernel rounds it
            a = np.maximum((a.astype(np.float64) * c["s1"].astype(np.float64) + c["t1"].astype(np.float64))
                           .astype(np.float32), np.float32(0))
        rc = ref.make_case(a=[np.ascontiguousarray(a)], w=c["w"].reshape(N, K, 1), M=M, T=M, B=1)
        rr = ref.reference(rc)
        y, by = rr["out"], rr["bound"]
        if flags & 2:
            s2, t2 = _t(c["s2"]), _t(c["t2"])
            want = torch.clamp(y * s2 + t2, min=0.0)
            bound = s2.abs() * by + 4 * EPS24 * ((y * s2).abs() + t2.abs() + want.abs())
        else:
            want, bound = y, by
        raw = r["arrays"][0].reshape(M + 8, ldo)
        assert _untouched(raw[M:]), f"{tag}: guard rows written"
        assert _untouched(raw[:M, N:]), f"{tag}: guard columns written"
        got = _t(raw[:M, :N])
        assert torch.isfinite(got).all(), tag
        ratio = float(((got - want).abs() / bound).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{tag}: |err| / bound = {ratio:.3f}"
        if flags & 4:
            B, n = M // T, nseg_of(T)
            ss = r["arrays"][1]
            assert ss.size == B * n * N + 128 and _untouched(ss[B * n * N:]), f"{tag}: segment-sum guard written"
            gs = _t(ss[:B * n * N]).reshape(B, n, N)
            for b in range(B):
                for q in range(n):
                    rows = slice(b * T + q * SEG, b * T + min(T, (q + 1) * SEG))
                    ws, bs = want[rows].sum(0), bound[rows].sum(0) + 16 * EPS24 * want[rows].abs().sum(0)
                    rs = float(((gs[b, q] - ws).abs() / bs).max())
                    worst_sum = max(worst_sum, rs)
                    assert rs <= 1.0, f"{tag}: segment sums ({b}, {q}) |err| / bound = {rs:.3f}"
        else:
            assert r["arrays"][1].size == 0
    print(f"\ncam_gemm: max |err| / bound {worst:.3f}; segment sums {worst_sum:.3f}")
    assert worst > 0.0


def test_context_mask(res):
    worst = excess = dev = zmax = 0.0
    for c, r in _of(res, 2):
        B, T = c["hdr"]
        n = nseg_of(T)
        ss, w1, b1, w2, b2 = (_t(c[k]) for k in ("segsum", "w1", "b1", "w2", "b2"))
        lens = torch.tensor([min(SEG, T - SEG * q) for q in range(n)], dtype=torch.float64)
        ctx = ss.sum(1, keepdim=True) / T + ss / lens[None, :, None]          # [B][n][128]
        hid = torch.clamp(ctx @ w1.t() + b1, min=0.0)
        z = hid @ w2.t() + b2
        want = torch.sigmoid(z)
        zmax = max(zmax, float(z.abs().max()))
        ulps4 = 4 * 2.0 ** -23 * want
        raw = r["arrays"][0]
        assert raw.size == B * n * 32 + 32 and _untouched(raw[B * n * 32:]), "mask guard written"
        got = _t(raw[:B * n * 32]).reshape(B, n, 32)
        assert torch.isfinite(got).all() and float(got.min()) > 0.0 and float(got.max()) < 1.0
        err = (got - want).abs()
        dev = max(dev, float(err.max()))
        excess = max(excess, float((err - ulps4).clamp(min=0).max()))
        worst = max(worst, float((err / (ulps4 + DEVICE_ERR)).max()))
    print(f"\ncam_mask: max |device - float64| {dev:.3e}, excess over 4 f32 ulps {excess:.3e}, "
          f"max |err| / allowance {worst:.3f}, max |z| {zmax:.2f}")
    assert 1.0 < zmax < 4.0  # the sigmoid is exercised off its centre and nowhere saturated
    assert 4.0 * excess < 1e-6, f"device deviation {excess:.3e} is a finding (ceiling 1e-6 / 4)"
    assert worst <= 1.0


def test_masked_local_conv(res):
    worst = 0.0
    for c, r in _of(res, 3):
        M, T, dil, ldh, ldo, ocol = c["hdr"]
        tag = f"local {c['hdr']}"
        rc = ref.make_case(a=[c["h"]], w=c["w"], M=M, T=T, dil=dil, pad=dil)
        rr = ref.reference(rc)
        rows = np.arange(M)
        mk = _t(c["mask"])[(rows // T) * nseg_of(T) + (rows % T) // SEG]
        want = rr["out"] * mk
        bound = mk * rr["bound"] + 4 * EPS24 * want.abs()
        raw = r["arrays"][0].reshape(M + 8, ldo)
        assert _untouched(raw[M:]), f"{tag}: guard rows written"
        assert _untouched(raw[:M, :ocol]) and _untouched(raw[:M, ocol + 32:]), f"{tag}: columns beside the slice written"
        got = _t(raw[:M, ocol:ocol + 32])
        assert torch.isfinite(got).all(), tag
        ratio = float(((got - want).abs() / bound).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{tag}: |err| / bound = {ratio:.3f}"
    print(f"\ncam_local: max |err| / bound {worst:.3f}")
    assert worst > 0.0


def test_frequency_strided_conv(res):
    worst = 0.0
    for c, r in _of(res, 4):
        B, Fi, T, relu, tfc, sc = c["hdr"]
        tag = f"fcm {c['hdr']}"
        Fo = (Fi - 1) // 2 + 1
        x = _t(c["x"]).reshape(B, Fi, T, 32).permute(0, 3, 1, 2)

        def check(raw, w, bias, pad, act, rows_tfc, K):
            nonlocal worst
            y = F.conv2d(x, w, stride=(2, 1), padding=pad)
            S = F.conv2d(x.abs(), w.abs(), stride=(2, 1), padding=pad)
            assert y.shape == (B, 32, Fo, T)
            order = (0, 3, 2, 1) if rows_tfc else (0, 2, 3, 1)
            y, S = (v.permute(*order).reshape(-1, 32) for v in (y, S))
            pre = y + bias
            want = torch.clamp(pre, min=0.0) if act else pre
            bound = (2.0 ** -16 + (K + 8) * EPS24) * S + 4 * EPS24 * (y.abs() + bias.abs() + want.abs())
            n = B * Fo * T * 32
            assert raw.size == n + 256 and _untouched(raw[n:]), f"{tag}: guard tail written"
            got = _t(raw[:n]).reshape(-1, 32)
            assert torch.isfinite(got).all(), tag
            ratio = float(((got - want).abs() / bound).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, f"{tag}: |err| / bound = {ratio:.3f}"

        check(r["arrays"][0], _t(c["w"]), _t(c["bias"]), 1, relu, tfc, 288)
        if sc:
            check(r["arrays"][1], _t(c["wsc"]).reshape(32, 32, 1, 1), _t(c["bsc"]), 0, 0, 0, 32)
        else:
            assert r["arrays"][1].size == 0
    print(f"\nfcm_conv: max |err| / bound {worst:.3f}")
    assert worst > 0.0
