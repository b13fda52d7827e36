"""Op-level conformance of the Gemini DF-ResNet kernels against float64 (tools/gemini_run).

The runner launches the shipped launchers of libwsp_hip.so (launch_gemini_dw, launch_gemini_tail,
launch_gemini_down and, for the bottleneck's 1x1 convs, the shared implicit GEMM with the family's
tile family, as the model does) and holds no reference
arithmetic; one run serves all tests.  Guard rows, the columns beside the slice written and the
columns past it must come back bit-untouched.

Downsample conv and the 1x1 convs: every output element is held to the bound tests/conv_gemm_ref.py
derives for bf16x3 products with f32 accumulation (imported, not restated),
    |y - ref| <= (2^-16 + (K + 8) 2^-24) S + 4 * 2^-24 (|pre| + |act|)          S = sum |a| |w|
through the ReLU, which is 1-Lipschitz.  The float64 convolution itself is torch's conv2d with the
(frequency, time) stride pair on the operands and on their absolute values.

Depthwise conv: h = relu(b + sum_tap w y) is a chain of 9 f32 fmaf (one rounding each, every
partial sum bounded by sum |w||y|) and one f32 addition of the bias (partial bounded by
sum |w||y| + |b|); a first-order bound is 10 roundings of 2^-24 relative to sum |w||y| + |b|, one
more covers the second-order terms, and the ReLU is 1-Lipschitz:
    delta = (9 + 2) 2^-24 (sum |w||y| + |b|).

Tail: out = relu(b3 + res + W3 h) with h the depthwise conv's f32 value.  h deviates from float64
by at most delta_k, which reaches the output as sum_k |W3[n][k]| delta_k; the product of the f32 h
with W3 is held to the imported bound (S = sum |h||W3|, K = 4 d) with its epilogue term
4 * 2^-24 (|pre| + |act|) for bias, residual and ReLU:
    allowance = sum_k |W3[n][k]| delta_k + imported bound.

Measured on an MI355X (these seeds), max |err| / allowance:
gemini_dw .227, gemini_tail .115, gemini_down .064, 1x1 convs .331.
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
from conv_gemm_ref import ACT_NONE, ACT_RELU, EPS24  # noqa: E402
from op_runner import untouched as _untouched  # noqa: E402

pytestmark = pytest.mark.gpu

MAGIC = 0x47505357
DW, TAIL, DOWN, PW = 1, 2, 3, 4


# ------------------------------------------------------------------------------ cases --
def _bottleneck_inputs(rng, M, d, ldy):
    K = 4 * d
    return dict(y=ref.rand_a(rng, M, ldy, relu=True), w2=ref.rand_w(rng, 9, K, amp=0.3), b2=ref.rand_w(rng, K, amp=0.3))


def dw_case(seed, B, Fq, T, d, ldy=None, yoff=0, ldo=None, ooff=0):
    rng = np.random.default_rng(seed)
    C = 4 * d
    ldy, ldo = ldy or C, ldo or C
    c = dict(op=DW, hdr=[B, Fq, T, C, ldy, yoff, ldo, ooff], B=B, F=Fq, T=T, d=d, K=C, M=B * Fq * T, ldy=ldy, yoff=yoff,
             ldo=ldo, ooff=ooff, N=C)
    c.update(_bottleneck_inputs(rng, c["M"], d, ldy))
    c["arrays"] = [c["y"], c["w2"], c["b2"]]
    return c


def tail_case(seed, B, Fq, T, d, ldy=None, yoff=0, ldres=None, roff=0, ldo=None, ooff=0):
    rng = np.random.default_rng(seed)
    K = 4 * d
    ldy, ldres, ldo = ldy or K, ldres or d, ldo or d
    c = dict(op=TAIL, hdr=[B, Fq, T, d, ldy, yoff, ldres, roff, ldo, ooff], B=B, F=Fq, T=T, d=d, K=K, M=B * Fq * T, ldy=ldy,
             yoff=yoff, ldres=ldres, roff=roff, ldo=ldo, ooff=ooff, N=d)
    c.update(_bottleneck_inputs(rng, c["M"], d, ldy))
    c["w3"] = ref.rand_w(rng, d, K)
    c["b3"] = ref.rand_w(rng, d, amp=0.3)
    c["res"] = ref.rand_a(rng, c["M"], ldres)
    c["arrays"] = [c["y"], c["w2"], c["b2"], c["w3"], c["b3"], c["res"]]
    return c


def down_case(seed, B, Fi, Ti, cin, N, sf, st, lda=None, aoff=0, ldo=None, ooff=0):
    rng = np.random.default_rng(seed)
    lda, ldo = lda or cin, ldo or N
    Fo, To = (Fi - 1) // sf + 1, (Ti - 1) // st + 1
    c = dict(op=DOWN, hdr=[B, Fi, Ti, cin, N, sf, st, lda, aoff, ldo, ooff], B=B, Fi=Fi, Ti=Ti, Fo=Fo, To=To, cin=cin, N=N,
             sf=sf, st=st, M=B * Fo * To, lda=lda, aoff=aoff, ldo=ldo, ooff=ooff)
    c["a"] = ref.rand_a(rng, B * Fi * Ti, lda)  # a stage's output or the stem's: signed after the first level
    c["w"] = ref.rand_w(rng, N, cin, 3, 3)
    c["bias"] = ref.rand_w(rng, N, amp=0.3)
    c["arrays"] = [c["a"], c["w"], c["bias"]]
    return c


def pw_case(seed, M, cin, N, res=False, lda=None, aoff=0, ldo=None, ooff=0):
    rng = np.random.default_rng(seed)
    lda, ldo = lda or cin, ldo or N
    c = dict(op=PW, hdr=[M, cin, N, int(res), lda, aoff, ldo, ooff], M=M, cin=cin, N=N, lda=lda, aoff=aoff, ldo=ldo,
             ooff=ooff)
    c["a"] = ref.rand_a(rng, M, lda, relu=True)
    c["w"] = ref.rand_w(rng, N, cin)
    c["bias"] = ref.rand_w(rng, N, amp=0.3)
    c["res"] = ref.rand_a(rng, M, N) if res else None
    c["arrays"] = [c["a"], c["w"], c["bias"]] + ([c["res"]] if res else [])
    return c


# (B, F, T) per width: one row of two frames (every tap but the centre column's reads padding),
# utterance and plane edges, 165 positions (past one 128-position block), and every wider width
_BOTTLENECK_SHAPES = [(32, 1, 1, 2), (32, 2, 3, 7), (32, 3, 5, 11), (64, 2, 2, 5), (128, 1, 10, 3), (256, 2, 1, 3),
                      (256, 1, 5, 2)]
# the network's (cin, N, sf, st): level 2 is the only one with time stride 2
_DOWN_LEVELS = [(32, 32, 2, 1), (32, 64, 2, 2), (64, 128, 2, 1), (128, 256, 2, 1)]

CASES = []
for i, (d, B, Fq, T) in enumerate(_BOTTLENECK_SHAPES):
    CASES.append(dw_case(100 + i, B, Fq, T, d))
    CASES.append(tail_case(100 + i, B, Fq, T, d))  # the same y, w2, b2 as the depthwise case
# row strides wider than the slice, slices at non-zero offsets
CASES.append(dw_case(120, 2, 3, 7, 32, ldy=136, yoff=4, ldo=140, ooff=8))
CASES.append(tail_case(120, 2, 3, 7, 32, ldy=136, yoff=4, ldres=36, roff=4, ldo=40, ooff=4))
CASES.append(tail_case(121, 1, 4, 9, 128, ldy=520, yoff=8, ldres=128, roff=0, ldo=132, ooff=4))
for li, (cin, N, sf, st) in enumerate(_DOWN_LEVELS):
    for Fi in (1, 2, 5):
        for Ti in (2, 7):  # (32, 64) with Fi = 5, Ti = 7: stride (2, 2) with both axes odd
            CASES.append(down_case(200 + 10 * li + Fi + Ti, 2, Fi, Ti, cin, N, sf, st))
CASES.append(down_case(250, 3, 9, 11, 32, 32, 2, 1))  # 3 x 5 x 11 = 165 output positions
CASES.append(down_case(251, 2, 5, 41, 32, 64, 2, 2, lda=40, aoff=4, ldo=72, ooff=8))  # 2 x 3 x 21 = 126, strided rows
CASES.append(down_case(252, 1, 7, 9, 128, 256, 2, 1, lda=132, aoff=4, ldo=260, ooff=4))
# the bottleneck's 1x1 convs: d -> 4d + ReLU, 4d -> d + residual + ReLU
CASES.append(pw_case(300, 165, 32, 128))
CASES.append(pw_case(301, 37, 128, 512, lda=136, aoff=8, ldo=516, ooff=4))
CASES.append(pw_case(302, 165, 128, 32, res=True))
CASES.append(pw_case(303, 10, 1024, 256, res=True))


@pytest.fixture(scope="module")
def res(tmp_path_factory):
    """One runner process for all cases."""
    out = op_runner.run("gemini_run", MAGIC, [(c["op"], c["hdr"], c["arrays"]) for c in CASES],
                        tmp_path_factory.mktemp("gemini_op"))
    return [dict(r, out=r["arrays"][0] if r["status"] == 0 else None) for r in out]


def _of(res, op):
    for c, r in zip(CASES, res):
        if c["op"] == op:
            assert r["status"] == 0, f"case {c['hdr']} refused: {r['message']}"
            yield c, r


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).double()


def _slice_out(c, r, tag):
    """The slice written, after checking that nothing else was."""
    M, N, ldo, ooff = c["M"], c["N"], c["ldo"], c["ooff"]
    raw = r["out"].reshape(M + 8, ldo)
    assert _untouched(raw[M:]), f"{tag}: guard rows written"
    assert _untouched(raw[:M, :ooff]) and _untouched(raw[:M, ooff + N:]), f"{tag}: columns beside the slice written"
    got = _t(raw[:M, ooff:ooff + N])
    assert torch.isfinite(got).all(), tag
    return got


def dw_reference(c):
    """(h, delta) of the depthwise conv, float64: torch's grouped conv2d on the NHWC slice."""
    B, Fq, T, K = c["B"], c["F"], c["T"], c["K"]
    y = _t(c["y"])[:, c["yoff"]:c["yoff"] + K].reshape(B, Fq, T, K).permute(0, 3, 1, 2)
    w = _t(c["w2"]).t().reshape(K, 1, 3, 3)  # [9][K] tap-major -> (K, 1, 3, 3)
    b = _t(c["b2"])
    pre = F.conv2d(y, w, b, padding=1, groups=K)
    S = F.conv2d(y.abs(), w.abs(), None, padding=1, groups=K) + b.abs().reshape(1, K, 1, 1)
    nhwc = lambda v: v.permute(0, 2, 3, 1).reshape(c["M"], K)  # noqa: E731
    return nhwc(pre).clamp(min=0.0), (9 + 2) * EPS24 * nhwc(S)


def test_depthwise_conv(res):
    worst = 0.0
    for c, r in _of(res, DW):
        tag = f"dw {c['hdr']}"
        got = _slice_out(c, r, tag)
        want, delta = dw_reference(c)
        assert float((want > 0).double().mean()) > 0.2 and float((want == 0).double().mean()) > 0.05, tag  # ReLU both ways
        ratio = float(((got - want).abs() / delta).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{tag}: |err| / allowance = {ratio:.3f}"
    print(f"\ngemini_dw: max |err| / allowance {worst:.3f}")
    assert worst > 0.0


def tail_reference(c):
    """(want, allowance) of a tail case, float64: the depthwise allowance through |W3|, plus the
    imported bound on the product with its epilogue."""
    h, delta = dw_reference(c)
    d, K, M = c["d"], c["K"], c["M"]
    w3 = _t(c["w3"])
    resid = np.ascontiguousarray(c["res"][:, c["roff"]:c["roff"] + d])
    rc = ref.make_case(a=[h.float().numpy()], w=c["w3"].reshape(d, K, 1), M=M, T=M, B=1, bias=c["b3"], res=resid,
                       act=ACT_RELU)
    rr = ref.reference(rc, y_S=(h @ w3.t(), h.abs() @ w3.abs().t()))
    return rr["out"], delta @ w3.abs().t() + rr["bound"]


def test_bottleneck_tail(res):
    worst = 0.0
    for c, r in _of(res, TAIL):
        tag = f"tail {c['hdr']}"
        got = _slice_out(c, r, tag)
        want, allow = tail_reference(c)
        ratio = float(((got - want).abs() / allow).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{tag}: |err| / allowance = {ratio:.3f}"
    print(f"\ngemini_tail: max |err| / allowance {worst:.3f}")
    assert worst > 0.0


def test_downsample_conv(res):
    worst = 0.0
    for c, r in _of(res, DOWN):
        tag = f"down {c['hdr']}"
        got = _slice_out(c, r, tag)
        B, Fi, Ti, cin, N, M = c["B"], c["Fi"], c["Ti"], c["cin"], c["N"], c["M"]
        a = np.ascontiguousarray(c["a"][:, c["aoff"]:c["aoff"] + cin])
        x = _t(a).reshape(B, Fi, Ti, cin).permute(0, 3, 1, 2)
        w = _t(c["w"])
        conv = lambda xi, wi: F.conv2d(xi, wi, stride=(c["sf"], c["st"]), padding=1).permute(0, 2, 3, 1).reshape(M, N)  # noqa: E731
        y, S = conv(x, w), conv(x.abs(), w.abs())
        assert y.shape == (M, N) and M == B * c["Fo"] * c["To"]
        rc = ref.make_case(a=[a], w=c["w"].reshape(N, cin, 9), M=M, T=M, B=1, bias=c["bias"], act=ACT_NONE)
        rr = ref.reference(rc, y_S=(y, S))
        ratio = float(((got - rr["out"]).abs() / rr["bound"]).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{tag}: |err| / bound = {ratio:.3f}"
    print(f"\ngemini_down: max |err| / bound {worst:.3f}")
    assert worst > 0.0


def test_pointwise_convs(res):
    worst = 0.0
    for c, r in _of(res, PW):
        tag = f"pw {c['hdr']}"
        got = _slice_out(c, r, tag)
        M, cin, N = c["M"], c["cin"], c["N"]
        rc = ref.make_case(a=[c["a"]], aoff=[c["aoff"], 0, 0], w=c["w"].reshape(N, cin, 1), M=M, T=M, B=1, bias=c["bias"],
                           res=c["res"], act=ACT_RELU)
        rr = ref.reference(rc)
        ratio = float(((got - rr["out"]).abs() / rr["bound"]).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{tag}: |err| / bound = {ratio:.3f}"
    print(f"\n1x1 convs: max |err| / bound {worst:.3f}")
    assert worst > 0.0
