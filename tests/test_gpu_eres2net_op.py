"""Op-level conformance of the ERes2Net kernels against float64 (tools/eres2net_run).

The runner launches the shipped launchers of libwsp_hip.so (launch_eres_conv3x3, launch_eres_pw,
launch_eres_aff) and holds no reference arithmetic; one run serves all tests.

Conv (the 3x3 Res2 step and the 1x1 convs): every output element is held to the bound
tests/conv_gemm_ref.py derives for bf16x3 products with f32 accumulation (imported, not restated),
    |y - ref| <= (2^-16 + (K + 8) 2^-24) S + 4 * 2^-24 (|pre| + |pre|)          S = sum |a| |w|
through the clamp to [0, 20], which is 1-Lipschitz.  The added slice (sp + spx[i]) is summed in
f32 before the split, as the implicit GEMM's kAAdd operand is; its 2^-24 S sits inside the slack
between 3 * 2^-18 and 2^-16.  Guard rows, the neighbouring slices of a row and the columns past the
concatenation must come back bit-untouched.

AFF: float64 of the same path from the same f32 inputs.  The allowance propagates that bound:
    du   = bound of u = Wa [x | y] + ba                                  (K = 2C)
    dh   = 1.1 du + 4 ulp |h|              (SiLU's slope is at most 1.0999)
    dz   = |Wb| dh + bound of Wb h + bb                                  (K = C / 4, padded to 32)
    dg   = dz + 4 ulp (1 + |tanh z|)       (tanh is 1-Lipschitz)
    dout = (|x| + |y|) dg + 4 * 2^-24 (|x g| + |y (2 - g)| + |out|)
plus DEVICE_ERR (|x| + |y|) for the device's expf / tanhf: DEVICE_ERR = 4 x the largest excess of
|device - float64| / (|x| + |y|) over that allowance measured on an MI355X (ceiling 1e-6).  The
weights are scaled so that the tanh argument stays within a few units of 0 (asserted).  The
(K + 8) 2^-24 S term is a worst case that grows through both products: at C = 2048 the allowance
reaches 0.35 (|x| + |y|), so that width is held tightly only by the model fixtures (aug's
fuse_mode1234, 1e-4 on the embedding); at C = 64 / 96 it is 1.2e-3 .. 2.7e-3 (|x| + |y|).
Measured (MI355X, these seeds): max |device - float64| 1.06e-4 on outputs up to 8 (C = 2048),
7.5e-5 at C = 64 / 96; max |err| / allowance 0.020 with DEVICE_ERR = 0, so the excess over the
propagated bound is 0 -> DEVICE_ERR 0; max |z| 4.95.
max |err| / bound: eres_conv3x3 .107, eres_pw .355.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import conv_gemm_ref as ref  # noqa: E402
import op_runner  # noqa: E402
from conv_gemm_ref import EPS24  # noqa: E402
from op_runner import untouched as _untouched  # noqa: E402

pytestmark = pytest.mark.gpu

MAGIC = 0x45505357
NONE, RELU, CLAMP = 0, 1, 2
MEASURED_AFF_EXCESS = 0.0  # MI355X: no element exceeds the propagated bound (docstring)
DEVICE_ERR = 4.0 * MEASURED_AFF_EXCESS
assert DEVICE_ERR < 1e-6


# ------------------------------------------------------------------------------ cases --
def conv_case(seed, taps, B, Fi, Ti, cin, N, stride=1, lda=None, aoff=0, a2off=-1, ldo=None, ooff=0, act=CLAMP,
              res=False, hot=False):
    rng = np.random.default_rng(seed)
    lda, ldo = lda or cin, ldo or N
    Fo, To = (Fi - 1) // stride + 1, (Ti - 1) // stride + 1
    c = dict(op=1, hdr=[taps, B, Fi, Ti, cin, N, stride, lda, aoff, a2off, ldo, ooff, act, int(res)], taps=taps, B=B,
             Fi=Fi, Ti=Ti, Fo=Fo, To=To, M=B * Fo * To, cin=cin, N=N, stride=stride, lda=lda, aoff=aoff, a2off=a2off,
             ldo=ldo, ooff=ooff, act=act, hot=hot)
    c["a"] = ref.rand_a(rng, B * Fi * Ti, lda, relu=True)
    c["arrays"] = [c["a"]]
    if a2off >= 0:
        c["a2"] = ref.rand_a(rng, B * Fi * Ti, lda, relu=True)
        c["arrays"].append(c["a2"])
    k = 3 if taps == 9 else 1
    c["w"] = ref.rand_w(rng, N, cin, k, k)
    # hot: biases around the ceiling, so that pre-clamp values fall on both sides of 20
    c["bias"] = rng.uniform(15.0, 25.0, N).astype(np.float32) if hot else ref.rand_w(rng, N, amp=0.3)
    c["arrays"] += [c["w"], c["bias"]]
    if res:
        c["res"] = ref.rand_a(rng, c["M"], N)
        c["arrays"].append(c["res"])
    return c


def aff_case(seed, M, C, ldx=None, xoff=0, ldy=None, yoff=0, ldo=None, ooff=0):
    rng = np.random.default_rng(seed)
    ldx, ldy, ldo = ldx or C, ldy or C, ldo or C
    H = C // 4
    c = dict(op=2, hdr=[M, C, ldx, xoff, ldy, yoff, ldo, ooff], M=M, C=C, H=H, ldx=ldx, xoff=xoff, ldy=ldy, yoff=yoff,
             ldo=ldo, ooff=ooff)
    c["x"] = ref.rand_a(rng, M, ldx, relu=True) * np.float32(4.0)  # activations up to 4
    c["y"] = ref.rand_a(rng, M, ldy, relu=True) * np.float32(4.0)
    c["wa"] = ref.rand_w(rng, H, 2 * C, amp=0.75 / np.sqrt(2 * C))
    c["ba"] = ref.rand_w(rng, H, amp=0.3)
    c["wb"] = ref.rand_w(rng, C, H, amp=4.0 / np.sqrt(H))
    c["bb"] = ref.rand_w(rng, C, amp=0.3)
    c["arrays"] = [c[k] for k in ("x", "y", "wa", "ba", "wb", "bb")]
    return c


CASES = [
    # the Res2 step: widths 16 (one tile, K = 144 padded to 160), 24 (padded to 32 columns), 64 and
    # 192; with and without the added slice; slices inside wider rows at non-zero offsets; one
    # frequency row, two frames (every tap but the centre column's reads padding); more than one
    # block of 128 positions (3 x 5 x 11 = 165); pre-clamp values on both sides of 20
    conv_case(1, 9, 1, 1, 2, 16, 16, lda=32, aoff=16, ldo=40, ooff=16),
    conv_case(2, 9, 2, 3, 7, 16, 16, lda=32, aoff=0, a2off=16, ldo=32, ooff=16),
    conv_case(3, 9, 3, 5, 11, 24, 24, lda=72, aoff=24, a2off=48, ldo=80, ooff=48),
    conv_case(4, 9, 1, 4, 9, 24, 24, lda=24, ldo=72, ooff=0),
    conv_case(5, 9, 3, 5, 11, 64, 64, lda=128, aoff=64, ldo=128, ooff=64),
    conv_case(6, 9, 2, 1, 2, 64, 64, lda=136, aoff=8, a2off=72, ldo=132, ooff=64),
    conv_case(7, 9, 1, 2, 5, 192, 192, lda=576, aoff=192, a2off=384, ldo=576, ooff=384),
    conv_case(8, 9, 1, 3, 3, 192, 192),
    conv_case(9, 9, 2, 4, 9, 64, 64, lda=128, aoff=0, a2off=64, ldo=128, ooff=64, hot=True),
    # the 1x1 convs: stride-2 gather with odd planes, N = 72 (aug's conv1, padded to 80 columns),
    # K = 72 (padded to 96), residual + clamp, no activation (the shortcut), hot
    conv_case(11, 1, 2, 5, 9, 64, 72, stride=2),
    conv_case(12, 1, 1, 3, 7, 72, 256, res=True),
    conv_case(13, 1, 3, 7, 11, 32, 64, stride=2, act=NONE),
    conv_case(14, 1, 1, 4, 40, 128, 128, res=True, hot=True),
    # AFF: C = 64 (hidden 16, padded to 32), 96 (24 -> 32), 2048 (512); slices of wider rows and dense
    # tensors; M = 2 (the T' = 2 plane), a tile tail, more than one block
    aff_case(21, 2, 64, ldx=128, xoff=0, ldy=128, yoff=64, ldo=64),
    aff_case(22, 300, 64),
    aff_case(23, 77, 96, ldx=288, xoff=96, ldy=288, yoff=192, ldo=104, ooff=4),
    aff_case(24, 259, 96),
    aff_case(25, 50, 2048),
    aff_case(26, 19, 2048, ldx=2056, xoff=8, ldy=2048, yoff=0, ldo=2052, ooff=4),
]


@pytest.fixture(scope="module")
def res(tmp_path_factory):
    """One runner process for all cases."""
    out = op_runner.run("eres2net_run", MAGIC, [(c["op"], c["hdr"], c["arrays"]) for c in CASES],
                        tmp_path_factory.mktemp("eres2net_op"))
    return [dict(r, out=r["arrays"][0] if r["status"] == 0 else None) for r in out]


def _of(res, op, taps=None):
    for c, r in zip(CASES, res):
        if c["op"] == op and (taps is None or c["taps"] == taps):
            assert r["status"] == 0, f"case {c['hdr']} refused: {r['message']}"
            yield c, r


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).double()


def conv_reference(c):
    """(want, bound, pre) of a conv case: conv_gemm_ref's float64 conv2d and its bound."""
    a = [c["a"]] + ([c["a2"]] if c["a2off"] >= 0 else [])
    k = 3 if c["taps"] == 9 else 1
    rc = ref.make_case(a=a, aoff=[c["aoff"], max(c["a2off"], 0), 0], amode=1 if c["a2off"] >= 0 else 0, w=c["w"],
                       M=c["M"], T=c["M"], B=c["B"], conv2d=1, Fi=c["Fi"], Ti=c["Ti"], Fo=c["Fo"], To=c["To"],
                       stride=c["stride"], kw=k, pad=k // 2, bias=c["bias"], res=c.get("res"))
    rr = ref.reference(rc)
    pre = rr["pre"]
    want = {NONE: pre, RELU: pre.clamp(min=0.0), CLAMP: pre.clamp(0.0, 20.0)}[c["act"]]
    return want, rr["bound"], pre


def _check_conv(res, taps):
    worst = 0.0
    for c, r in _of(res, 1, taps):
        tag = f"conv {c['hdr']}"
        M, N, ldo, ooff = c["M"], c["N"], c["ldo"], c["ooff"]
        want, bound, pre = conv_reference(c)
        if c["hot"]:
            assert float((pre > 20.5).double().mean()) > 0.1 and float((pre < 19.5).double().mean()) > 0.1, tag
        raw = r["out"].reshape(M + 8, ldo)
        assert _untouched(raw[M:]), f"{tag}: guard rows written"
        assert _untouched(raw[:M, :ooff]) and _untouched(raw[:M, ooff + N:]), f"{tag}: columns beside the slice written"
        got = _t(raw[:M, ooff:ooff + N])
        assert torch.isfinite(got).all(), tag
        if c["act"] == CLAMP:
            assert float(got.min()) >= 0.0 and float(got.max()) <= 20.0, tag
        ratio = float(((got - want).abs() / bound).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{tag}: |err| / bound = {ratio:.3f}"
    return worst


def test_res2_step_conv3x3(res):
    worst = _check_conv(res, 9)
    print(f"\neres_conv3x3: max |err| / bound {worst:.3f}")
    assert worst > 0.0


def test_pointwise_conv(res):
    worst = _check_conv(res, 1)
    print(f"\neres_pw: max |err| / bound {worst:.3f}")
    assert worst > 0.0


def aff_reference(c):
    """(want, allowance without DEVICE_ERR, |x| + |y|, max |z|), float64."""
    M, C, H = c["M"], c["C"], c["H"]
    x = _t(c["x"])[:, c["xoff"]:c["xoff"] + C]
    y = _t(c["y"])[:, c["yoff"]:c["yoff"] + C]
    xy = np.ascontiguousarray(np.concatenate([c["x"][:, c["xoff"]:c["xoff"] + C], c["y"][:, c["yoff"]:c["yoff"] + C]], 1))
    r1 = ref.reference(ref.make_case(a=[xy], w=c["wa"].reshape(H, 2 * C, 1), M=M, T=M, B=1, bias=c["ba"]))
    u, du = r1["pre"], r1["bound"]
    h = u * torch.sigmoid(u)
    dh = 1.1 * du + 4 * 2.0 ** -23 * h.abs()
    wb, bb = _t(c["wb"]), _t(c["bb"])
    z = h @ wb.t() + bb
    S2 = h.abs() @ wb.abs().t()
    Hp = (H + 31) // 32 * 32
    dz = dh @ wb.abs().t() + (2.0 ** -16 + (Hp + 8) * EPS24) * S2 + 4 * EPS24 * 2 * z.abs()
    t = torch.tanh(z)
    g = 1.0 + t
    dg = dz + 4 * 2.0 ** -23 * (1.0 + t.abs())
    want = x * g + y * (2.0 - g)
    mag = x.abs() + y.abs()
    allow = mag * dg + 4 * EPS24 * ((x * g).abs() + (y * (2.0 - g)).abs() + want.abs())
    return want, allow, mag, float(z.abs().max())


def test_aff(res):
    worst = excess = zmax = 0.0
    for c, r in _of(res, 2):
        tag = f"aff {c['hdr']}"
        M, C, ldo, ooff = c["M"], c["C"], c["ldo"], c["ooff"]
        want, allow, mag, zm = aff_reference(c)
        zmax = max(zmax, zm)
        raw = r["out"].reshape(M + 8, ldo)
        assert _untouched(raw[M:]), f"{tag}: guard rows written"
        assert _untouched(raw[:M, :ooff]) and _untouched(raw[:M, ooff + C:]), f"{tag}: columns beside the slice written"
        got = _t(raw[:M, ooff:ooff + C])
        assert torch.isfinite(got).all(), tag
        err = (got - want).abs()
        live = mag > 0
        excess = max(excess, float(((err - allow).clamp(min=0)[live] / mag[live]).max()))
        ratio = float((err[live] / (allow + DEVICE_ERR * mag)[live]).max())
        assert float(err[~live].max() if (~live).any() else 0.0) == 0.0, tag  # x = y = 0 gives exactly 0
        worst = max(worst, ratio)
        print(f"\n{tag}: max |err| {float(err.max()):.3e}, |err| / allowance {ratio:.3f}, max |z| {zm:.2f}")
    print(f"\neres_aff: max |err| / allowance {worst:.3f}, excess over the propagated bound {excess:.3e}, max |z| {zmax:.2f}")
    assert 1.0 < zmax < 6.0  # the tanh is exercised off its centre and nowhere pinned at +-1 in f32
    assert 4.0 * excess < 1e-6, f"device deviation {excess:.3e} is a finding (ceiling 1e-6 / 4)"
    assert worst <= 1.0
