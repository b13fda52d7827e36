"""Cases of the ResNet / SimAM-ResNet op-level conformance tests (tests/test_gpu_resnet_op.py on the
MI355X, tests/test_resnet_op_ref_cpu.py against the numpy emulations), with their header ints and arrays
as the op table of tools/resnet_run.cpp lists them.  Every case draws from
np.random.default_rng([op, idx]); `refuse` names the WSP_CHECK that must refuse the case (asserted there
and nowhere else).  Every case has B of 2 or more with different data per utterance (but the two SimAM
cases the chunking asks for), so a halo or a statistic that leaks across utterances shows, and every input
is a continuous random draw: non-zero at every border.

conv3x3 / tail.  The shapes are the smallest at which the tiling can go wrong: conv3x3_img's tiles are
4 x 64 positions (F x T) for C = 32 and 4 x 32 for C = 64 / 128 (C = 128 in variants 0 and 3);
bottleneck_tail_kernel has the same tiles and tail2_kernel (the tail with the next conv1 fused) FB x 32
with FB = 8 / 4 / 2 for C = 32 / 64 / 128.  CONV_SHAPES and TAIL_SHAPES hold a partial and a full tile in
each direction, F < FB and T = 1.  x in [-1, 1], |W| <= 1.5 / sqrt(K): outputs of order 1, biases of a
tenth of that, so a ReLU cuts about half of the values (asserted on the CPU).

SimAM.  C in {4, 64, 128, 512, 1024} (256, 16, 8, 2, 1 rows per pass of the moment kernel) against rows in
{2, 63, 64, 65, 129} at B = 3; B = 40 x 200 rows (3 chunks); B = 1 x 4481 rows (70 chunks of 65 rows: the
last one is empty).  z regimes:
  normal    N(0, 1)
  offset    30 + 0.01 N(0, 1): the variance is 1e-5 of the second moment or less (the cancellation)
  constant  N(0, 1) with every fourth channel constant per utterance (variance 0: the 1e-4 term alone)
  relu      N(0, 1) with res = -100 on half of the elements
In every regime one element per (utterance, channel) of every fourth channel (offset by one from the
constant ones) sits 14 sd above the mean, which carries the sigmoid's argument past 8 once rows >= 63 (in the offset regime the
1e-4 is as large as the variance and halves the argument).
res = N(0, 1) - 0.65 z elsewhere (0.65 is the gate at its median argument), so that the ReLU cuts about half of the values in every regime.
"""
import functools

import numpy as np

MAGIC = 0x4E505357
OPS = dict(conv3x3=1, tail=2, stem=3, simam=4, tfc=5)
F32 = np.float32
GUARD = 4  # guard rows on either side of every output (tools/resnet_run.cpp)

CONV_SHAPES = ((1, 1, 3), (3, 31, 2), (4, 32, 3), (5, 33, 2), (9, 65, 2), (4, 70, 2), (1, 64, 2))  # F, T, B
CONV_CONFIGS = ((32, 0), (64, 0), (128, 0), (128, 3))  # C, variant
CONV_OPTIONS = ("relu", "res", "norelu", "scale")
TAIL_SHAPES = ((1, 1), (3, 33), (9, 70), (11, 45))  # F, T
STEM_SHAPES = ((1, 8), (2, 16), (37, 24), (257, 8))  # T, F
SIMAM_C = (4, 64, 128, 512, 1024)
SIMAM_ROWS = (2, 63, 64, 65, 129)
SIMAM_REGIMES = ("normal", "offset", "constant", "relu")
TFC_SHAPES = ((2, 3, 5, 4), (3, 10, 33, 64))  # B, F, T, C


def _case(op_name, idx, name, group, **kw):
    return dict(op=OPS[op_name], op_name=op_name, idx=idx, name=f"{op_name}-{name}", group=group, refuse=None, **kw)


def _empty():
    return np.zeros(0, F32)


def _weight(rng, n, k, *taps):
    a = 1.5 / np.sqrt(k * int(np.prod(taps, dtype=np.int64)))
    return rng.uniform(-a, a, (n, k) + taps).astype(F32)


def _bias(rng, n):
    return rng.uniform(-0.05, 0.05, n).astype(F32)


# ------------------------------------------------------------------------------ conv3x3 --
def conv_case(idx, C, variant, F, T, B, option, name, group, gv=7, twin=1):
    rng = np.random.default_rng([1, idx])
    x = rng.uniform(-1.0, 1.0, (B, F, T, C)).astype(F32)
    W = _weight(rng, C, C, 3, 3)
    bias = _bias(rng, C)
    res = rng.uniform(-0.5, 0.5, (B, F, T, C)).astype(F32) if "res" in option else None
    scale = shift = None
    if "scale" in option:
        scale = rng.uniform(-1.5, 1.5, C).astype(F32)
        scale[0], scale[1] = 0.0, -1.25
        shift = rng.uniform(0.01, 0.05, C).astype(F32) * rng.choice(np.array([-1.0, 1.0], F32), C)
    relu = int("norelu" not in option)
    return _case("conv3x3", idx, name, group, C=C, variant=variant, F=F, T=T, B=B, relu=relu, x=x, W=W, bias=bias, res=res,
                 scale=scale, shift=shift, twin=twin, gv=gv,
                 hdr=[C, B, F, T, variant, relu, int(res is not None), int(scale is not None), twin, gv],
                 arrays=[x, W, bias, _empty() if res is None else res, _empty() if scale is None else scale,
                         _empty() if shift is None else shift])


def conv_cases():
    out = []
    for C, variant in CONV_CONFIGS:
        for F, T, B in CONV_SHAPES:
            for option in CONV_OPTIONS:
                gv = (4, 5, 7)[len(out) % 3]  # the implicit GEMM's tile family of the twin launch
                out.append(conv_case(len(out), C, variant, F, T, B, option, f"c{C}-v{variant}-f{F}-t{T}-b{B}-{option}",
                                     f"conv3x3 c{C} v{variant}", gv=gv))
    c = conv_case(len(out), 96, 0, 3, 33, 2, "relu", "refuse-c96", "conv3x3 refusals", twin=0)
    c["refuse"] = "conv3x3_img: channels"
    out.append(c)
    c = conv_case(len(out), 64, 0, 3, 33, 2, "res-norelu", "refuse-res-norelu", "conv3x3 refusals", twin=0)
    c["refuse"] = "conv3x3_img: a residual comes with the ReLU"
    out.append(c)
    return out


# --------------------------------------------------------------------------------- tail --
def tail_case(idx, C, F, T, form, name, group, B=2, alias=0, with_res=None, c1n=None):
    """form: alone | c1 (next conv1 C -> C) | c2 (next conv1 -> 2C) | xsc (in-tail shortcut, next conv1 C -> C)"""
    rng = np.random.default_rng([2, idx])
    fuse1, xsc = int(form != "alone"), int(form == "xsc")
    if c1n is None:
        c1n = 0 if form == "alone" else 2 * C if form == "c2" else C
    with_res = int(not xsc) if with_res is None else with_res
    C4 = 4 * C
    y1 = rng.uniform(0.0, 1.0, (B, F, T, C)).astype(F32) * rng.choice(np.array([0.0, 1.0], F32), (B, F, T, C), p=[0.3, 0.7])
    y1 += F32(0.01)  # a conv1 + ReLU output, a third of it at its floor; never exactly zero
    res = rng.uniform(-0.5, 0.5, (B, F, T, C4)).astype(F32) if with_res else None
    W2, b2 = _weight(rng, C, C, 3, 3), _bias(rng, C)
    W3, b3 = _weight(rng, C4, C), _bias(rng, C4)
    xs = None
    if xsc:
        xs = rng.uniform(-1.0, 1.0, (B, F, T, C)).astype(F32)
        W3 = np.concatenate([W3, _weight(rng, C4, C)], axis=1)  # [conv3 | shortcut], b3 the summed bias
    W1 = _weight(rng, c1n, C4) if fuse1 else None
    b1 = _bias(rng, c1n) if fuse1 else None
    both = int(fuse1 and not xsc and with_res and not alias)  # the same operands through bottleneck_tail_kernel too
    return _case("tail", idx, name, group, C=C, F=F, T=T, B=B, form=form, fuse1=fuse1, c1n=c1n, xsc=xsc, alias=alias,
                 with_res=with_res, both=both, y1=y1, res=res, W2=W2, b2=b2, W3=W3, b3=b3, W1=W1, b1=b1, xs=xs,
                 hdr=[C, B, F, T, fuse1, c1n, xsc, alias, with_res, both],
                 arrays=[y1, _empty() if res is None else res, W2, b2, W3, b3, _empty() if W1 is None else W1,
                         _empty() if b1 is None else b1, _empty() if xs is None else xs])


def tail_cases():
    out = []
    for C in (32, 64, 128):
        forms = ("alone", "c1") + (("c2",) if C <= 64 else ()) + (("xsc",) if C == 32 else ())
        for form in forms:
            for F, T in TAIL_SHAPES:
                out.append(tail_case(len(out), C, F, T, form, f"c{C}-{form}-f{F}-t{T}", f"tail c{C} {form}"))
    for name, kw in (("refuse-out-is-res", dict(C=32, form="alone", alias=1)),
                     ("refuse-c128-c1n-2c", dict(C=128, form="c1", c1n=256)),
                     ("refuse-xsc-c64", dict(C=64, form="xsc")),
                     ("refuse-xsc-and-res", dict(C=32, form="xsc", with_res=1))):
        kw = dict(kw)
        c = tail_case(len(out), kw.pop("C"), 3, 33, kw.pop("form"), name, "tail refusals", **kw)
        c["refuse"] = "bottleneck_tail"
        out.append(c)
    return out


# --------------------------------------------------------------------------------- stem --
def stem_case(idx, C0, T, F, name, group, B=3):
    rng = np.random.default_rng([3, idx])
    feats = rng.standard_normal((B, T, F)).astype(F32)
    w = rng.uniform(-0.5, 0.5, (C0, 9)).astype(F32)
    bias = rng.uniform(-0.2, 0.2, C0).astype(F32)
    return _case("stem", idx, name, group, B=B, T=T, F=F, C0=C0, feats=feats, w=w, bias=bias, hdr=[B, T, F, C0],
                 arrays=[feats, w, bias])


def stem_cases():
    out = []
    for C0 in (32, 64):
        for T, F in STEM_SHAPES:
            out.append(stem_case(len(out), C0, T, F, f"c{C0}-t{T}-f{F}", f"stem c{C0}"))
    c = stem_case(len(out), 16, 2, 16, "refuse-c16", "stem refusals")
    c["refuse"] = "resnet stem"
    out.append(c)
    return out


# -------------------------------------------------------------------------------- simam --
def constant_channels(C):
    return np.arange(C) % 4 == 1


def outlier_channels(C):
    return np.arange(C) % 4 == 2


def simam_case(idx, B, rows, C, regime, name, group):
    rng = np.random.default_rng([4, idx])
    mean, sd = (30.0, 0.01) if regime == "offset" else (0.0, 1.0)
    z = mean + sd * rng.standard_normal((B, rows, C))
    if regime == "constant":
        z[:, :, constant_channels(C)] = rng.uniform(0.5, 2.0, (B, 1, int(constant_channels(C).sum())))
    if rows > 1:
        at = rng.integers(0, rows, (B, C))
        oc = np.nonzero(outlier_channels(C))[0]
        for b in range(B):
            z[b, at[b, oc], oc] = mean + 14.0 * sd
    z = z.astype(F32)
    res = (rng.standard_normal((B, rows, C)) - 0.65 * z).astype(F32)
    if regime == "relu":
        res[rng.uniform(0.0, 1.0, res.shape) < 0.5] = F32(-100.0)
    return _case("simam", idx, name, group, B=B, rows=rows, C=C, regime=regime, z=z, res=res, hdr=[B, rows, C], arrays=[z, res])


def simam_cases():
    out = []
    for iC, C in enumerate(SIMAM_C):
        for iR, rows in enumerate(SIMAM_ROWS):
            regime = SIMAM_REGIMES[(iC + iR) % 4]
            out.append(simam_case(len(out), 3, rows, C, regime, f"b3-r{rows}-c{C}-{regime}", f"simam {regime}"))
    for regime in SIMAM_REGIMES:  # every regime on more than one chunk and on a partial last pass
        out.append(simam_case(len(out), 3, 129, 64, regime, f"b3-r129-c64-{regime}-all", f"simam {regime}"))
    out.append(simam_case(len(out), 40, 200, 64, "offset", "b40-r200-c64-offset-3chunks", "simam offset"))
    out.append(simam_case(len(out), 1, 4481, 64, "normal", "b1-r4481-c64-normal-empty-chunk", "simam normal"))
    for name, rows, C, msg in (("refuse-rows1", 1, 64, "simam: need >= 2"), ("refuse-c12", 65, 12, "simam: C must be")):
        c = simam_case(len(out), 3, rows, C, "normal", name, "simam refusals")
        c["refuse"] = msg
        out.append(c)
    return out


# ------------------------------------------------------------------------------------ tfc --
def tfc_cases():
    out = []
    for B, F, T, C in TFC_SHAPES:
        x = np.random.default_rng([5, len(out)]).standard_normal((B, F, T, C)).astype(F32)
        out.append(_case("tfc", len(out), f"b{B}-f{F}-t{T}-c{C}", "nhwc_to_tfc", B=B, F=F, T=T, C=C, x=x, hdr=[B, F, T, C],
                         arrays=[x]))
    return out


@functools.lru_cache(maxsize=None)
def _all():
    return tuple(conv_cases() + tail_cases() + stem_cases() + simam_cases() + tfc_cases())


def all_cases():
    """Every case, built once per process and shared: the tests leave the arrays unchanged."""
    return list(_all())


def op_case(c):
    return c["op"], c["hdr"], c["arrays"]


NARRAYS = {1: 6, 2: 9, 3: 3, 4: 2, 5: 1}


def narrays(op, hdr):
    return NARRAYS[op]
