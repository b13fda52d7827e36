"""Cases of ECAPA's op-level conformance tests (tests/test_gpu_ecapa_op.py on the MI355X,
tests/test_ecapa_op_ref_cpu.py against the numpy emulations), with their header ints and arrays as the
op table of tools/ecapa_run.cpp lists them.  Every case draws from np.random.default_rng([op, idx]);
`refuse` marks the cases a WSP_CHECK of the library must refuse (asserted there and nowhere else).
Every leading dimension exceeds its width by a multiple of 4 unless the case exists to break
alignment, and the pad columns hold random values.

Scaling.  The allowances are proportional to S = sum |a||w|, so the inputs are scaled until the largest
allowance of a case is below 1e-5 (tests/test_ecapa_op_ref_cpu.py asserts it): res2 x in [-0.1, 0.1]
with |W| <= 1 / (3w); the gate / seam weights in +-0.0015; small_linear's weights shrink with K; the
ASTP x regimes (a) and (b) are N(0, 1) and max(0, N(0.5, 1)) times XS = 2^-6 -- a power of two, so every
product, sum and rounding of the kernel is the unscaled one shifted by 6 (or 12) binades and only the
variance floor sits elsewhere.  An utterance whose softmax rests on fewer than 8 frames in some channel
(the single maxima, a rising staircase whose top chunk holds one frame, T of 1 or 2) has its variance at
the floor, where sqrt's slope is 1 / (2 sqrt(floor)): its x is scaled by XS_PEAKED = 2^-10 instead
(utterance_scales), so that the std's allowance stays below 1e-5 there too.  The cancellation regimes -- ASTP x (c) (mean 30, sd 0.1) and (d)
(constant per channel) and frame_stats' offset columns (mean 100, sd 0.01) -- are exempt by name.

Chain.  Per width, variant and dilation: a ragged batch whose lengths put utterance boundaries at many
window phases (res2_lens), 5 x 77 and 2 x 263; one long-strip case (BIG); and, per width and variant, two
one-sided cases (res2_case, `side`) on which a halo one row short on either side exceeds the allowance,
which it does not on the random weights.

ASTP logits.  att = uniform (-0.98, 0.98) with column 0 structured, W2[:, 1:] ~ N(0, sn), W2[:, 0] = G:
e[t][c] = G_c u_t + noise + bias_c, so S = sum |att||W2| stays near |e| + 4 even where the logits span
84 units.  Regimes:
  sd1    no structure, noise sd about 1
  sd8    u_t = -min(|N(0, 1)| / 4, 0.99), G about 32: a peaky softmax, noise sd about 0.5
  rise   u_t = -0.12 (chunks - 1 - chunk(t)) - 0.01 U, G about 100: chunk maxima rise by about 12 per
         32-frame chunk, the running max is raised in every chunk
  fall   the same falling by 12 per chunk
  last   e = -30 everywhere but the last live frame of the utterance (0)
  first  e = -30 everywhere but frame 0
The unfused op takes float32(e) of the same construction as its input.
"""
import functools
import inspect
import struct

import numpy as np

MAGIC = 0x41505357
OPS = dict(res2=1, astp_fused=2, astp_pool=3, frame_stats=4, small_linear=5, residual_scale=6, gate=7, seam=8)
XS = 2.0 ** -6
XS_PEAKED = 2.0 ** -10
F32 = np.float32


def f32_bits(v):
    return struct.unpack("<i", struct.pack("<f", float(v)))[0]


def _seg(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def _no_seg():
    return np.zeros(0, np.int32)


def _case(op_name, idx, name, group, **kw):
    return dict(op=OPS[op_name], op_name=op_name, idx=idx, name=f"{op_name}-{name}", group=group, refuse=None, **kw)


def lazy(op_name=None):
    """The decorated builder returns a spec -- dict(op_name, name, group, refuse, make) -- without drawing
    anything; materialize(spec) builds the case.  Listing the cases (pytest's collection) then costs nothing."""
    def deco(fn):
        sig = inspect.signature(fn)

        @functools.wraps(fn)
        def wrapper(*a, **k):
            args = sig.bind(*a, **k).arguments
            op = op_name or args["op_name"]
            return dict(op_name=op, name=f"{op}-{args['name']}", group=args["group"], refuse=None,
                        make=functools.partial(fn, *a, **k))
        return wrapper
    return deco


def materialize(spec):
    c = spec["make"]()
    assert (c["name"], c["group"], c["op_name"]) == (spec["name"], spec["group"], spec["op_name"])
    c["refuse"] = spec["refuse"]
    return c


# --------------------------------------------------------------------------- res2_chain --
def res2_lens(d):
    r = 128 - 12 * d
    return [1, 2, d, 2 * d + 1, r - 1, r, r + 1, 131, 2 * r + 5, 9]


@lazy("res2")
def res2_case(idx, w, variant, dil, lens, uniform, name, group, ldx=None, ldo=None, rout_delta=0, side=None):
    rng = np.random.default_rng([1, idx])
    M = int(sum(lens))
    ldx = 8 * w + 8 if ldx is None else ldx
    ldo = 7 * w + 4 if ldo is None else ldo
    K = 3 * w
    x = rng.uniform(-0.1, 0.1, (M, ldx)).astype(F32)
    W = rng.uniform(-1.0 / K, 1.0 / K, (7, w, w, 3)).astype(F32)
    ystd = np.sqrt(K) * (1.0 / K) * 0.1 / 3.0
    bias = (rng.uniform(-1.0, 1.0, (7, w)) * ystd).astype(F32)  # ReLU cuts about half of the values
    scale = rng.uniform(-1.5, 1.5, (7, w)).astype(F32)
    scale[:, 0], scale[:, 1] = 0.0, -1.25
    shift = rng.uniform(0.01, 0.05, (7, w)).astype(F32) * rng.choice(np.array([-1.0, 1.0], F32), (7, w))
    if side is not None:
        # One-sided operands: positive, the weight on one outer tap (0: offset -d, 2: offset +d), unit
        # scale.  The chain then carries a row's value 7d rows to one side at a gain of 2 / 3 per step; with
        # the random weights above (gain below 1 per step, random sign) a row's contribution 7d rows away
        # is far below the allowance and a halo one row short would pass.
        x, W, bias = np.abs(x) * F32(0.5), np.abs(W) * F32(0.05), np.abs(bias)
        W[..., side] *= F32(80.0)
        scale, shift = np.ones_like(scale), np.abs(shift) * F32(0.01)
    seg = _seg(lens)
    return _case("res2", idx, name, group, w=w, variant=variant, dil=dil, B=len(lens),
                 T=int(max(lens)), M=M, ldx=ldx, ldo=ldo, lens=list(lens), seg=None if uniform else seg, x=x, W=W,
                 bias=bias, scale=scale, shift=shift,
                 hdr=[w, variant, dil, len(lens), int(max(lens)), M, ldx, ldo, int(not uniform), rout_delta],
                 arrays=[x, W, bias, scale, shift, _no_seg() if uniform else seg])


# the strip case: M just above 128 x 256 CUs (B = 67, T = 498, M = 33 366)
BIG = dict(w=128, variant=4, dil=3, B=67, T=498)


def res2_cases(big=True):
    out = []
    combos = []
    for w in (64, 128):
        for variant in (0, 2, 3) + ((4,) if w == 128 else ()):
            for dil in (2, 3, 4):
                combos.append((w, variant, dil))
        combos.append((w, 3, 1))
    for w, variant, dil in combos:
        tag = f"w{w}-v{variant}-d{dil}"
        out.append(res2_case(len(out), w, variant, dil, res2_lens(dil), False, tag + "-ragged", f"res2 w{w} v{variant}"))
        out.append(res2_case(len(out), w, variant, dil, [77] * 5, True, tag + "-5x77", f"res2 w{w} v{variant}"))
        out.append(res2_case(len(out), w, variant, dil, [263] * 2, True, tag + "-2x263", f"res2 w{w} v{variant}"))
    for w in (64, 128):
        for variant in (0, 2, 3) + ((4,) if w == 128 else ()):
            for side in (0, 2):
                out.append(res2_case(len(out), w, variant, 4, res2_lens(4), False, f"w{w}-v{variant}-d4-ragged-tap{side}",
                                     f"res2 one-sided w{w}", side=side))
    if big:
        out.append(res2_case(len(out), BIG["w"], BIG["variant"], BIG["dil"], [BIG["T"]] * BIG["B"], True, "strips-67x498",
                             "res2 long strips", ldx=8 * BIG["w"]))
    # the last one is not a shape the model launches (it asks for variant 3 at w = 64): the launcher let it
    # through to the window kernel with a strip's rout, which a 128-row window cannot own
    for name, kw in (("refuse-w96", dict(w=96)), ("refuse-dil5", dict(dil=5)), ("refuse-rout", dict(rout_delta=1)),
                     ("refuse-ldo", dict(ldo=7 * 128 - 4)), ("refuse-w64-v4", dict(w=64, variant=4))):
        a = dict(w=128, variant=3, dil=2, rout_delta=0, ldo=None)
        a.update(kw)
        c = res2_case(len(out), a["w"], a["variant"], a["dil"], [77] * 2, True, name, "res2 refusals", ldo=a["ldo"],
                      rout_delta=a["rout_delta"])
        c["refuse"] = "res2_chain"
        out.append(c)
    return out


# ---------------------------------------------------------------------------------- astp --
LOGITS = ("sd1", "sd8", "rise", "fall", "last", "first")
XREG = ("a", "b", "c", "d")
EXEMPT_X = ("c", "d")


def astp_operands(rng, lens, C, logits):
    """att [rows][128], W2 [C][128], bias [C] (float32) of a logit regime."""
    rows = int(sum(lens))
    att = rng.uniform(-0.98, 0.98, (rows, 128)).astype(F32)
    sn = 0.157 if logits == "sd1" else 0.078
    w2 = (sn * rng.standard_normal((C, 128))).astype(F32)
    bias = rng.standard_normal(C).astype(F32)
    if logits == "sd1":
        return att, w2, bias
    u = np.zeros(rows)
    r0 = 0
    for L in lens:
        t = np.arange(L)
        nch = (L + 31) // 32
        if logits == "sd8":
            uu = -np.minimum(np.abs(rng.standard_normal(L)) / 4.0, 0.99)
        elif logits in ("rise", "fall"):
            step = (nch - 1 - t // 32) if logits == "rise" else t // 32
            uu = -0.12 * step - 0.01 * rng.uniform(0.0, 1.0, L)
        else:
            uu = np.full(L, -0.3)
            uu[L - 1 if logits == "last" else 0] = 0.0
        u[r0:r0 + L] = uu
        r0 += L
    att[:, 0] = u
    G = 32.0 if logits == "sd8" else 100.0
    w2[:, 0] = G * (1.0 + 0.02 * rng.uniform(-1.0, 1.0, C))
    return att, w2, bias


def utterance_scales(e, lens):
    """XS per utterance, XS_PEAKED where its softmax rests on fewer than 8 frames in some channel
    (1 / sum alpha^2 from the float64 logits e [rows][C]): both powers of two."""
    out, r0 = [], 0
    for L in lens:
        p = np.exp(e[r0:r0 + L] - e[r0:r0 + L].max(axis=0))
        al = p / p.sum(axis=0)
        out.append(XS if (1.0 / (al * al).sum(axis=0)).min() >= 8.0 else XS_PEAKED)
        r0 += L
    return np.repeat(out, lens)[:, None]


def astp_x(rng, rows, ld, C, xreg, scales):
    if xreg == "a":
        return (scales * rng.standard_normal((rows, ld))).astype(F32)
    if xreg == "b":
        return (scales * np.maximum(0.0, 0.5 + rng.standard_normal((rows, ld)))).astype(F32)
    if xreg == "c":
        return (30.0 + 0.1 * rng.standard_normal((rows, ld))).astype(F32)
    return np.broadcast_to(rng.uniform(0.5, 2.0, ld).astype(F32), (rows, ld)).copy()


@lazy("astp_fused")
def astp_fused_case(idx, C, lens, uniform, logits, xreg, floor, name, group, ldx=None):
    rng = np.random.default_rng([2, idx])
    rows = int(sum(lens))
    ldx = C + 8 if ldx is None else ldx
    att, w2, bias = astp_operands(rng, lens, C, logits)
    e = att.astype(np.float64) @ w2.astype(np.float64).T + bias
    x = astp_x(rng, rows, ldx, C, xreg, utterance_scales(e, lens))
    seg = _seg(lens)
    B, T = len(lens), int(max(lens))
    return _case("astp_fused", idx, name, group, B=B, T=T, C=C, ldx=ldx, lens=list(lens), seg=None if uniform else seg,
                 logits=logits, xreg=xreg, var_floor=floor, att=att, w2=w2, bias2=bias, x=x,
                 hdr=[B, T, C, ldx, int(not uniform), rows, f32_bits(floor)],
                 arrays=[att, x, w2, bias, _no_seg() if uniform else seg])


ASTP_T = (1, 2, 31, 32, 33, 64, 65, 96, 97, 129, 193, 225)


def astp_fused_cases():
    out = []
    for iC, C in enumerate((256, 512, 1536)):
        for iT, T in enumerate(ASTP_T):
            for ragged in (0, 1):
                logits = LOGITS[(iT + 2 * iC + 3 * ragged) % 6]
                xreg = XREG[(iT + iC + ragged) % 4]
                floor = (1e-7, 1e-5)[(iT + iC) % 2]
                lens = [T, 1, 33] if ragged else [T] * 3
                name = f"c{C}-t{T}-{'ragged' if ragged else 'uniform'}-{logits}-x{xreg}"
                out.append(astp_fused_case(len(out), C, lens, not ragged, logits, xreg, floor, name,
                                           "astp_fused x " + xreg))
    for T in (97, 225):  # every staircase on a partial last chunk, 4 and 8 chunks
        for logits in ("rise", "fall", "last", "first"):
            for xreg in ("a", "c"):
                out.append(astp_fused_case(len(out), 256, [T] * 3, True, logits, xreg, 1e-7, f"stair-t{T}-{logits}-x{xreg}",
                                           "astp_fused staircase x " + xreg))
    # rising and falling staircases whose top chunk is full (32 comparable frames): the std after a rescale in
    # every chunk, away from the floor
    for T in (64, 96, 128, 224):
        for logits in ("rise", "fall"):
            out.append(astp_fused_case(len(out), 256, [T] * 3, True, logits, "a", 1e-7, f"stair-t{T}-{logits}-xa",
                                       "astp_fused full-top staircase x a"))
    c = astp_fused_case(len(out), 320, [33] * 3, True, "sd1", "a", 1e-7, "refuse-c320", "astp_fused refusals")
    c["refuse"] = "astp_fused"
    out.append(c)
    return out


POOL_T = (1, 2, 3, 4, 5, 8, 9, 12, 13, 257)


@lazy("astp_pool")
def astp_pool_case(idx, C, eoff, lens, uniform, logits, xreg, floor, name, group):
    rng = np.random.default_rng([3, idx])
    rows = int(sum(lens))
    att, w2, bias = astp_operands(rng, lens, C, logits)
    e = (att.astype(np.float64) @ w2.astype(np.float64).T + bias).astype(F32)
    x = astp_x(rng, rows, C, C, xreg, utterance_scales(e.astype(np.float64), lens))
    seg = _seg(lens)
    B, T = len(lens), int(max(lens))
    ebuf = np.concatenate([rng.standard_normal(eoff).astype(F32), e.reshape(-1)])
    return _case("astp_pool", idx, name, group, B=B, T=T, C=C, lens=list(lens), seg=None if uniform else seg, logits=logits,
                 xreg=xreg, var_floor=floor, e=e, x=x, eoff=eoff,
                 hdr=[B, T, C, int(not uniform), rows, eoff, f32_bits(floor)], arrays=[ebuf, x, _no_seg() if uniform else seg])


def astp_pool_cases():
    out = []
    for iF, (C, eoff, form) in enumerate(((260, 0, "vector"), (1536, 0, "vector"), (6, 0, "scalar"), (256, 1, "scalar"))):
        for iT, T in enumerate(POOL_T):
            for ragged in (0, 1):
                logits = LOGITS[(iT + 2 * iF + 3 * ragged) % 6]
                xreg = XREG[(iT + iF + ragged) % 4]
                floor = (1e-7, 1e-5)[(iT + iF) % 2]
                lens = [T, 1, 33] if ragged else [T] * 3
                name = f"c{C}{'-eoff1' if eoff else ''}-t{T}-{'ragged' if ragged else 'uniform'}-{logits}-x{xreg}"
                out.append(astp_pool_case(len(out), C, eoff, lens, not ragged, logits, xreg, floor, name,
                                          f"astp_pool {form} x {xreg}"))
    return out


# --------------------------------------------------------------------------- frame_stats --
STATS_T = (2, 3, 4, 5, 15, 16, 17, 19, 20, 21, 498)


def offset_columns(C):
    return np.arange(C) % 8 == 5


@lazy("frame_stats")
def frame_stats_case(idx, C, ldx, lens, uniform, with_std, std_off, name, group):
    rng = np.random.default_rng([4, idx])
    rows = int(sum(lens))
    ldo = 2 * C + 8
    x = rng.standard_normal((rows, ldx)).astype(F32)
    off = offset_columns(C)
    x[:, :C][:, off] = (100.0 + 0.01 * rng.standard_normal((rows, int(off.sum())))).astype(F32)
    seg = _seg(lens)
    B, T = len(lens), int(max(lens))
    return _case("frame_stats", idx, name, group, B=B, T=T, C=C, ldx=ldx, ldo=ldo, with_std=with_std, std_off=std_off,
                 lens=list(lens), seg=None if uniform else seg, x=x,
                 hdr=[B, T, C, ldx, ldo, with_std, std_off, int(not uniform), rows], arrays=[x, _no_seg() if uniform else seg])


def frame_stats_cases():
    out = []
    forms = ((260, 268, "vector"), (1536, 1544, "vector"), (6, 14, "scalar"), (260, 266, "scalar"))  # C, ldx
    for C, ldx, form in forms:
        for iT, T in enumerate(STATS_T):
            for ragged in (0, 1):
                with_std, so = ((1, C), (1, C + 2), (0, C), (1, C + 2))[(iT + 2 * ragged) % 4]
                lens = [T, 2, 17] if ragged else [T] * 3
                name = f"c{C}-ldx{ldx}-t{T}-{'ragged' if ragged else 'uniform'}-std{with_std}-off{so - C}"
                out.append(frame_stats_case(len(out), C, ldx, lens, not ragged, with_std, so, name, "frame_stats " + form))
        for ragged in (0, 1):
            lens = [1, 5, 1] if ragged else [1] * 3
            name = f"c{C}-ldx{ldx}-t1-{'ragged' if ragged else 'uniform'}-std0"
            out.append(frame_stats_case(len(out), C, ldx, lens, not ragged, 0, C, name, "frame_stats " + form))
    return out


# -------------------------------------------------------------------------- small_linear --
@lazy("small_linear")
def small_linear_case(idx, R, K, N, act, has_bias, scratch, name, group, seed_idx=None):
    rng = np.random.default_rng([5, idx if seed_idx is None else seed_idx])
    ldin, ldo = K + 4, N + 8
    amp = min(1.0, 3e-6 * 4.0 / ((K + 32) * K * 2.0 ** -24))
    a = rng.uniform(-1.0, 1.0, (R, ldin)).astype(F32)
    wt = rng.uniform(-amp, amp, (K, N)).astype(F32)
    bias = rng.uniform(-2.0, 2.0, N).astype(F32) if has_bias else None
    c = _case("small_linear", idx, name, group, R=R, K=K, N=N, ldin=ldin, ldo=ldo, act=act, scratch=scratch, bias=bias,
              wt=wt, hdr=[R, K, N, ldin, ldo, act, int(has_bias), scratch],
              arrays=[a, wt, bias if has_bias else np.zeros(0, F32)])
    c["in"] = a
    return c


SL_R, SL_K, SL_N = (1, 3, 4, 5, 17), (1, 3, 15, 16, 17, 128, 3072, 4096, 4097, 20480), (1, 63, 64, 65, 192)


def small_linear_cases():
    out = []
    for sweep in range(3):  # three sweeps over K with the other parameters rotating against it
        for iK, K in enumerate(SL_K):
            R = SL_R[(iK + 2 * sweep) % 5]
            N = SL_N[(2 * iK + sweep) % 5] if K < 20480 or sweep == 0 else 65
            act = (iK + sweep) % 4
            has_bias = (iK + sweep) % 2 == 0 or act >= 2  # tanh / sigmoid cover their range through the bias
            out.append(small_linear_case(len(out), R, K, N, act, has_bias, 0,
                                         f"r{R}-k{K}-n{N}-act{act}-{'bias' if has_bias else 'nobias'}", "small_linear one pass"))
    # K >= 4096 both ways on the same operands: one pass (no scratch) and split-K (exactly the scratch asked for)
    for K, R, N, act in ((4096, 17, 192, 1), (4096, 1, 65, 3), (4097, 5, 64, 2), (4097, 17, 63, 0), (20480, 3, 65, 2),
                         (20480, 17, 64, 0)):
        for scratch in (0, 1):
            seed = len(out) - scratch
            out.append(small_linear_case(len(out), R, K, N, act, True, scratch,
                                         f"r{R}-k{K}-n{N}-act{act}-{'splitk' if scratch else 'onepass'}",
                                         "small_linear split-K" if scratch else "small_linear one pass", seed_idx=seed))
    c = small_linear_case(len(out), 5, 4096, 64, 0, True, 2, "refuse-scratch-short", "small_linear refusals")
    c["refuse"] = "small_linear"
    out.append(c)
    assert len(out) <= 60
    return out


# ------------------------------------------------------------------------ residual_scale --
RS_UNIFORM = {1: (1, 1), 7: (7, 1), 63: (21, 3), 64: (64, 1), 65: (1, 65), 130: (2, 65)}  # rows -> (B, T)
RS_RAGGED = {1: [1], 7: [1, 5, 1], 63: [3, 59, 1], 64: [1, 62, 1], 65: [64, 1], 130: [65, 1, 64]}


@lazy("residual_scale")
def residual_scale_case(idx, C, lens, uniform, has_x, name, group):
    rng = np.random.default_rng([6, idx])
    M, B = int(sum(lens)), len(lens)
    x = rng.uniform(-1.0, 1.0, (M, C)).astype(F32) if has_x else None
    h = rng.uniform(-1.0, 1.0, (M, C)).astype(F32)
    g = rng.uniform(0.0, 1.0, (B, C)).astype(F32)
    seg = _seg(lens)
    return _case("residual_scale", idx, name, group, B=B, T=int(max(lens)), C=C, M=M, lens=list(lens),
                 seg=None if uniform else seg, x=x, h=h, g=g, hdr=[B, int(max(lens)), C, int(has_x), int(not uniform), M],
                 arrays=[x if has_x else np.zeros(0, F32), h, g, _no_seg() if uniform else seg])


def residual_scale_cases():
    out = []
    for C in (64, 512, 1024, 2048):
        for has_x in (1, 0):
            for rows in (1, 7, 63, 64, 65, 130):
                B, T = RS_UNIFORM[rows]
                tag = f"c{C}-{'x' if has_x else 'nox'}-rows{rows}"
                out.append(residual_scale_case(len(out), C, [T] * B, True, has_x, tag + "-uniform", "residual_scale"))
                out.append(residual_scale_case(len(out), C, RS_RAGGED[rows], False, has_x, tag + "-ragged", "residual_scale"))
    for C in (6, 384):
        c = residual_scale_case(len(out), C, [3] * 7, True, 1, f"refuse-c{C}", "residual_scale refusals")
        c["refuse"] = "residual_scale"
        out.append(c)
    return out


# --------------------------------------------------------------------------- gate / seam --
@lazy()
def gemm_case(op_name, idx, lens, uniform, N, K, gate_k0, name, group, variant=7):
    rng = np.random.default_rng([OPS[op_name], idx])
    M, B, T = int(sum(lens)), len(lens), int(max(lens))
    seam = op_name == "seam"
    lda, ldg, ldo, ldh, ldso = K + 8, K - gate_k0 + 4, N + 4, K + 4, K + 12
    a = rng.uniform(-1.0, 1.0, (M, lda)).astype(F32)
    w = rng.uniform(-0.0015, 0.0015, (N, K)).astype(F32)
    bias = rng.uniform(-0.05, 0.05, N).astype(F32)
    scale = rng.uniform(-1.5, 1.5, N).astype(F32)
    scale[0], scale[1] = 0.0, -1.25
    shift = rng.uniform(0.01, 0.05, N).astype(F32) * rng.choice(np.array([-1.0, 1.0], F32), N)
    gate = rng.uniform(0.0, 1.0, (B, ldg)).astype(F32)
    gate[:, 0], gate[:, 1] = 0.0, 1.0
    seg = _seg(lens)
    hdr = [variant, B, T, N, K, gate_k0, lda, ldg, ldo, int(not uniform), M]
    arrays = [a, w, bias, scale, shift, gate, _no_seg() if uniform else seg]
    c = _case(op_name, idx, name, group, B=B, T=T, M=M, N=N, K=K, gate_k0=gate_k0, variant=variant, lda=lda, ldg=ldg,
              ldo=ldo, ldh=ldh, ldso=ldso, lens=list(lens), seg=None if uniform else seg, a=a, w=w, bias=bias, scale=scale,
              shift=shift, gate=gate, h=None)
    if seam:
        c["h"] = rng.uniform(-1.0, 1.0, (M, ldh)).astype(F32)
        hdr += [ldh, ldso]
        arrays.append(c["h"])
    c["hdr"], c["arrays"] = hdr, arrays
    return c


def gate_cases():
    out = []
    for B in (2, 3):
        for T in (256, 257):
            for N in (256, 512):
                for K, k0 in ((384, 0), (384, 128), (384, 256), (256, 128)):
                    out.append(gemm_case("gate", len(out), [T] * B, True, N, K, k0, f"b{B}-t{T}-n{N}-k{K}-k0{k0}", "gated tail"))
    for name, kw in (("refuse-variant6", dict(variant=6)), ("refuse-t255", dict(lens=[255] * 3)),
                     ("refuse-ragged", dict(lens=[256, 257, 258], uniform=False))):
        a = dict(variant=7, lens=[257] * 3, uniform=True)
        a.update(kw)
        c = gemm_case("gate", len(out), a["lens"], a["uniform"], 256, 384, 128, name, "gated tail refusals", variant=a["variant"])
        c["refuse"] = "conv_gemm"
        out.append(c)
    return out


def seam_cases():
    out = []
    for B in (2, 3):
        for T in (256, 257):
            for N, K in ((256, 256), (512, 192), (768, 320)):
                out.append(gemm_case("seam", len(out), [T] * B, True, N, K, 0, f"b{B}-t{T}-n{N}-k{K}", "seam"))
    for name, kw in (("refuse-variant6", dict(variant=6)), ("refuse-t255", dict(lens=[255] * 3)),
                     ("refuse-ragged", dict(lens=[256, 257, 258], uniform=False))):
        a = dict(variant=7, lens=[257] * 3, uniform=True)
        a.update(kw)
        c = gemm_case("seam", len(out), a["lens"], a["uniform"], 256, 256, 0, name, "seam refusals", variant=a["variant"])
        c["refuse"] = "conv_gemm"
        out.append(c)
    return out


def all_cases(big=True):
    return (res2_cases(big) + astp_fused_cases() + astp_pool_cases() + frame_stats_cases() + small_linear_cases()
            + residual_scale_cases() + gate_cases() + seam_cases())


def op_case(c):
    return c["op"], c["hdr"], c["arrays"]


def exempt(c):
    """The named cancellation regimes, exempt from the 1e-5 ceiling on the allowance (frame_stats: its
    offset columns only, see offset_columns)."""
    return c["op_name"] in ("astp_fused", "astp_pool") and c["xreg"] in EXEMPT_X
