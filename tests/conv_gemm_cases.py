"""The operand sets of the conv-GEMM op tests (tests/test_gpu_conv_gemm_op.py runs them on the
GPU; tests/test_conv_gemm_ref_cpu.py runs an emulation over groups 1, 2, 3 and 14).

Every group returns base cases (no variant chosen yet) built from fixed seeds: activations in
[-1, 1], every second case post-ReLU, weights in +-0.05.  The shapes are the smallest that still
cross every block edge (128 / 256 rows x 32 / 64 / 128 / 256 columns), k-tile edge (32, Kp a
multiple of 64) and utterance edge.
"""
import numpy as np

from conv_gemm_ref import ACT_GELU, ACT_NONE, ACT_RELU, ACT_TANH, make_case, rand_a, rand_w, to_bf16, with_

X3_VARIANTS = (3, 4, 5, 6, 7)


class _Gen:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.n = 0

    def a(self, rows, ld):
        self.n += 1
        return rand_a(self.rng, rows, ld, relu=self.n % 2 == 0)

    def w(self, *shape):
        return rand_w(self.rng, *shape)

    def vec(self, n, lo=-0.5, hi=0.5):
        return self.rng.uniform(lo, hi, size=n).astype(np.float32)

    def bn(self, n):
        return self.vec(n, 0.5, 1.5) * np.where(self.rng.uniform(size=n) < 0.25, -1, 1).astype(np.float32), self.vec(n)


def group1():
    """Dense 1x1: M = 333 (a partial 256-row block, nine utterances per block), Kp = 128 > K."""
    g, out = _Gen(101), []
    B, T, cin = 9, 37, 96
    for N in (32, 64, 96, 128, 256, 384):
        sc, sh = g.bn(N)
        out.append(make_case(name=f"g1 N={N}", a=[g.a(B * T, cin + 4)], w=g.w(N, cin, 1), M=B * T, T=T, ldo=N + 8,
                             bias=g.vec(N), act=ACT_RELU, scale=sc, shift=sh))
    return out


def group2():
    """Dilated k3 convs; with T = 5 every tap leaves the utterance somewhere."""
    g, out = _Gen(102), []
    for B, T in ((9, 37), (40, 5)):
        for dil in (2, 3, 4):
            for N in (128, 256):
                out.append(make_case(name=f"g2 B={B} T={T} dil={dil} N={N}", a=[g.a(B * T, 64)], w=g.w(N, 64, 3),
                                     M=B * T, T=T, dil=dil, pad=dil, bias=g.vec(N)))
    return out


def group3():
    """K-tiles that straddle taps (cin % 32 != 0): family 7's AM 2, the others' per-lane path."""
    g, out = _Gen(103), []
    B, T = 3, 101
    for cin, taps, pad, N in ((80, 5, 2, 64), (80, 5, 2, 256), (20, 3, 1, 128)):
        out.append(make_case(name=f"g3 cin={cin} taps={taps} N={N}", a=[g.a(B * T, cin)], w=g.w(N, cin, taps),
                             M=B * T, T=T, pad=pad, bias=g.vec(N)))
    return out


def group4():
    """torch.cat(dim=1) without a copy: three buffers, the last a view into a wider one."""
    g, out = _Gen(104), []
    B, T = 9, 37
    M = B * T
    for N in (128, 256):
        for cseg, lda, aoff in (([0, 64, 128, 192], (64, 72, 256), [0, 0, 128]),
                                ([0, 32, 96, 192], (32, 68, 96), [0, 4, 0]),
                                ([0, 64, 192, 192], (64, 132, 0), [0, 4, 0])):
            a = [g.a(M, ld) if ld else None for ld in lda]
            out.append(make_case(name=f"g4 cseg={cseg} N={N}", a=a, aoff=aoff, cseg=cseg, w=g.w(N, 192, 1), M=M, T=T,
                                 bias=g.vec(N), act=ACT_RELU))
    return out


def group5():
    """kAAdd: a[0] + a[1] under a dilated k3 conv (Res2Net's sp + spx[i])."""
    g, out = _Gen(105), []
    B, T = 9, 37
    for N in (64, 128, 256):
        out.append(make_case(name=f"g5 N={N}", a=[g.a(B * T, 64), g.a(B * T, 68)], amode=1, w=g.w(N, 64, 3), M=B * T,
                             T=T, dil=2, pad=2, bias=g.vec(N), act=ACT_RELU))
    return out


def group6():
    """Strided 1-D convs (the HuBERT feature extractor), uniform and ragged with iseg, GELU."""
    g, out = _Gen(106), []
    B, T, cin, N = 3, 40, 64, 256
    for taps, extra in ((3, 1), (2, 0)):
        Ti = 2 * T + extra
        out.append(make_case(name=f"g6 k{taps} s2 uniform", a=[g.a(B * Ti, cin)], w=g.w(N, cin, taps), M=B * T, T=T,
                             Ti=Ti, stride=2, bias=g.vec(N), act=ACT_GELU))
        lo = [40, 17, 33]
        li = [2 * n + extra for n in lo]
        seg, iseg = np.cumsum([0] + lo).astype(np.int32), np.cumsum([0] + li).astype(np.int32)
        out.append(make_case(name=f"g6 k{taps} s2 ragged", a=[g.a(int(iseg[-1]), cin)], w=g.w(N, cin, taps),
                             M=int(seg[-1]), T=max(lo), Ti=max(li), stride=2, seg=seg, iseg=iseg, bias=g.vec(N),
                             act=ACT_GELU))
    return out


def group7():
    """Ragged batches (an utterance of one frame, one that ends a row past a block edge), and the
    uniform 1x1 whose input rows differ from its output rows (family 7 must take AM 0)."""
    g, out = _Gen(107), []
    lens = [300, 1, 257, 6, 123]
    seg = np.cumsum([0] + lens).astype(np.int32)
    M = int(seg[-1])
    for N in (64, 256):
        out.append(make_case(name=f"g7 1x1 row_bias N={N}", a=[g.a(M, 64)], w=g.w(N, 64, 1), M=M, T=max(lens),
                             seg=seg, bias=g.vec(N), row_bias=g.vec(len(lens) * N).reshape(len(lens), N),
                             act=ACT_RELU))
        sc, sh = g.bn(N)
        out.append(make_case(name=f"g7 k3 dil2 BN N={N}", a=[g.a(M, 64)], w=g.w(N, 64, 3), M=M, T=max(lens), seg=seg,
                             dil=2, pad=2, bias=g.vec(N), act=ACT_RELU, scale=sc, shift=sh))
        B, T = 3, 37
        out.append(make_case(name=f"g7 1x1 Ti=T+10 N={N}", a=[g.a(B * (T + 10), 64)], w=g.w(N, 64, 1), M=B * T, T=T,
                             Ti=T + 10, bias=g.vec(N)))
    return out


def group8():
    """Grouped columns (HuBERT pos_conv as an implicit GEMM): 4 groups of 48 channels, k8."""
    g, out = _Gen(108), []
    lens = [70, 3, 131]
    seg = np.cumsum([0] + lens).astype(np.int32)
    M = int(seg[-1])
    for gcols in (64, 32):
        N = 4 * gcols
        out.append(make_case(name=f"g8 gcols={gcols}", a=[g.a(M, 4 * 48 + 4)], w=g.w(N, 48, 8), M=M, T=max(lens),
                             seg=seg, pad=4, gcols=gcols, gcin=48, bias=g.vec(N), act=ACT_GELU))
    return out


def group9():
    """2-D NHWC convs (ResNet): 3x3 s1, 3x3 s2, 1x1 s2; bias + ReLU and residual + ReLU."""
    g, out = _Gen(109), []
    B, Fi, Ti, cin = 2, 5, 13, 32
    for kh, stride, pad in ((3, 1, 1), (3, 2, 1), (1, 2, 0)):
        Fo, To = (Fi + 2 * pad - kh) // stride + 1, (Ti + 2 * pad - kh) // stride + 1
        M = B * Fo * To
        for N in (32, 64, 128, 256):
            for res in (False, True):
                out.append(make_case(name=f"g9 {kh}x{kh} s{stride} N={N} res={int(res)}", a=[g.a(B * Fi * Ti, cin)],
                                     w=g.w(N, cin, kh, kh), M=M, T=M, B=B, conv2d=1, Fi=Fi, Ti=Ti, Fo=Fo, To=To,
                                     stride=stride, kw=kh, pad=pad, bias=g.vec(N), act=ACT_RELU,
                                     res=g.a(M, N + 4) if res else None))
    return out


def group10():
    """ResNet conv3 + projection shortcut in one GEMM (sc2d): a dense segment and a strided one."""
    g, out = _Gen(110), []
    B, Fi, Ti, N = 3, 6, 14, 256
    for stride in (2, 1):
        Fo, To = (Fi - 1) // stride + 1, (Ti - 1) // stride + 1
        M = B * Fo * To
        out.append(make_case(name=f"g10 stride={stride}", a=[g.a(M, 64), g.a(B * Fi * Ti, 64)], cseg=[0, 64, 128, 128],
                             w=g.w(N, 128, 1), M=M, T=M, B=B, sc2d=1, Fi=Fi, Ti=Ti, Fo=Fo, To=To, stride=stride,
                             bias=g.vec(N), act=ACT_RELU))
    return out


def group11():
    """SE column sums: blocks straddle utterances, so both slots of a block's partials are used."""
    g, out = _Gen(111), []
    B = 3
    for T in (256, 257, 300):
        for taps, dil in ((1, 1), (3, 2)):
            for N in (64, 128, 256):
                sc, sh = g.bn(N)
                out.append(make_case(name=f"g11 T={T} taps={taps} N={N}", a=[g.a(B * T, 64)], w=g.w(N, 64, taps),
                                     M=B * T, T=T, dil=dil, pad=dil * (taps // 2), bias=g.vec(N), act=ACT_RELU,
                                     scale=sc, shift=sh, colsum=True))
    return out


def ln_partials(x):
    """(mean, M2) of each 128-column piece of the rows of x -> float32 [M][parts][2], the form in
    which a producer GEMM (lnmode 1) hands a row's LayerNorm statistics on."""
    M, width = x.shape
    p = np.asarray(x, dtype=np.float64).reshape(M, width // 128, 128)
    mean = p.mean(axis=2)
    return np.stack([mean, ((p - mean[:, :, None]) ** 2).sum(axis=2)], axis=2).astype(np.float32)


def ln_images_colsum(w):
    """ln_cs[n] = sum_c of the bf16 hi + lo images of W'[n][c], an f64 sum rounded once
    (hubert_model.cpp: HLayer::fc1_cs)."""
    hi = to_bf16(w)
    lo = to_bf16(w - hi)
    return (hi.astype(np.float64) + lo.astype(np.float64)).sum(axis=1).astype(np.float32)


def group12():
    """HuBERT LayerNorm fold (tile family 7, dense 1x1): rows whose mean is about 3 x their
    standard deviation, so that acc - mu * ln_cs cancels.  Each case carries the unfolded layer
    (`ln_w`, `ln_b0`, `ln_gamma`, `ln_beta`) it was prepared from where it has one."""
    g, out = _Gen(112), []
    M, eps = 300, 1e-5

    def rows(width, ld):  # mean in [1, 2] per row, spread 0.85 * U(-1, 1): sigma ~ 0.5
        x = g.rng.uniform(1.0, 2.0, size=(M, 1)) + 0.85 * g.rng.uniform(-1.0, 1.0, size=(M, ld))
        return x.astype(np.float32)

    for width in (256, 768):
        parts = width // 128
        # mode 1: y = A W^T + b + res, statistics of y emitted
        out.append(make_case(name=f"g12 mode 1 width={width}", a=[g.a(M, 256)], w=g.w(width, 256, 1), M=M, T=M,
                             bias=g.vec(width), res=rows(width, width + 4), lnmode=1))
        # mode 2: LayerNorm(A) W^T + b as (A W'^T - mu ln_cs) rstd + b'
        a = rows(width, width)
        w, b0 = g.w(width, width, 1), g.vec(width)
        gamma, beta = g.vec(width, 0.5, 1.5), g.vec(width)
        w64 = w.reshape(width, width).astype(np.float64)
        wf = (w64 * gamma.astype(np.float64)[None, :]).astype(np.float32)
        bf = (b0.astype(np.float64) + w64 @ beta.astype(np.float64)).astype(np.float32)
        for act in (ACT_NONE, ACT_GELU):  # the two activations the fold implements
            out.append(make_case(name=f"g12 mode 2 width={width} act={act}", a=[a], w=wf.reshape(width, width, 1), M=M,
                                 T=M, bias=bf, act=act, lnmode=2, ln_in=ln_partials(a), ln_parts=parts,
                                 ln_cs=ln_images_colsum(wf), ln_eps=eps, ln_w=w64, ln_b0=b0, ln_gamma=gamma,
                                 ln_beta=beta))
        # modes 4 / 5: y = A W^T + b + LayerNorm(res) (5: statistics of y emitted as well)
        for mode in (4, 5):
            res = rows(width, width + 4)
            out.append(make_case(name=f"g12 mode {mode} width={width}", a=[g.a(M, 256)], w=g.w(width, 256, 1), M=M,
                                 T=M, bias=g.vec(width), res=res, lnmode=mode, ln_in=ln_partials(res[:, :width]),
                                 ln_parts=parts, ln_g=g.vec(width, 0.5, 1.5), ln_b=g.vec(width), ln_eps=eps))
        # statistics probes: W = 0, no bias, ln_g = 1, ln_b = 0 leave out = (res - mu) rstd, so the
        # mean and rstd the kernel merges from ln_in (g_ln_row, shared by modes 2 / 4 / 5) stand
        # alone: with S = 0 the bound is their 8 f32 ulps plus the f32 epilogue
        for mode in (4, 5):
            res = rows(width, width + 4)
            out.append(make_case(name=f"g12 statistics probe mode {mode} width={width}", a=[g.a(M, 256)],
                                 w=np.zeros((width, 256, 1), dtype=np.float32), M=M, T=M, res=res, lnmode=mode,
                                 ln_in=ln_partials(res[:, :width]), ln_parts=parts,
                                 ln_g=np.ones(width, dtype=np.float32), ln_b=np.zeros(width, dtype=np.float32),
                                 ln_eps=eps, stats_probe=True))
    return out


def _epilogue_shape(g):
    B, T, K, N = 2, 65, 64, 256
    return B, T, K, N, g.a(B * T, K), g.w(N, K, 1)


def group13():
    """Epilogue matrix on one small shape (M = 130, K = 64, N = 256)."""
    g, out = _Gen(113), []
    B, T, K, N, a, w = _epilogue_shape(g)
    bias, rb, res = g.vec(N, -5.0, 5.0), g.vec(B * N, -1.0, 1.0).reshape(B, N), g.a(B * T, N + 8)
    sc, sh = g.bn(N)
    for hb in (True, False):
        for hbn in (True, False):
            for extra in ("none", "row_bias", "res"):
                for act in (ACT_NONE, ACT_RELU, ACT_TANH, ACT_GELU):
                    out.append(make_case(name=f"g13 bias={int(hb)} bn={int(hbn)} {extra} act={act}", a=[a], w=w,
                                         M=B * T, T=T, bias=bias if hb else None,
                                         row_bias=rb if extra == "row_bias" else None,
                                         res=res if extra == "res" else None, act=act, scale=sc if hbn else None,
                                         shift=sh if hbn else None, twin_key=(hb, extra)))
    return out


def group14():
    """Split-term probes: one operand exactly representable in bf16 (its lo image is zero), so
    the two surviving product terms must carry the other operand's lo part: 2^-17 S."""
    g = _Gen(114)
    B, T, K, N, a, w = _epilogue_shape(g)
    bias = g.vec(N)
    return [make_case(name="g14 A exact", a=[to_bf16(a)], w=w, M=B * T, T=T, bias=bias, prod_exp=17),
            make_case(name="g14 W exact", a=[a], w=to_bf16(w), M=B * T, T=T, bias=bias, prod_exp=17)]


def group15():
    """The prefetched-residual epilogue (role = 2 with a residual on the tiles of at most four
    accumulator tiles per wave: the residual is loaded ahead of the last two k-tiles).  M = 130
    leaves the last 128-row block partial; with K = 64 the k-loop ahead of the prefetch runs zero
    times, with K = 192 twice.  The wide tiles, family 7 and the f32 kernel ignore `role`."""
    g, out = _Gen(115), []
    B, T = 2, 65
    for K in (64, 192):
        for N in (32, 64, 128, 256):
            out.append(make_case(name=f"g15 K={K} N={N}", a=[g.a(B * T, K)], w=g.w(N, K, 1), M=B * T, T=T, role=2,
                                 bias=g.vec(N), res=g.a(B * T, N + 8), act=ACT_RELU))
    return out


def f32_takes(c):
    """Operands launch_conv_gemm documents: 1-D convs with N % 64 == 0, no column sums."""
    return (not c["conv2d"] and not c["sc2d"] and not c["lnmode"] and c["N"] % 64 == 0 and not c["colsum"]
            and (not c["gcols"] or c["gcols"] % 64 == 0))


def expand(cases, variants=X3_VARIANTS, f32=True):
    """Every base case under each bf16x3 tile family and, where it takes them, the f32 kernel."""
    out = []
    for i, c in enumerate(cases):  # `base` = the case's index in its group (keys the shared references)
        out += [with_(c, variant=v, precision=1, base=i) for v in variants]
        if f32 and f32_takes(c):
            out.append(with_(c, variant=0, precision=0, base=i))
    return out


def uniform_ktiles(c):
    return c["cin"] % 32 == 0 and (c["amode"] == 1 or (c["cseg"][1] % 32 == 0 and c["cseg"][2] % 32 == 0))


def expected_tile(c):
    """The kernel each case is written for (kernels.h / conv_gemm_x3.hip: family 7 takes 1-D
    single- or concat-operand convs with N % 256 == 0; 2-D, added-operand and grouped GEMMs and
    other widths fall to family 6's tiles)."""
    N, g = c["N"], c["gcols"]
    if not c["precision"]:
        return "f32_128x128" if N % 128 == 0 and not g else "f32_128x64"
    v = c["variant"]
    if v == 7:
        if (N % 256 == 0 and not c["conv2d"] and not g and c["amode"] == 0
                and (uniform_ktiles(c) or (c["cseg"][1] >= c["cin"] and not c["colsum"]))):
            return "g256"
        v = 6
    if N % 64 or (g and g % 64):
        return "128x32"
    if g:
        return "256x64" if v >= 5 else "128x64"
    if N % 128:
        return "128x64"
    if v == 3:
        return "128x128"
    if v == 4 or N % 256:
        return "256x128"
    return "256x256mf16" if v == 6 else "256x256"
