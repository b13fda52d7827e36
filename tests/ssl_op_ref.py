"""Float64 references and element-wise allowances for the kernels only the HuBERT / WavLM front end
uses: attn.hip (attention plain / biased, the gate), pos_conv.hip, and hubert.hip's layernorm_kernel
and conv0.  Every reference is computed in float64 from the same f32 inputs and never reproduces a
kernel's index arithmetic.  EPS24 = 2^-24 (half an f32 ulp of 1), U4 = 4 f32 ulps = 4 * 2^-23.

Attention (both kernels; dh = 64, scale 1/8).  s_ij = q_i . k_j / 8 (+ g_i table[clamp(j - i)]),
a = softmax_j(s), o = a v.  With S_ij = sum_d |q_id| |k_jd| / 8:
    ds_ij  = (2^-16 + (64 + 8 + 2) 2^-24) S_ij + 2 * 2^-24 |g_i table|
             the bf16x3 product (3 * 2^-18 < 2^-16, as conv_gemm_ref), the f32 accumulation over
             K = 64, the pre-scaling of q (by 1/8: exact; by log2(e)/8 in the pipelined kernel: one
             rounding of the factor and one of the product), and the bias fma (the table is
             pre-scaled by log2(e) there: one more rounding, hence 2).
    rel_ij = ds_ij + 2^-24 |s_ij - m_i| C_ARG + e_exp           (m_i = max_j s_ij)
             the relative error of the weight p_ij = exp(s_ij - m): the absolute error of the
             exponent's argument, i.e. ds, the rounding of the subtraction, and the arguments of
             the rescales a weight goes through later, which telescope to at most |s_ij - m_i|
             again: C_ARG = 2.  (The pipelined kernel's lazy maximum trails m_i by up to 8 log2
             units, 5.5 natural: 3.3e-7 more, inside the slack of 2^-16 S against 3 * 2^-18 S for
             S > 0.03.)  e_exp = E_EXP is the device's v_exp_f32 / __expf part: not chosen in
             advance but measured, see tests/test_gpu_ssl_op.py.
    |do_id| <= (2 max_j rel_ij + 2^-16 + (T + 8) 2^-24) sum_j a_ij |v_jd| + 4 * 2^-24 |o_id|
             numerator and denominator each carry max rel; the second bf16x3 product (P V) and its
             f32 accumulation over T keys (and of l); the final 1 / l and product.

Gate: ga (gb grep_a[h] - 1) + 2 with ga = sigmoid(x_h . wa + ba), gb = sigmoid(x_h . wb + bb).
    da   = (64 + 8) 2^-24 (sum |x| |wa| + |ba|)           the f32 dot product (16 lanes x 4, 4 shuffles)
    dga  = da / 4 + U4 ga + E_GATE / 4                    sigmoid's slope is at most 1/4; expf's relative
                                                          error e moves sigmoid by at most e / 4
    dt   = |grep| dgb + U4 (|gb grep| + |t|)              t = gb grep - 1
    dout = |t| dga + ga dt + U4 (|ga t| + |out|)

pos_conv: conv_gemm_ref's bound with K = 6144 on the float64 pre-activation (one grouped float64
conv per utterance, 16 groups x 48 channels x 128 taps, pad 64, the last frame of SamePad dropped),
    dpre = (2^-16 + (6144 + 8) 2^-24) S + 4 * 2^-24 (|y| + |pre|)
then the GELU rule of DESIGN.md section 4.  The kernel has no act-none twin, so the documented GELU
allowance is applied to the float64 pre-activation with dpre carried through GELU, whose slope is at
most 1.13:
    dout = 1.13 dpre + 0.5 |pre| 1.5e-7 + U4 |gelu| + GELU_DEVICE_ERR
GELU_DEVICE_ERR = 1.114e-7 is the device part of the same gelu_as function measured by
tests/test_gpu_conv_gemm_op.py (4 x 2.785e-8).

LayerNorm (one wave per row, lane owns 4 V4 channels, V4 = D / 256; two passes).  x' = x + add:
    dx   = 2^-24 |x'| with add, else 0
    dmu  = dx-mean + (4 + (V4 - 1) + 6 + 2) 2^-24 mean |x'|
             4 adds in a lane, V4 - 1 across its registers, 6 shuffle steps, the product with 1 / D
             and that factor's own rounding (1 / 768)
    dc   = dx + dmu + 2^-24 |c|                            c = x' - mu
    dvar = (4 V4 + 6 + 2) 2^-24 var + mean(2 |c| dc + dc^2)    the fma chain, 6 shuffle steps, 1 / D
    dr   = rstd (dvar / (2 (var + eps)) + 4 * 2^-24)       the sum with eps, sqrtf, the division
    dout = |gamma| (rstd dc + |c| dr) + 2 * 2^-24 |c rstd gamma| + 2^-24 |out|
The featurizer line is feat = w y or fma(w, y, feat): dfeat = |w| dout + 2^-24 |feat|.

conv0 (k10, s5 -> GroupNorm over time per channel, biased variance, eps 1e-5 -> exact GELU).  The
statistics are f64 sums of at most T0 terms (from 65 waveform moments), so the allowance is the f32
part plus the f64 cancellation of var = E[y^2] - mean^2:
    dy     = 10 * 2^-24 sum |w| |x|                        10 fmas
    dvar   = 2 (T0 + 128) 2^-53 mean((sum |w| |x|)^2)
    dscale = |scale| (dvar / (2 (var + eps)) + 3 * 2^-24)  rstd to f32, the product with gamma
    dshift = |mean| dscale + 3 * 2^-24 |mean scale| + 2^-24 |shift|     beta - (float) mean * scale
    dz     = |scale| dy + |y| dscale + dshift + 2^-24 |z|  z = fma(y, scale, shift)
    dout   = 1.13 dz + 0.5 |z| 1.5e-7 + U4 |gelu| + GELU_DEVICE_ERR
"""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from conv_gemm_ref import EPS24, FILL, rand_a, rand_w  # noqa: E402,F401

U4 = 4 * 2.0 ** -23
C_ARG = 2.0
GELU_DEVICE_ERR = 4.0 * 2.785e-8
REL_MAX, REL_N, REL_STRIDE = 778, 1557, 1560  # attn.h kAttnRelMax / kAttnRelN / kAttnRelStride
DH = 64


def t64(x):
    return torch.from_numpy(np.ascontiguousarray(x)).double()


def gelu64(y):
    return 0.5 * y * (1.0 + torch.erf(y / math.sqrt(2.0)))


# ------------------------------------------------------------------------- attention --
def attn_scores(q, k, table=None, gate=None):
    """float64 scores s [T][T] of one (utterance, head) and the bias part g_i table[j - i]."""
    T = q.shape[0]
    s = q @ k.t() / 8.0
    bias = torch.zeros_like(s)
    if table is not None:
        i = torch.arange(T)
        d = (i[None, :] - i[:, None]).clamp(-REL_MAX, REL_MAX) + REL_MAX  # key - query
        bias = gate[:, None] * table[d]
    return s + bias, bias


def attn_head(q, k, v, table=None, gate=None):
    """(want [T][64], allowance without e_exp, A = sum_j a_ij |v_jd|): the allowance with the
    device part is allow + 2 e_exp A."""
    T = q.shape[0]
    s, bias = attn_scores(q, k, table, gate)
    S = q.abs() @ k.abs().t() / 8.0
    ds = (2.0 ** -16 + (64 + 8 + 2) * EPS24) * S + 2 * EPS24 * bias.abs()
    m = s.max(dim=1, keepdim=True).values
    rel = ds + EPS24 * (s - m).abs() * C_ARG
    a = torch.softmax(s, dim=1)
    o = a @ v
    A = a @ v.abs()
    allow = (2 * rel.max(dim=1, keepdim=True).values + 2.0 ** -16 + (T + 8) * EPS24) * A + 4 * EPS24 * o.abs()
    return o, allow, A


def attn_reference(c):
    """(want, allow, A) [rows][H * 64] of an attention case (ssl_op_cases' attn_random, attn_selector
    and attn_staircase)."""
    H, seg = c["H"], c["seg"]
    qkv = t64(c["qkv"])
    D = H * DH
    outs = [torch.zeros(c["rows"], D, dtype=torch.float64) for _ in range(3)]
    for b in range(len(seg) - 1):
        r0, r1 = int(seg[b]), int(seg[b + 1])
        for h in range(H):
            q, k, v = (qkv[r0:r1, j * D + h * DH:j * D + (h + 1) * DH] for j in range(3))
            tab = gate = None
            if c["table"] is not None:
                tab, gate = t64(c["table"])[h, :REL_N], t64(c["gate"])[r0:r1, h]
            for dst, src in zip(outs, attn_head(q, k, v, tab, gate)):
                dst[r0:r1, h * DH:(h + 1) * DH] = src
    return outs


# ------------------------------------------------------------------------------ gate --
def gate_reference(c, e_gate=0.0):
    """(want, allowance, pre-sigmoid arguments) [rows][H]."""
    H = c["H"]
    x = t64(c["x"])[:, :H * DH].reshape(-1, H, DH)
    w = t64(c["w"])
    wa, wb, ba, bb, grep = w[:DH], w[DH:2 * DH], w[2 * DH], w[2 * DH + 1], w[2 * DH + 2:]
    a, b = x @ wa + ba, x @ wb + bb
    da = 72 * EPS24 * (x.abs() @ wa.abs() + ba.abs())
    db = 72 * EPS24 * (x.abs() @ wb.abs() + bb.abs())
    ga, gb = torch.sigmoid(a), torch.sigmoid(b)
    dga, dgb = da / 4 + U4 * ga + e_gate / 4, db / 4 + U4 * gb + e_gate / 4
    t = gb * grep - 1.0
    dt = grep.abs() * dgb + U4 * ((gb * grep).abs() + t.abs())
    out = ga * t + 2.0
    allow = t.abs() * dga + ga * dt + U4 * ((ga * t).abs() + out.abs())
    return out, allow, torch.stack([a, b])


# -------------------------------------------------------------------------- pos_conv --
PC_G, PC_CIN, PC_TAPS, PC_PAD = 16, 48, 128, 64


def pos_conv_pre(x, seg, w, bias, gout):
    """(pre, S) [M][16][48] float64: bias + the grouped conv per utterance (taps that leave the
    utterance read zero), and S = sum |x| |w|.  w [16 gout][48][128] torch layout, rows g gout + n."""
    M = int(seg[-1])
    x = t64(x)[:, :PC_G * PC_CIN].reshape(M, PC_G, PC_CIN)
    w = t64(w).reshape(PC_G, gout, PC_CIN, PC_TAPS)[:, :PC_CIN]  # the 48 real rows of every group
    bias = t64(bias).reshape(PC_G, gout)[:, :PC_CIN]
    wk = w.permute(0, 3, 2, 1).reshape(PC_G, PC_TAPS * PC_CIN, PC_CIN)  # [g][tap * 48 + c][n]
    pre = torch.zeros(M, PC_G, PC_CIN, dtype=torch.float64)
    S = torch.zeros_like(pre)
    for b in range(len(seg) - 1):
        r0, r1 = int(seg[b]), int(seg[b + 1])
        T = r1 - r0
        xp = torch.zeros(T + PC_TAPS, PC_G, PC_CIN, dtype=torch.float64)
        xp[PC_PAD:PC_PAD + T] = x[r0:r1]
        win = xp.unfold(0, PC_TAPS, 1)[:T]  # [T][g][c][tap]: frames t - 64 .. t + 63
        a = win.permute(1, 0, 3, 2).reshape(PC_G, T, PC_TAPS * PC_CIN)
        pre[r0:r1] = torch.bmm(a, wk).permute(1, 0, 2)
        S[r0:r1] = torch.bmm(a.abs(), wk.abs()).permute(1, 0, 2)
    return pre + bias, S, bias


def pos_conv_reference(c):
    """(want, allowance) [M][16][48]."""
    pre, S, bias = pos_conv_pre(c["x"], c["seg"], c["w"], c["bias"], c["gout"])
    dpre = (2.0 ** -16 + (PC_CIN * PC_TAPS + 8) * EPS24) * S + 4 * EPS24 * ((pre - bias).abs() + pre.abs())
    out = gelu64(pre)
    return out, 1.13 * dpre + 0.5 * pre.abs() * 1.5e-7 + U4 * out.abs() + GELU_DEVICE_ERR


# ------------------------------------------------------------------------- LayerNorm --
def ln_lengths(c):
    """(hidden-state lengths, feature lengths) per utterance of a featurizer case."""
    if c["seg"] is not None:
        return list(np.diff(c["seg"])), list(np.diff(c["fseg"]))
    return [c["T"]] * (c["M"] // c["T"]), [c["Tout"]] * (c["M"] // c["T"])


def ln_reference(c):
    """dict(out, allow [M][D]; feat, dfeat [frows][D], written [frows] when the case has a featurizer)."""
    M, D = c["M"], c["D"]
    V4 = D // 256
    x = t64(c["x"])[:, :D]
    dx = torch.zeros_like(x)
    if c["add"] is not None:
        col = torch.arange(D)
        x = x + t64(c["add"])[:, (col // c["gin"]) * c["gout"] + col % c["gin"]]
        dx = EPS24 * x.abs()
    g, b = t64(c["gamma"]), t64(c["beta"])
    mu = x.mean(dim=1, keepdim=True)
    dmu = dx.mean(dim=1, keepdim=True) + (4 + (V4 - 1) + 6 + 2) * EPS24 * x.abs().mean(dim=1, keepdim=True)
    cc = x - mu
    dc = dx + dmu + EPS24 * cc.abs()
    var = (cc * cc).mean(dim=1, keepdim=True)
    dvar = (4 * V4 + 6 + 2) * EPS24 * var + (2 * cc.abs() * dc + dc * dc).mean(dim=1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + c["eps"])
    dr = rstd * (dvar / (2 * (var + c["eps"])) + 4 * EPS24)
    out = cc * rstd * g + b
    allow = g.abs() * (rstd * dc + cc.abs() * dr) + 2 * EPS24 * (cc * rstd * g).abs() + EPS24 * out.abs()
    r = dict(out=out, allow=allow)
    if c["feat_w"] is not None:
        fw = float(np.float32(c["feat_w"]))
        frows = c["frows"]
        y, dy = torch.zeros(frows, D, dtype=torch.float64), torch.zeros(frows, D, dtype=torch.float64)
        written = torch.zeros(frows, dtype=torch.bool)
        r0 = f0 = 0
        for T, Tout in zip(*ln_lengths(c)):
            n = min(T, Tout)
            idx = torch.cat([torch.arange(n), torch.full((Tout - n,), T - 1, dtype=torch.long)])  # last frame replicated
            y[f0:f0 + Tout], dy[f0:f0 + Tout] = out[r0 + idx], allow[r0 + idx]
            written[f0:f0 + Tout] = True
            r0, f0 = r0 + T, f0 + Tout
        prior = torch.zeros(frows, D, dtype=torch.float64) if c["feat_init"] else t64(c["prior"])
        r["feat"] = fw * y + prior
        r["dfeat"] = abs(fw) * dy + EPS24 * r["feat"].abs()
        r["written"] = written
    return r


# ----------------------------------------------------------------------------- conv0 --
def conv0_reference(c):
    """(want, allowance) [orows][512]."""
    w, g, b = t64(c["w"]), t64(c["gamma"]), t64(c["beta"])
    outs, allows = [], []
    for x in c["utts"]:  # the samples of each utterance (tail samples included)
        x = t64(x)
        fr = x.unfold(0, 10, 5)  # [T0][10]
        T0 = fr.shape[0]
        y = fr @ w.t()
        S = fr.abs() @ w.abs().t()
        mean = y.mean(dim=0, keepdim=True)
        var = ((y - mean) ** 2).mean(dim=0, keepdim=True)
        rstd = 1.0 / torch.sqrt(var + 1e-5)
        scale = rstd * g
        shift = b - mean * scale
        z = (y - mean) * scale + b
        dy = 10 * EPS24 * S
        dvar = 2 * (T0 + 128) * 2.0 ** -53 * (S * S).mean(dim=0, keepdim=True)
        dscale = scale.abs() * (dvar / (2 * (var + 1e-5)) + 3 * EPS24)
        dshift = mean.abs() * dscale + 3 * EPS24 * (mean * scale).abs() + EPS24 * shift.abs()
        dz = scale.abs() * dy + y.abs() * dscale + dshift + EPS24 * z.abs()
        out = gelu64(z)
        outs.append(out)
        allows.append(1.13 * dz + 0.5 * z.abs() * 1.5e-7 + U4 * out.abs() + GELU_DEVICE_ERR)
    return torch.cat(outs), torch.cat(allows)
