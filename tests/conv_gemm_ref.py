"""Float64 reference, error bound and case files for the implicit-GEMM conv kernels.

The contract is `ConvGemmArgs` (wespeaker_hubert_amd/csrc/kernels.h).  `reference()` computes it
with torch.nn.functional.conv1d / conv2d in float64 -- one call per utterance for ragged batches,
`groups=` for grouped columns, explicit slices for the concat segments and the `sc2d` shortcut --
and never reproduces the kernels' index arithmetic.  The epilogue is
    out = act(y + bias + row_bias + res) * scale + shift      (GELU: exact erf form).

Error bound (no free constants).  With S[m][n] = sum |a| |w| over the same taps:
  * bf16x3 products: bf16 rounds to 2^-9 relative, so hi + lo represents an operand to 2^-18;
    the dropped a_lo * w_lo term is <= 2^-18 |a||w|; together <= 3 * 2^-18 S < 2^-16 S.
    (`prod_exp` = 17 for the split-term probes, where one operand has no lo part and the two
    surviving terms must reproduce the products.)  The f32 kernel (precision 0) has no such term.
  * f32 accumulation: <= (K + 8) * 2^-24 S.
  * both pass through the activation (none / ReLU: 1-Lipschitz) and are multiplied by |scale|.
  * the f32 epilogue: <= 4 * 2^-24 (|pre-activation| + |scale * act| + |shift|).
tanh and GELU are checked in two steps instead (`act_expected`): the same operands with act = none
are held to the bound above, then the kernel's activation output is compared with the float64
activation of the kernel's OWN act-none output, within the activation's own error.

Case files: `op_cases` / `read_cases` / `results_of` map a case onto the header, arrays, results and
own words of tools/conv_gemm_run.cpp's op table; the file format itself is tests/op_runner.py's.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import op_runner
from op_runner import FILL  # noqa: F401

MAGIC, OP_CONV_GEMM = 0x43505357, 1
NH = op_runner.LAYOUT["conv_gemm_run"][0]  # 42 ints + ln_eps
ACT_NONE, ACT_RELU, ACT_TANH, ACT_GELU = 0, 1, 2, 3
EPS24 = 2.0 ** -24

HDR = ["variant", "precision", "flags", "lda0", "lda1", "lda2", "cseg0", "cseg1", "cseg2", "cseg3", "cin", "taps",
       "dil", "pad", "M", "T", "N", "ldres", "ldo", "act", "amode", "role", "conv2d", "Fi", "Ti", "Fo", "To",
       "stride", "kw", "sc2d", "gcols", "gcin", "nseg", "lnmode", "ln_parts", "arows0", "arows1", "arows2",
       "aoff0", "aoff1", "aoff2", "B"]
F_BIAS, F_ROWBIAS, F_RES, F_SCALE, F_SEG, F_ISEG, F_COLSUM, F_LNIN, F_LNCS, F_LNGB = (
    8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096)


def make_case(**kw):
    """A case with the 1-D single-operand defaults; `a` = list of up to 3 float32 [rows][lda]
    buffers, `w` = float32 [N][cin][taps] (2-D: [N][cin][kh][kw])."""
    c = dict(variant=5, precision=1, dil=1, pad=0, act=ACT_NONE, amode=0, role=0, conv2d=0, Fi=0, Ti=0, Fo=0,
             To=0, stride=0, kw=0, sc2d=0, gcols=0, gcin=0, lnmode=0, ln_parts=0, ln_eps=0.0, aoff=[0, 0, 0],
             bias=None, row_bias=None, res=None, scale=None, shift=None, seg=None, iseg=None, colsum=False,
             ln_in=None, ln_cs=None, ln_g=None, ln_b=None, prod_exp=16, name="")
    c.update(kw)
    a = list(c["a"]) + [None] * (3 - len(c["a"]))
    c["a"] = a
    w = c["w"]
    c["N"], c["cin"] = int(w.shape[0]), int(w.shape[1])
    c["taps"] = int(np.prod(w.shape[2:]))
    if "cseg" not in kw:
        c["cseg"] = [0, c["cin"], c["cin"], c["cin"]]
    c.setdefault("ldo", c["N"])
    c["ldres"] = 0 if c["res"] is None else int(c["res"].shape[1])
    if c["seg"] is not None:
        c["B"] = len(c["seg"]) - 1
    elif "B" not in kw:
        c["B"] = c["M"] // c["T"]
    return c


def with_(case, **kw):
    c = dict(case)
    c.update(kw)
    return c


def _flags(c):
    f = sum(1 << i for i in range(3) if c["a"][i] is not None)
    for bit, key in ((F_BIAS, "bias"), (F_ROWBIAS, "row_bias"), (F_RES, "res"), (F_SCALE, "scale"), (F_SEG, "seg"),
                     (F_ISEG, "iseg"), (F_LNIN, "ln_in"), (F_LNCS, "ln_cs"), (F_LNGB, "ln_g")):
        if c[key] is not None:
            f |= bit
    return f | (F_COLSUM if c["colsum"] else 0)


def _header(c):
    a = c["a"]
    h = dict(c)
    h["flags"] = _flags(c)
    for i in range(3):
        h[f"lda{i}"] = 0 if a[i] is None else a[i].shape[1]
        h[f"arows{i}"] = 0 if a[i] is None else a[i].shape[0]
        h[f"aoff{i}"] = c["aoff"][i]
    for i in range(4):
        h[f"cseg{i}"] = c["cseg"][i]
    h["nseg"] = 0 if c["seg"] is None else len(c["seg"]) - 1
    return [int(h[k]) for k in HDR]


# optional arrays in file order: (flag bit, keys); the a[] buffers and `colsum` have no key of their own
_OPTIONAL = ((F_BIAS, ("bias",)), (F_ROWBIAS, ("row_bias",)), (F_RES, ("res",)), (F_SCALE, ("scale", "shift")),
             (F_SEG, ("seg",)), (F_ISEG, ("iseg",)), (F_LNIN, ("ln_in",)), (F_LNCS, ("ln_cs",)), (F_LNGB, ("ln_g", "ln_b")))
_INT_KEYS = ("seg", "iseg")


def _arrays(c):
    """The case's arrays in the op table's order: a[0..2], w, then the flagged ones."""
    out = [np.asarray(x, np.float32) for x in c["a"] + [c["w"]] if x is not None]
    for bit, keys in _OPTIONAL:
        if _flags(c) & bit:
            out += [np.asarray(c[k], np.int32 if k in _INT_KEYS else np.float32) for k in keys]
    return out


def op_cases(cases):
    """(op, header, arrays) per case; ln_eps travels as f32 in the header's last word."""
    return [(OP_CONV_GEMM, _header(c) + [int(np.float32(c["ln_eps"]).view(np.int32))], _arrays(c)) for c in cases]


def write_cases(path, cases):
    op_runner.write_cases(path, MAGIC, op_cases(cases), NH)


def _narrays(op, hdr):
    assert op == OP_CONV_GEMM
    fl = hdr[HDR.index("flags")]
    return bin(fl & 7).count("1") + 1 + sum(len(keys) for bit, keys in _OPTIONAL if fl & bit)


def read_cases(path):
    """Header fields by name and arrays by key, shaped as the header says (the reverse of write_cases)."""
    out = []
    for _, hdr, arrays in op_runner.read_cases(path, MAGIC, NH, _narrays):
        h = dict(zip(HDR, hdr))
        h["ln_eps"] = float(np.int32(hdr[-1]).view(np.float32))
        arrays = iter(arrays)
        fl = h["flags"]
        h["a"] = [next(arrays).reshape(h[f"arows{i}"], h[f"lda{i}"]) if fl & (1 << i) else None for i in range(3)]
        h["w"] = next(arrays).reshape(h["N"], h["cin"], h["taps"])
        for bit, keys in _OPTIONAL:
            for k in keys:
                h[k] = (next(arrays).view(np.int32) if k in _INT_KEYS else next(arrays)) if fl & bit else None
        if h["row_bias"] is not None:
            h["row_bias"] = h["row_bias"].reshape(h["B"], h["N"])
        if h["res"] is not None:
            h["res"] = h["res"].reshape(h["M"], h["ldres"])
        h["colsum"] = bool(fl & F_COLSUM)
        out.append(h)
    return out


def results_of(raw, cases):
    """op_runner results -> status, message, tile and block_rows (the record's own words), out, means, ln_out."""
    res = []
    for c, r in zip(cases, raw):
        tile, bm = r["own"][:24].split(b"\0")[0].decode(), int.from_bytes(r["own"][24:], "little", signed=True)
        r = dict(status=r["status"], message=r["message"], tile=tile, block_rows=bm, arrays=r["arrays"])
        if r["status"] == 0:
            out, r["means"], r["ln_out"] = r.pop("arrays")
            r["out"] = out.reshape(c["M"] + 8, c["ldo"])
        res.append(r)
    return res


# ------------------------------------------------------------------ inputs --
def rand_a(rng, rows, ld, relu=False):
    """Activations in [-1, 1] (post-ReLU: half of them zero), pad columns included."""
    x = rng.uniform(-1.0, 1.0, size=(rows, ld)).astype(np.float32)
    return np.maximum(x, 0.0) if relu else x


def rand_w(rng, *shape, amp=0.05):
    return rng.uniform(-amp, amp, size=shape).astype(np.float32)


def to_bf16(x):
    """float32 -> nearest-even bf16, as float32 (torch's conversion; finite inputs)."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).bfloat16().float().numpy()


# --------------------------------------------------------------- reference --
def lengths(c):
    """(input rows, output rows) per utterance of a 1-D case."""
    if c["seg"] is not None:
        so = np.asarray(c["seg"], dtype=np.int64)
        si = so if c["iseg"] is None else np.asarray(c["iseg"], dtype=np.int64)
        return list(np.diff(si)), list(np.diff(so))
    Ti = c["Ti"] if c["Ti"] > 0 else c["T"]
    return [Ti] * c["B"], [c["T"]] * c["B"]


def utterance_of_rows(c):
    if c["conv2d"] or c["sc2d"]:
        return np.repeat(np.arange(c["B"]), c["M"] // c["B"])
    return np.repeat(np.arange(c["B"]), lengths(c)[1])


def _view(c, i, lo, width):
    off = c["aoff"][i]
    return torch.from_numpy(np.ascontiguousarray(c["a"][i])).double()[:, off + lo:off + lo + width]


def operand(c):
    """The logical input rows X [rows][channels]: concat segments / the added pair / the groups'
    channel ranges laid side by side."""
    cin, cs = c["cin"], c["cseg"]
    if c["amode"] == 1:
        return _view(c, 0, 0, cin) + _view(c, 1, 0, cin)
    if c["gcols"]:
        return torch.cat([_view(c, 0, g * c["gcin"], cin) for g in range(c["N"] // c["gcols"])], dim=1)
    return torch.cat([_view(c, i, 0, cs[i + 1] - cs[i]) for i in range(3) if cs[i + 1] > cs[i]], dim=1)


def _gemm_pair(c, fn):
    """fn(x, w) on the operands and on their absolute values -> (y, S)."""
    w = torch.from_numpy(np.ascontiguousarray(c["w"])).double()
    x = operand(c) if not c["sc2d"] else None
    return fn(x, w), fn(None if x is None else x.abs(), w.abs(), True)


def conv_y_S(c):
    """y [M][N] (the bare convolution) and S = sum |a||w|, float64."""
    M, N, cin = c["M"], c["N"], c["cin"]
    groups = c["N"] // c["gcols"] if c["gcols"] else 1

    def run(x, w, absolute=False):
        if c["sc2d"]:
            c1 = c["cseg"][1]
            B, Fi, Ti, Fo, To, st = c["B"], c["Fi"], c["Ti"], c["Fo"], c["To"], c["stride"]
            x0 = _view(c, 0, 0, c1)[:M]
            x1 = _view(c, 1, 0, cin - c1)[:B * Fi * Ti].reshape(B, Fi, Ti, cin - c1)
            x1 = x1[:, ::st, ::st][:, :Fo, :To].reshape(M, cin - c1)
            if absolute:
                x0, x1 = x0.abs(), x1.abs()
            w2 = w.reshape(N, cin)
            return x0 @ w2[:, :c1].t() + x1 @ w2[:, c1:].t()
        if c["conv2d"]:
            B, Fi, Ti, Fo, To = c["B"], c["Fi"], c["Ti"], c["Fo"], c["To"]
            kw = c["kw"]
            w4 = w.reshape(N, cin, c["taps"] // kw, kw)
            xi = x[:B * Fi * Ti].reshape(B, Fi, Ti, cin).permute(0, 3, 1, 2)
            y = F.conv2d(xi, w4, stride=c["stride"], padding=c["pad"])
            assert y.shape[2] >= Fo and y.shape[3] >= To
            return y[:, :, :Fo, :To].permute(0, 2, 3, 1).reshape(M, N)
        w3 = w.reshape(N, cin, c["taps"])
        st = max(c["stride"], 1)
        li, lo = lengths(c)
        ys, r0 = [], 0
        for ti, to in zip(li, lo):
            xi = x[r0:r0 + ti].t().unsqueeze(0)
            r0 += ti
            # frames past the utterance read zero: pad the right generously, keep the first `to`
            xi = F.pad(xi, (c["pad"], c["pad"] + to * st + c["dil"] * c["taps"]))
            y = F.conv1d(xi, w3, stride=st, dilation=c["dil"], groups=groups)
            ys.append(y[0, :, :to].t())
        return torch.cat(ys, dim=0)

    y, S = _gemm_pair(c, run)
    assert y.shape == (M, N)
    return y, S


def act_f64(y, act):
    if act == ACT_RELU:
        return torch.clamp(y, min=0.0)
    if act == ACT_TANH:
        return torch.tanh(y)
    if act == ACT_GELU:
        return 0.5 * y * (1.0 + torch.erf(y / math.sqrt(2.0)))
    return y


def _vec(x, shape=None):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).double()


def reference(c, y_S=None):
    """dict(y, S, pre, act, out, bound), float64 tensors [M][N]."""
    y, S = conv_y_S(c) if y_S is None else y_S
    N = c["N"]
    pre = y.clone()
    if c["bias"] is not None:
        pre = pre + _vec(c["bias"])
    if c["row_bias"] is not None:
        pre = pre + _vec(c["row_bias"]).reshape(c["B"], N)[torch.from_numpy(utterance_of_rows(c))]
    if c["res"] is not None:
        pre = pre + _vec(c["res"])[:, :N]
    a = act_f64(pre, c["act"])
    scale = torch.ones(N, dtype=torch.float64) if c["scale"] is None else _vec(c["scale"])
    shift = torch.zeros(N, dtype=torch.float64) if c["scale"] is None else _vec(c["shift"])
    out = a * scale + shift
    K = c["cin"] * c["taps"]
    gemm = ((2.0 ** -c["prod_exp"] if c["precision"] else 0.0) + (K + 8) * EPS24) * S
    bound = scale.abs() * gemm + 4 * EPS24 * (pre.abs() + (a * scale).abs() + shift.abs())
    return dict(y=y, S=S, pre=pre, act=a, out=out, bound=bound)


# A&S 7.1.26 erf (common.h gelu_as): |erf error| <= 1.5e-7 -> 0.5 |y| 1.5e-7 on GELU; 4 f32 ulps
# for the float arithmetic around it.  The device's own __expf / tanhf contribution is measured on
# the MI355X (tests/test_gpu_conv_gemm_op.py records the figures) and enters as `device_err`.
def act_expected(y_none, c, device_err):
    """Step (b): float64 activation of the kernel's own act-none output (`y_none`, float32, the
    output of the same case with act = none and no scale) and the deviation allowed."""
    y = torch.from_numpy(np.ascontiguousarray(y_none)).double()
    a = act_f64(y, c["act"])
    N = c["N"]
    scale = torch.ones(N, dtype=torch.float64) if c["scale"] is None else _vec(c["scale"])
    shift = torch.zeros(N, dtype=torch.float64) if c["scale"] is None else _vec(c["shift"])
    own = 4 * 2.0 ** -23 * a.abs() + device_err
    if c["act"] == ACT_GELU:
        own = own + 0.5 * y.abs() * 1.5e-7
    tol = scale.abs() * own + 4 * EPS24 * ((a * scale).abs() + shift.abs())
    return a * scale + shift, tol


# ------------------------------------------------------- LayerNorm fold --
U8 = 8 * 2.0 ** -23  # 8 f32 ulps: what the kernel's mean / rstd (merged from ln_in in f32) may be off


def reference_ln(c):
    """The LayerNorm-fold modes (ConvGemmArgs::lnmode) against the float64 LayerNorm.
    mode 1: y = conv + bias + res.  mode 2: y = LayerNorm0(A) W'^T + b' (LayerNorm0 = without the
    affine part, which the case folded into W' and b').  modes 4 / 5: y = conv + bias +
    LayerNorm(res; ln_g, ln_b).  The bound is the GEMM bound with, for mode 2,
    S = rstd (sum |a||w'| + |mu||ln_cs|) -- the two terms that cancel -- plus 8 f32 ulps on the
    kernel's mean and rstd, plus the f32 epilogue."""
    mode, N, K = c["lnmode"], c["N"], c["cin"] * c["taps"]
    y, S = conv_y_S(c)
    bias = _vec(c["bias"]) if c["bias"] is not None else torch.zeros(N, dtype=torch.float64)
    unit = 2.0 ** -16 + (K + 8) * EPS24
    if mode == 2:
        A = operand(c)
        mu = A.mean(dim=1, keepdim=True)
        rstd = 1.0 / torch.sqrt(A.var(dim=1, unbiased=False, keepdim=True) + c["ln_eps"])
        w = _vec(c["w"]).reshape(N, -1)
        core = F.layer_norm(A, (A.shape[1],), eps=c["ln_eps"]) @ w.t()
        cs = _vec(c["ln_cs"]).abs()
        pre = core + bias
        a = act_f64(pre, c["act"])
        bound = (unit * rstd * (S + mu.abs() * cs) + U8 * (rstd * mu.abs() * cs + core.abs())
                 + 4 * EPS24 * (pre.abs() + core.abs() + a.abs()))
        return dict(out=a, bound=bound, S=S)
    r = _vec(c["res"])[:, :N]
    pre = y + bias
    extra = 0.0
    if mode & 4:
        mu = r.mean(dim=1, keepdim=True)
        rstd = 1.0 / torch.sqrt(r.var(dim=1, unbiased=False, keepdim=True) + c["ln_eps"])
        g, b = _vec(c["ln_g"]), _vec(c["ln_b"])
        ln = F.layer_norm(r, (N,), g, b, eps=c["ln_eps"])
        pre = pre + ln
        # (res - mu) rstd g + b in f32: 8 ulps on mu and on rstd, one rounding per operation
        extra = (2.0 ** -23 * rstd * g.abs() * (8 * mu.abs() + 8 * (r - mu).abs() + 2 * (r.abs() + mu.abs()))
                 + 2 * EPS24 * (ln.abs() + b.abs()))
    else:
        pre = pre + r
    bound = unit * S + extra + 4 * EPS24 * (pre.abs() + (y + bias).abs() + pre.abs())
    return dict(out=pre, bound=bound, S=S)


def ln_out_ratio(y_kernel, ln_out):
    """ln_out [M][N / 128][2] = (mean, M2) of each 128-column piece of the kernel's own y, against
    float64 statistics of that y.  The kernel forms them from 4 values per lane and 5 pairwise
    merges (about 9 roundings on the mean, under 64 on M2), every intermediate bounded by
    max |y| and Q = sum (|y| + |mean|)^2: mean within 16 * 2^-24 max |y|, M2 within 64 * 2^-24 Q.
    Returns max(|err| / tolerance)."""
    M, N = y_kernel.shape
    p = torch.from_numpy(np.array(y_kernel)).double().reshape(M, N // 128, 128)
    mean = p.mean(dim=2)
    m2 = ((p - mean[:, :, None]) ** 2).sum(dim=2)
    got = torch.from_numpy(np.array(ln_out)).double().reshape(M, N // 128, 2)
    tol_mean = 16 * EPS24 * p.abs().amax(dim=2)
    tol_m2 = 64 * EPS24 * ((p.abs() + mean.abs()[:, :, None]) ** 2).sum(dim=2)
    return max(float(((got[:, :, 0] - mean).abs() / tol_mean).max()), float(((got[:, :, 1] - m2).abs() / tol_m2).max()))
