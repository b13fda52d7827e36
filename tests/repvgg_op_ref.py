"""Float64 reference and derived allowance for the RepVGG op-level cases (tests/repvgg_op_cases.py), and
CPU emulations of the kernels: a faithful one (bf16x3 products, f32 sums) and the wrong kernels the allowance
must reject (tests/test_repvgg_op_ref_cpu.py).

Allowance.  unit(K) = 2^-16 + (K + 8) 2^-24 is tests/conv_gemm_ref.py's bound of a bf16x3 product with f32
accumulation over K terms, per unit of S = sum |x| |w|.  A block: K = 17 cin live terms,

    unit(17 cin) S + 4 * 2^-24 (|pre| + |pre|),      pre = bias + conv,

the second term the f32 roundings of the bias add; through the ReLU, which is 1-Lipschitz, exactly as
tests/res2net_op_ref.py.  The stem's f32 FMA chain over K = 9 / 17 / 25 taps is inside the same bound
(its products are exact: no 2^-16 term is needed, but none is taken off either)."""
import numpy as np
import torch
import torch.nn.functional as F

from conv_gemm_ref import EPS24, to_bf16
from repvgg_op_cases import OP_BLOCK


def unit(K):
    return 2.0 ** -16 + (K + 8) * EPS24


def _t(x, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype)


def _image(c, x=None):
    """The case's input as (B, C, F, T)."""
    if c["op"] == OP_BLOCK:
        x = c["x"][:, :c["cin"]] if x is None else x
        return x.reshape(c["B"], c["Fi"], c["Ti"], c["cin"]).transpose(0, 3, 1, 2)
    return c["feats"].transpose(0, 2, 1)[:, None]  # (B, T, F) -> (B, 1, F, T)


def _rows(o):
    """(B, N, Fo, To) -> [M][N]"""
    return o.permute(0, 2, 3, 1).reshape(-1, o.shape[1])


def _conv(xi, w, stride):
    return F.conv2d(xi, w, stride=stride, padding=w.shape[-1] // 2)


def reference(c):
    """dict(out, pre, allow) of a block or stem case, float64; the stem's pad channels [C0, Cpad) are zeros."""
    stride = c.get("stride", 1)
    xi, w = _t(_image(c)), _t(c["w"])
    pre = _rows(_conv(xi, w, stride)) + _t(c["bias"])
    S = _rows(_conv(xi.abs(), w.abs(), stride))
    K = 17 * c["cin"] if c["op"] == OP_BLOCK else c["taps"]
    allow = unit(K) * S + 4 * EPS24 * (pre.abs() + pre.abs())
    out = pre.clamp_min(0.0)
    if c["op"] != OP_BLOCK and c["Cpad"] > c["C0"]:
        z = torch.zeros(out.shape[0], c["Cpad"] - c["C0"], dtype=torch.float64)
        pre, out, allow = torch.cat((pre, z), 1), torch.cat((out, z), 1), torch.cat((allow, z), 1)
    return dict(pre=pre, out=out, allow=allow)


# -------------------------------------------------------------------------- emulations --
def _x3(x, w, fn, single=False):
    """fn(x, w) as a bf16x3 product in f32: lo hi + hi lo + hi hi (single: hi hi only)."""
    xh, wh = to_bf16(x), to_bf16(w)
    xh_t, wh_t = _t(xh, torch.float32), _t(wh, torch.float32)
    y = fn(xh_t, wh_t)
    if single:
        return y
    xl_t, wl_t = _t(to_bf16(x - xh), torch.float32), _t(to_bf16(w - wh), torch.float32)
    return fn(xl_t, wh_t) + fn(xh_t, wl_t) + y


BLOCK_WRONG = ("dilated_at_inner_taps", "centre_from_one_branch", "stride_on_one_axis", "padding_1", "single_bf16",
               "bias_after_relu", "cross_utterance")


def emulate_block(c, wrong=None):
    """The block in f32 with bf16x3 products; `wrong` names one defect (BLOCK_WRONG)."""
    assert wrong is None or wrong in BLOCK_WRONG
    s, B, Fi, Ti, Fo, To = c["stride"], c["B"], c["Fi"], c["Ti"], c["Fo"], c["To"]
    w = c["w"]
    if wrong == "dilated_at_inner_taps":
        w = np.zeros_like(w)
        w[:, :, 1:4, 1:4] = c["w3"] + c["wd"]
    elif wrong == "centre_from_one_branch":
        w = w.copy()
        w[:, :, 2, 2] = c["w3"][:, :, 1, 1]
    xi = np.ascontiguousarray(_image(c))

    def conv(xt, wt):
        if wrong == "stride_on_one_axis":  # output column `to` reads input column `to`, not `to * s`
            return F.conv2d(xt, wt, stride=(s, 1), padding=2)[:, :, :, :To]
        if wrong == "padding_1":  # tap (kf, kt) reads (fo s + kf - 1, to s + kt - 1)
            return F.conv2d(F.pad(xt, (1, 3, 1, 3)), wt, stride=s)
        if wrong == "cross_utterance":  # the batch as one tall plane: rows of the neighbouring utterance are read
            tall = xt.permute(1, 0, 2, 3).reshape(1, xt.shape[1], B * Fi, Ti)
            o = F.conv2d(tall, wt, stride=s, padding=2)
            assert o.shape[2] == B * Fo, "pick a case whose F is even, or stride 1"
            return o.reshape(o.shape[1], B, Fo, To).permute(1, 0, 2, 3)
        return F.conv2d(xt, wt, stride=s, padding=2)

    acc = _rows(_x3(xi, w, conv, wrong == "single_bf16"))
    b = _t(c["bias"], torch.float32)
    if wrong == "bias_after_relu":
        return (acc.clamp_min(0.0) + b).double()
    return (acc + b).clamp_min(0.0).double()


def emulate_stem(c):
    """The stem in f32 (its products are exact f32 FMAs)."""
    xi, w = _t(_image(c), torch.float32), _t(c["w"], torch.float32)
    out = (_rows(_conv(xi, w, 1)) + _t(c["bias"], torch.float32)).clamp_min(0.0).double()
    if c["Cpad"] > c["C0"]:
        out = torch.cat((out, torch.zeros(out.shape[0], c["Cpad"] - c["C0"], dtype=torch.float64)), 1)
    return out


def ratio(got, r):
    """max |got - reference| / allowance; an element whose allowance is 0 (a pad channel) must be exact."""
    err = (got - r["out"]).abs()
    if bool(((r["allow"] == 0) & (err > 0)).any()):
        return float("inf")
    return float((err / r["allow"].clamp_min(1e-300)).max())
