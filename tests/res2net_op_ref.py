"""Float64 reference and derived allowance for the Res2Net op-level cases (tests/res2net_op_cases.py),
and CPU emulations of the kernels: a faithful one (bf16x3 products, f32 sums) and the wrong kernels the
allowance must reject (tests/test_res2net_op_ref_cpu.py).

Allowance.  unit(K) = 2^-16 + (K + 8) 2^-24 is tests/conv_gemm_ref.py's bound of a bf16x3 product
with f32 accumulation over K terms, per unit of S = sum |a| |w|.

  1x1 conv over the concatenated operand: the ERes2Net op tests' bound as it stands,
      unit(cin) S + 4 * 2^-24 (|pre| + |pre|), through the 1-Lipschitz activation.

  fused tail:
      ds   = unit(9 w) S1 + 4 * 2^-24 |pre1|          pre1 = b1 + conv3x3(y[:, :w]), s = clamp(pre1)
             (the 3x3 conv's allowance; 0 where pre1 lies further than that outside [0, 20]: the clamp
             passes no error there)
      dz   = |W3[:, :w]| ds                            s's error through conv3
           + unit(2 w) S2                              S2 = |W3| |[s | y[:, w:]]|: the second product's own
                                                       bound (the split of the f32 s is inside it)
           + 4 * 2^-24 (|z + b3| + |pre|)              pre = z + b3 + res: the two f32 roundings of the epilogue
      through the final clamp, which is 1-Lipschitz.
"""
import numpy as np
import torch
import torch.nn.functional as F

from conv_gemm_ref import EPS24, to_bf16

CLAMP_LO, CLAMP_HI = 0.0, 20.0


def unit(K):
    return 2.0 ** -16 + (K + 8) * EPS24


def _t(x, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype)


def _act(v, act):
    if act == 2:
        return v.clamp(CLAMP_LO, CLAMP_HI)
    return v.clamp_min(0.0) if act == 1 else v


def _conv3x3(x, w, B, Fh, T):
    """x [M][c] rows over [B][F][T] -> [M][n], zero padding at each utterance's plane edge."""
    c, n = x.shape[1], w.shape[0]
    xi = x.reshape(B, Fh, T, c).permute(0, 3, 1, 2)
    return F.conv2d(xi, w, padding=1).permute(0, 2, 3, 1).reshape(B * Fh * T, n)


# ------------------------------------------------------------------ float64 references --
def tail_reference(c):
    """dict(s, pre1, out, pre, allow) of a tail case, float64."""
    w, B, Fh, T = c["w"], c["B"], c["F"], c["T"]
    y = _t(c["y"])[:, :2 * w]
    w1, b1, w3, b3 = _t(c["w1"]), _t(c["b1"]), _t(c["w3"]), _t(c["b3"])
    pre1 = _conv3x3(y[:, :w], w1, B, Fh, T) + b1
    S1 = _conv3x3(y[:, :w].abs(), w1.abs(), B, Fh, T)
    s = pre1.clamp(CLAMP_LO, CLAMP_HI)
    ds = unit(9 * w) * S1 + 4 * EPS24 * pre1.abs()
    ds = torch.where((pre1 < CLAMP_LO - ds) | (pre1 > CLAMP_HI + ds), torch.zeros_like(ds), ds)
    u = torch.cat((s, y[:, w:]), 1)
    z = u @ w3.t() + b3
    pre = z + (_t(c["res"])[:, :c["N"]] if c["has_res"] else 0.0)
    S2 = u.abs() @ w3.abs().t()
    allow = ds @ w3[:, :w].abs().t() + unit(2 * w) * S2 + 4 * EPS24 * (z.abs() + pre.abs())
    return dict(s=s, pre1=pre1, pre=pre, out=pre.clamp(CLAMP_LO, CLAMP_HI), allow=allow)


def pw_reference(c):
    """dict(out, pre, allow) of a concatenated-operand 1x1 case, float64."""
    ks, cin, st = c["ksplit"], c["cin"], c["stride"]
    x = torch.cat((_t(c["a"])[:, :ks], _t(c["a2"])[:, :cin - ks]), 1)
    x = x.reshape(c["B"], c["Fi"], c["Ti"], cin)[:, ::st, ::st].reshape(c["M"], cin)
    w = _t(c["w"]).reshape(c["N"], cin)
    pre = x @ w.t() + _t(c["bias"]) + (_t(c["res"]) if c["has_res"] else 0.0)
    S = x.abs() @ w.abs().t()
    return dict(pre=pre, out=_act(pre, c["act"]), allow=unit(cin) * S + 4 * EPS24 * (pre.abs() + pre.abs()))


# -------------------------------------------------------------------------- emulations --
def _x3(x, w, fn, single=False):
    """fn(x, w) as a bf16x3 product in f32: hi hi + hi lo + lo hi (single: hi hi only)."""
    xh, wh = to_bf16(x), to_bf16(w)
    xh_t, wh_t = _t(xh, torch.float32), _t(wh, torch.float32)
    y = fn(xh_t, wh_t)
    if single:
        return y
    xl_t, wl_t = _t(to_bf16(x - xh), torch.float32), _t(to_bf16(w - wh), torch.float32)
    return fn(xl_t, wh_t) + fn(xh_t, wl_t) + y


TAIL_WRONG = ("pass_first_slice", "no_clamp_s", "no_ceiling_out", "swap_kf_kt", "edge_clamp", "no_residual",
              "single_bf16", "cross_utterance")


def emulate_tail(c, wrong=None):
    """The tail in f32 with bf16x3 products; `wrong` names one defect (TAIL_WRONG)."""
    assert wrong is None or wrong in TAIL_WRONG
    w, B, Fh, T, N = c["w"], c["B"], c["F"], c["T"], c["N"]
    y = np.ascontiguousarray(c["y"][:, :2 * w])
    w1 = c["w1"].transpose(0, 1, 3, 2).copy() if wrong == "swap_kf_kt" else c["w1"]
    single = wrong == "single_bf16"

    def conv(x, wt):
        if wrong == "cross_utterance":  # the batch as one tall plane: rows of the neighbouring utterance are read
            return _conv3x3(x, wt, 1, B * Fh, T)
        if wrong == "edge_clamp":
            xi = x.reshape(B, Fh, T, w).permute(0, 3, 1, 2)
            xi = F.pad(xi, (1, 1, 1, 1), mode="replicate")
            return F.conv2d(xi, wt).permute(0, 2, 3, 1).reshape(B * Fh * T, w)
        return _conv3x3(x, wt, B, Fh, T)

    pre1 = _x3(y[:, :w], w1, conv, single) + _t(c["b1"], torch.float32)
    s = pre1 if wrong == "no_clamp_s" else pre1.clamp(CLAMP_LO, CLAMP_HI)
    y2 = y[:, :w] if wrong == "pass_first_slice" else y[:, w:]
    u = np.concatenate((s.numpy(), y2), 1)
    z = _x3(u, c["w3"], lambda a, b: a @ b.t(), single) + _t(c["b3"], torch.float32)
    if c["has_res"] and wrong != "no_residual":
        z = z + _t(c["res"], torch.float32)[:, :N]
    return (z.clamp_min(0.0) if wrong == "no_ceiling_out" else z.clamp(CLAMP_LO, CLAMP_HI)).double()


PW_WRONG = ("ksplit_off_by_8", "single_bf16")


def emulate_pw(c, wrong=None):
    assert wrong is None or wrong in PW_WRONG
    cin, st = c["cin"], c["stride"]
    ks = c["ksplit"] + (8 if wrong == "ksplit_off_by_8" else 0)
    x = np.concatenate((c["a"][:, :ks], c["a2"][:, :cin - ks]), 1)
    x = np.ascontiguousarray(x.reshape(c["B"], c["Fi"], c["Ti"], cin)[:, ::st, ::st].reshape(c["M"], cin))
    z = _x3(x, c["w"].reshape(c["N"], cin), lambda a, b: a @ b.t(), wrong == "single_bf16")
    z = z + _t(c["bias"], torch.float32)
    if c["has_res"]:
        z = z + _t(c["res"], torch.float32)
    return _act(z, c["act"]).double()


def ratio(got, r):
    """max |got - reference| / allowance."""
    return float(((got - r["out"]).abs() / r["allow"]).max())
