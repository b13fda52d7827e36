"""Float64 references and allowances of the ResNet / SimAM-ResNet kernels (tests/test_gpu_resnet_op.py
on the MI355X, tests/test_resnet_op_ref_cpu.py against numpy emulations).  Every function takes a case
dict of tests/resnet_op_cases.py and returns float64 arrays shaped as the kernel's output; the
convolutions are torch.nn.functional.conv2d in float64, one call per utterance, and never reproduce the
kernels' index arithmetic.  Every allowance is a function of the inputs and the float64 reference only,
never of a kernel's output (the next conv1 of the fused tail is the one stated exception: its reference
input is the kernel's own `out`, as the issue of this test sets it).  First order in u throughout.

u = 2^-24 (one f32 rounding, relative).  GEMM(K) = 2^-16 + (K + 8) u is DESIGN.md section 4's conv-GEMM
bound per unit of S = sum |a||w| (bf16x3 products: 3 x 2^-18 < 2^-16; f32 accumulation over K).

conv3x3   out = act(conv(x, W) + bias (+ res)) scale + shift, act = ReLU or none:
            |scale| GEMM(9C) S + 4u (|pre| + |scale act(pre)| + |shift|)          (tests/conv_gemm_ref.py's bound)
tail      y2 = relu(conv2(y1) + b2), out = relu(conv3(y2) (+ sc(x)) + b3 (+ res)):
            A2   = GEMM(9C) S2 + u |pre2|                  conv2 and the one rounding of acc + b2
            out: A2 |W3|^T                                 A2 through the ReLU (1-Lipschitz) and conv3
                 + GEMM(K3) S3                             conv3's own products and sums on |y2| (y2's bf16 split is
                                                           of its f32 value; with xsc the shortcut's products join:
                                                           S3 = |y2||W3|^T + |x||Wsc|^T, K3 = 2C, else K3 = C)
                 + 2u (|acc3| + |b3| + |res|)              the two additions of the epilogue
          y1n = relu(conv1(out~) + b1) on the kernel's own out~ (float32):
            GEMM(4C) |out~||W1|^T + u (|acc1| + |b1|)
stem      relu(bias + sum of 9 products), nine f32 FMAs and the bias:  (9 + 2) u (S + |bias|)
simam     out = relu(z g + res), g = sigmoid(e), e = d^2 k + 0.5, d = z - mean, k = 1 / (4 (var + 1e-4)), mean and
          var (n - 1) per (utterance, channel) over the n rows.  The kernel sums z and z^2 in f64, forms mean and
          var = (s2 - s1 mean) / (n - 1) in f64, rounds mean, var and k to f32 and applies the gate in f32:
            dmean = (n + 4) 2^-53 mean|z| + u |mean|
            dvar  = (n + 4) 2^-53 (s2 + n mean^2) / (n - 1) + u var       (the two terms that cancel, each summed in f64)
            dk    = k dvar / (var + 1e-4) + u k
            dd    = dmean + u |d|                                         (the f32 subtraction)
            de    = 2 |d| k dd + d^2 dk + 2u d^2 k + u e                  (d * d, * k, + 0.5)
            dg    = g (1 - g) (de + u + E_EXP) + 2u g                     (exp's argument and rounding; 1 + E; the division)
            allow = |z| dg + u |z g + res|                                (one fmaf; ReLU is 1-Lipschitz)
          The kernel's coefficient buffer (f32 mean and k per utterance and channel) is held to dmean and dk as well.
          E_EXP is the device part of `expf`, relative: what it is off beyond one correct rounding.
tfc       the numpy transpose, allowance 0 (bit-equal).

Measured on the MI355X (tests/test_gpu_resnet_op.py's docstring has the ratios): with E_EXP at 0 no element
exceeds its allowance, so 0 ships.
"""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
LAMBDA = 1e-4

# The device part of `expf` in SimAM's sigmoid, measured with the term at 0 (test_gpu_resnet_op.py): no
# element exceeded its allowance without it, so 0 ships.
E_EXP = 0.0


def gemm_unit(K):
    return 2.0 ** -16 + (K + 8) * U


def t64(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))


def f64(x):
    return np.asarray(x, np.float64)


def conv2d(x, W):
    """x [B][F][T][C], W [N][C][3][3] -> [B][F][T][N]: zero padding 1, stride 1, every utterance on its own."""
    w = t64(W)
    return np.stack([F.conv2d(t64(xb).permute(2, 0, 1)[None], w, padding=1)[0].permute(1, 2, 0).numpy() for xb in x])


# ------------------------------------------------------------------------------ conv3x3 --
def conv3x3_reference(c):
    """(out, allow, pre) [B][F][T][C]."""
    x, W = f64(c["x"]), f64(c["W"])
    pre = conv2d(x, W) + f64(c["bias"])
    if c["res"] is not None:
        pre = pre + f64(c["res"])
    S = conv2d(np.abs(x), np.abs(W))
    a = np.maximum(pre, 0.0) if c["relu"] else pre
    scale = np.ones(c["C"]) if c["scale"] is None else f64(c["scale"])
    shift = np.zeros(c["C"]) if c["shift"] is None else f64(c["shift"])
    allow = np.abs(scale) * gemm_unit(9 * c["C"]) * S + 4 * U * (np.abs(pre) + np.abs(a * scale) + np.abs(shift))
    return a * scale + shift, allow, pre


# --------------------------------------------------------------------------------- tail --
def tail_reference(c):
    """dict(out, allow, pre2, pre3) with out [B][F][T][4C]."""
    C = c["C"]
    y1, W2 = f64(c["y1"]), f64(c["W2"])
    pre2 = conv2d(y1, W2) + f64(c["b2"])
    A2 = gemm_unit(9 * C) * conv2d(np.abs(y1), np.abs(W2)) + U * np.abs(pre2)
    y2 = np.maximum(pre2, 0.0)
    W3 = f64(c["W3"])
    W3c = W3[:, :C]
    acc3 = y2 @ W3c.T
    S3 = y2 @ np.abs(W3c).T  # y2 >= 0
    K3 = C
    if c["xsc"]:
        xs, Wsc = f64(c["xs"]), W3[:, C:]
        acc3 = acc3 + xs @ Wsc.T
        S3 = S3 + np.abs(xs) @ np.abs(Wsc).T
        K3 = 2 * C
    b3 = f64(c["b3"])
    res = 0.0 if c["res"] is None else f64(c["res"])
    pre3 = acc3 + b3 + res
    allow = A2 @ np.abs(W3c).T + gemm_unit(K3) * S3 + 2 * U * (np.abs(acc3) + np.abs(b3) + np.abs(res))
    return dict(out=np.maximum(pre3, 0.0), allow=allow, pre2=pre2, pre3=pre3)


def next_conv1_reference(c, out):
    """(y1n, allow, pre) [B][F][T][c1n]: the float64 next conv1 of `out` (the kernel's own, float32)."""
    src, W1, b1 = f64(out), f64(c["W1"]), f64(c["b1"])
    acc = src @ W1.T
    allow = gemm_unit(4 * c["C"]) * (np.abs(src) @ np.abs(W1).T) + U * (np.abs(acc) + np.abs(b1))
    return np.maximum(acc + b1, 0.0), allow, acc + b1


# --------------------------------------------------------------------------------- stem --
def stem_reference(c):
    """(out, allow, pre) [B][F][T][C0]; feats (B, T, F) is the (B, 1, F, T) image."""
    img = t64(c["feats"]).permute(0, 2, 1)[:, None]
    w = t64(c["w"]).reshape(c["C0"], 1, 3, 3)
    bias = f64(c["bias"])
    pre = F.conv2d(img, w, padding=1).permute(0, 2, 3, 1).numpy() + bias
    S = F.conv2d(img.abs(), w.abs(), padding=1).permute(0, 2, 3, 1).numpy()
    return np.maximum(pre, 0.0), (9 + 2) * U * (S + np.abs(bias)), pre


# -------------------------------------------------------------------------------- simam --
def simam_reference(c, e_exp=None):
    """dict(out, allow, e, pre, mean, dmean, var, k, dk) with out [B][rows][C] and the statistics [B][1][C]; e is
    the sigmoid's argument."""
    e_exp = E_EXP if e_exp is None else e_exp
    z, res = f64(c["z"]), f64(c["res"])
    n = z.shape[1]
    mean = z.mean(axis=1, keepdims=True)
    d = z - mean
    var = (d * d).sum(axis=1, keepdims=True) / (n - 1)
    s2 = (z * z).sum(axis=1, keepdims=True)
    acc = (n + 4) * 2.0 ** -53
    dmean = acc * np.abs(z).mean(axis=1, keepdims=True) + U * np.abs(mean)
    dvar = acc * (s2 + n * mean * mean) / (n - 1) + U * var
    k = 1.0 / (4.0 * (var + LAMBDA))
    dk = k * dvar / (var + LAMBDA) + U * k
    dd = dmean + U * np.abs(d)
    e = d * d * k + 0.5
    de = 2 * np.abs(d) * k * dd + d * d * dk + 2 * U * d * d * k + U * e
    g = 1.0 / (1.0 + np.exp(-e))
    dg = g * (1.0 - g) * (de + U + e_exp) + 2 * U * g
    pre = z * g + res
    return dict(out=np.maximum(pre, 0.0), allow=np.abs(z) * dg + U * np.abs(pre), e=e, pre=pre, mean=mean, var=var,
                dmean=dmean, k=k, dk=dk)


# ---------------------------------------------------------------------------------- tfc --
def tfc_reference(c):
    want = np.ascontiguousarray(np.transpose(c["x"], (0, 2, 1, 3)))
    return want.astype(np.float64), np.zeros(want.shape)


# ------------------------------------------------------------------------------ dispatch --
def reference(c, got=None, e_exp=None):
    """[(label, want, allowance)] of a case, in the order the tests carve the kernel's outputs.  `got`: the
    kernel's outputs in that order (the fused tail's next conv1 is referred to the kernel's own `out`)."""
    op = c["op_name"]
    if op == "conv3x3":
        return [("out",) + conv3x3_reference(c)[:2]]
    if op == "tail":
        r = tail_reference(c)
        refs = [("out", r["out"], r["allow"])]
        if c["fuse1"]:
            refs.append(("y1n",) + next_conv1_reference(c, got[0])[:2])
        return refs
    if op == "stem":
        return [("out",) + stem_reference(c)[:2]]
    if op == "simam":
        r = simam_reference(c, e_exp)
        # the kernel's own coefficients [B][2][C] too: a statistic that leaks across utterances shows there first
        return [("out", r["out"], r["allow"]), ("mean", r["mean"][:, 0], r["dmean"][:, 0]), ("k", r["k"][:, 0], r["dk"][:, 0])]
    return [("out",) + tfc_reference(c)]


def ratios(refs, got):
    """{label: (max |err| / allowance, max |err|)} over the outputs of a case (`got` in the order of `refs`);
    every element of every output is compared."""
    out = {}
    assert len(refs) == len(got)
    for (label, want, allow), g in zip(refs, got):
        g = np.asarray(g, np.float64)
        assert g.shape == want.shape, (label, g.shape, want.shape)
        assert np.isfinite(g).all(), label
        err = np.abs(g - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(err == 0.0, 0.0, err / allow)
        out[label] = (float(q.max()), float(err.max()))
    return out


def ratio(refs, got):
    """max |err| / allowance over all outputs of a case, and max |err|."""
    r = ratios(refs, got).values()
    return max(q for q, _ in r), max(e for _, e in r)
