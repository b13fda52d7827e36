"""Float64 references and allowances of ECAPA's own kernels (tests/test_gpu_ecapa_op.py on the MI355X,
tests/test_ecapa_op_ref_cpu.py against numpy emulations).  Every function takes a case dict of
tests/ecapa_op_cases.py and returns float64 arrays shaped as the kernel's output; every allowance is a
function of the inputs and the float64 reference only, never of a kernel's output.

u = 2^-24 (one f32 rounding, relative).  GEMM(K) = 2^-16 + (K + 8) u is DESIGN.md section 4's conv-GEMM
bound per unit of S = sum |a||w| (bf16x3 products, f32 accumulation over K).

res2_chain      sp_i = scale_i relu(conv_i(X_i) + b_i) + shift_i, X_0 = spx[0], X_{i+1} = sp_i + spx[i+1],
                per utterance (torch conv1d, dilation = padding = d).  With E_i the bound on X_i's error
                (E_0 = 0; ReLU is 1-Lipschitz):
                  allow_i = |scale_i| conv(E_i, |W_i|) + local_i,   E_{i+1} = allow_i + u |X_{i+1}|
                  local_i = |scale_i| GEMM(3w) conv(|X_i|, |W_i|) + 4u (|pre| + |scale relu(pre)| + |shift|)
astp            e = bias + att W2^T (fused: de = GEMM(128) sum|att||W2| + 2u|e|; unfused: e is an input,
                de = 0), alpha = softmax_t e, mu = sum alpha x, var = sum alpha x^2 - mu^2, m2 = sum alpha x^2.
                A weight reaches the result through exp factors whose arguments sum to e_t - max e and
                each of which is the device's exp2 of a rounded product:
                  r_t = de_t + 3u |e_t - max e| + nfac (4u + e_exp)
                with nfac the factors a weight can pass through (fused: chunks + 2; unfused: frames of
                its wave + 2) and g = (2 nterm + nfac + 8) u the f32 running sums (nterm = frames a lane
                adds: 16 per chunk fused, ceil(T / 4) unfused).  First order:
                  dmu  = sum alpha r |x - mu| + g (sum alpha |x| + |mu|) + 2u |mu|
                  dvar = sum alpha r |(x - mu)^2 - var| + 2 g m2 + 2 |mu| g (sum alpha |x| + |mu|) + 4u (m2 + mu^2)
                sd must lie in [sqrt(max(var - dvar, floor)), sqrt(max(var + dvar, floor))] widened by
                2 f32 ulps: the allowance is the pair of distances from sqrt(max(var, floor)) to the
                interval's ends, not a linearisation through the clamp.
frame_stats     mean and sqrt(var_unbiased + 1e-7).  n = ceil(T / 4) frames per wave.
                scalar: dmean = (n + 4) u mean|x| + u |mean|;  dv = v ((n + 4) u + 3u) + T / (T - 1) dmean^2 + 2u (v + 1e-7)
                vector: dmean = u |mean| + (T + 4) 2^-53 mean|x|;  dv = v (3u + (T + 4) 2^-53) + T / (T - 1) dmean^2 + 2u (v + 1e-7)
                (both square x - mean~ about the f32 mean: sum (x - mean~)^2 = sum (x - mean)^2 + T dmean^2);
                std in the interval [sqrt(max(v - dv, 0) + 1e-7), sqrt(v + dv + 1e-7)] widened by 2 ulps.
small_linear    act(b + in Wt): ((K + 32) u sum|in||w| + u |pre|) slope + 4 ulps (2^-23) of |out| + e_act (tanh,
                sigmoid), slope = the activation's largest slope over the pre-activation's interval.
residual_scale  x + h g: u (|h g| + |out|), either rounding of x + h * g.
gate / seam     relu(A' W^T + b) scale + shift with A' = a gate (k >= gate_k0) or x + g h:
                |scale| (GEMM(K) + u) S + 4u (|pre| + |scale relu(pre)| + |shift|), S = sum |A'||w|;
                seam_out = float32(x + g h) within 1 ulp.

Measured on the MI355X (tests/test_gpu_ecapa_op.py's docstring has the ratios): the device parts
E_EXP (astp, `__expf` / `expf`) and E_ACT (small_linear, `tanhf` / `expf`) ship as measured there.
"""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
ULP = 2.0 ** -23
F32_1E7 = float(np.float32(1e-7))

# Device parts, measured with the term at 0 (test_gpu_ecapa_op.py): no element exceeded the
# allowance without them, so 0 ships for both.
E_EXP = 0.0
E_ACT = 0.0


def gemm_unit(K):
    return 2.0 ** -16 + (K + 8) * U


def t64(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))


def seg_of(c):
    """Row offsets [B + 1] of a case (uniform: multiples of T)."""
    if c.get("seg") is not None:
        return np.asarray(c["seg"], np.int64)
    return np.arange(c["B"] + 1, dtype=np.int64) * c["T"]


def interval(mid2, lo2, hi2):
    """The allowance (down, up) about sqrt(mid2) that spans [sqrt(lo2), sqrt(hi2)] widened by 2 f32 ulps.
    Where a floor clamps mid2 and lo2 alike, `down` is the 2 ulps alone and a kernel that returns
    sqrt(floor) has error 0."""
    mid = np.sqrt(mid2)
    return mid, (mid - np.sqrt(lo2) * (1.0 - 2 * ULP), np.sqrt(hi2) * (1.0 + 2 * ULP) - mid)


# --------------------------------------------------------------------------- res2_chain --
def res2_reference(c):
    """(out, allow) [M][7w], float64."""
    w, d = c["w"], c["dil"]
    seg = seg_of(c)
    x = np.asarray(c["x"], np.float64)[:, :8 * w]
    W = t64(c["W"]).reshape(7, w, w, 3)
    bias, scale, shift = (np.asarray(c[k], np.float64).reshape(7, w) for k in ("bias", "scale", "shift"))
    out = np.zeros((x.shape[0], 7 * w))
    allow = np.zeros_like(out)
    unit = gemm_unit(3 * w)

    def conv(a, wt):  # [n][L][w] -> [n][L][w], every utterance on its own (zero padding)
        return F.conv1d(t64(a).permute(0, 2, 1), wt, dilation=d, padding=d).permute(0, 2, 1).numpy()

    # a uniform batch goes through conv1d as one batch, a ragged one utterance by utterance
    uniform = c.get("seg") is None
    groups = [(0, x.shape[0])] if uniform else [(seg[b], seg[b + 1]) for b in range(len(seg) - 1)]
    for r0, r1 in groups:
        xu = x[r0:r1].reshape(-1, c["T"] if uniform else r1 - r0, 8 * w)
        X, E = xu[:, :, :w], np.zeros(xu.shape[:2] + (w,))
        for i in range(7):
            pre = conv(X, W[i]) + bias[i]
            S = conv(np.abs(X), W[i].abs())
            a = np.maximum(pre, 0.0)
            sp = a * scale[i] + shift[i]
            local = np.abs(scale[i]) * unit * S + 4 * U * (np.abs(pre) + np.abs(a * scale[i]) + np.abs(shift[i]))
            al = np.abs(scale[i]) * conv(E, W[i].abs()) + local
            out[r0:r1, i * w:(i + 1) * w] = sp.reshape(r1 - r0, w)
            allow[r0:r1, i * w:(i + 1) * w] = al.reshape(r1 - r0, w)
            if i < 6:
                X = sp + xu[:, :, (i + 1) * w:(i + 2) * w]
                E = al + U * np.abs(X)
    return out, allow


# ---------------------------------------------------------------------------------- astp --
def astp_logits(c):
    """Fused: (e, de) [rows][C] from att, W2 and the bias.  Unfused: the given logits, de = 0."""
    if c["op_name"] == "astp_pool":
        e = np.asarray(c["e"], np.float64)
        return e, np.zeros_like(e)
    att, w2, b = (np.asarray(c[k], np.float64) for k in ("att", "w2", "bias2"))
    e = att @ w2.T + b
    return e, gemm_unit(128) * (np.abs(att) @ np.abs(w2).T) + 2 * U * np.abs(e)


def astp_counts(c, T):
    """(nfac, nterm) of an utterance of T frames (module docstring)."""
    if c["op_name"] == "astp_fused":
        nch = (T + 31) // 32
        return nch + 2, 16 * nch
    n = (T + 3) // 4
    return n + 2, n


def astp_reference(c, e_exp=None):
    """dict(mean, dmean, var, dvar, sd, sd_down, sd_up, neff) [B][C]: sd = sqrt(max(var, floor)), sd_down /
    sd_up its distances to the interval's ends, neff = 1 / sum alpha^2."""
    e_exp = E_EXP if e_exp is None else e_exp
    C = c["C"]
    seg = seg_of(c)
    e_all, de_all = astp_logits(c)
    x_all = np.asarray(c["x"], np.float64)[:, :C]
    floor = float(np.float32(c["var_floor"]))
    B = len(seg) - 1
    r = {k: np.zeros((B, C)) for k in ("mean", "dmean", "var", "dvar", "sd", "sd_down", "sd_up", "neff")}
    for b in range(B):
        e, de, x = (a[seg[b]:seg[b + 1]] for a in (e_all, de_all, x_all))
        T = e.shape[0]
        nfac, nterm = astp_counts(c, T)
        mx = e.max(axis=0)
        p = np.exp(e - mx)
        al = p / p.sum(axis=0)
        mu = (al * x).sum(axis=0)
        m2 = (al * x * x).sum(axis=0)
        var = (al * (x - mu) ** 2).sum(axis=0)  # = m2 - mu^2 without the cancellation
        rel = de + 3 * U * np.abs(e - mx) + nfac * (4 * U + e_exp)
        g = (2 * nterm + nfac + 8) * U
        ax = (al * np.abs(x)).sum(axis=0)
        dmu = (al * rel * np.abs(x - mu)).sum(axis=0) + g * (ax + np.abs(mu)) + 2 * U * np.abs(mu)
        dvar = ((al * rel * np.abs((x - mu) ** 2 - var)).sum(axis=0) + 2 * g * m2 + 2 * np.abs(mu) * g * (ax + np.abs(mu))
                + 4 * U * (m2 + mu * mu))
        sd, (down, up) = interval(np.maximum(var, floor), np.maximum(var - dvar, floor), np.maximum(var + dvar, floor))
        neff = 1.0 / (al * al).sum(axis=0)  # frames the softmax effectively averages over
        for k, v in (("mean", mu), ("dmean", dmu), ("var", var), ("dvar", dvar), ("sd", sd), ("sd_down", down),
                     ("sd_up", up), ("neff", neff)):
            r[k][b] = v
    return r


# --------------------------------------------------------------------------- frame_stats --
def frame_stats_vector(c):
    """Whether launch_frame_stats takes the vector form (the buffers themselves are 16-B aligned)."""
    return c["C"] % 4 == 0 and c["ldx"] % 4 == 0 and c["ldo"] % 4 == 0


def frame_stats_reference(c):
    """dict(mean, dmean [B][C]) and, with_std, std with its distances std_down / std_up to the interval's ends."""
    C = c["C"]
    seg = seg_of(c)
    x_all = np.asarray(c["x"], np.float64)[:, :C]
    B = len(seg) - 1
    vec = frame_stats_vector(c)
    r = {k: np.zeros((B, C)) for k in ("mean", "dmean", "std", "std_down", "std_up")}
    for b in range(B):
        x = x_all[seg[b]:seg[b + 1]]
        T = x.shape[0]
        n = (T + 3) // 4
        mean = x.mean(axis=0)
        ax = np.abs(x).mean(axis=0)
        dmean = U * np.abs(mean) + ((T + 4) * 2.0 ** -53 * ax if vec else (n + 4) * U * ax)
        r["mean"][b], r["dmean"][b] = mean, dmean
        if c["with_std"]:
            v = ((x - mean) ** 2).sum(axis=0) / (T - 1)
            acc = (T + 4) * 2.0 ** -53 if vec else (n + 4) * U
            dv = v * (acc + 3 * U) + T / (T - 1) * dmean ** 2 + 2 * U * (v + 1e-7) + abs(F32_1E7 - 1e-7)
            r["std"][b], (r["std_down"][b], r["std_up"][b]) = interval(v + 1e-7, np.maximum(v - dv, 0.0) + 1e-7, v + dv + 1e-7)
    return r


# -------------------------------------------------------------------------- small_linear --
def _act(pre, act):
    if act == 1:
        return np.maximum(pre, 0.0)
    if act == 2:
        return np.tanh(pre)
    if act == 3:
        return 1.0 / (1.0 + np.exp(-pre))
    return pre


def _slope(pre, d, act):
    """The activation's largest slope on [pre - d, pre + d]."""
    if act in (0, 1):
        return np.ones_like(pre)
    near = np.maximum(np.abs(pre) - d, 0.0)  # tanh' and sigmoid' fall with |pre|
    if act == 2:
        return 1.0 - np.tanh(near) ** 2
    s = 1.0 / (1.0 + np.exp(-near))
    return s * (1.0 - s)


def small_linear_reference(c, e_act=None):
    """(out, allow) [R][N]."""
    e_act = E_ACT if e_act is None else e_act
    K, act = c["K"], c["act"]
    a = np.asarray(c["in"], np.float64)[:, :K]
    w = np.asarray(c["wt"], np.float64)
    pre = a @ w
    if c["bias"] is not None:
        pre = pre + np.asarray(c["bias"], np.float64)
    d = (K + 32) * U * (np.abs(a) @ np.abs(w)) + U * np.abs(pre)
    out = _act(pre, act)
    return out, d * _slope(pre, d, act) + 4 * ULP * np.abs(out) + (e_act if act >= 2 else 0.0)


# ------------------------------------------------------------------------ residual_scale --
def rows_utterance(c):
    return np.repeat(np.arange(c["B"]), np.diff(seg_of(c)))


def residual_scale_reference(c):
    """(out, allow) [M][C]."""
    h = np.asarray(c["h"], np.float64)
    hg = h * np.asarray(c["g"], np.float64)[rows_utterance(c)]
    out = hg if c["x"] is None else np.asarray(c["x"], np.float64) + hg
    return out, U * (np.abs(hg) + np.abs(out))


# --------------------------------------------------------------------------- gate / seam --
def gemm_operand(c):
    """The A operand the GEMM multiplies, float64 [M][K]: a gate (k >= gate_k0) or x + g h."""
    K, k0 = c["K"], c["gate_k0"]
    a = np.asarray(c["a"], np.float64)[:, :K]
    g = np.asarray(c["gate"], np.float64)[:, :K - k0][rows_utterance(c)]
    if c["op_name"] == "seam":
        return a + g * np.asarray(c["h"], np.float64)[:, :K]
    a = a.copy()
    a[:, k0:] *= g
    return a


def gemm_reference(c):
    """dict(out, allow [M][N]) and, for the seam, sum [M][K] (float64 x + g h)."""
    A = gemm_operand(c)
    w = np.asarray(c["w"], np.float64)
    bias, scale, shift = (np.asarray(c[k], np.float64) for k in ("bias", "scale", "shift"))
    pre = A @ w.T + bias
    S = np.abs(A) @ np.abs(w).T
    a = np.maximum(pre, 0.0)
    allow = np.abs(scale) * (gemm_unit(c["K"]) + U) * S + 4 * U * (np.abs(pre) + np.abs(a * scale) + np.abs(shift))
    return dict(out=a * scale + shift, allow=allow, sum=A)


def ulp_distance(got32, want64):
    """|got - float32(want)| in units of float32(want)'s ulp."""
    want = np.asarray(want64, np.float64).astype(np.float32)
    return np.abs(got32.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


# ------------------------------------------------------------------------------ dispatch --
def reference(c, e_exp=None, e_act=None):
    """[(label, want, allowance)] of a case, in the order the tests carve the kernel's outputs."""
    op = c["op_name"]
    if op == "res2":
        return [("out",) + res2_reference(c)]
    if op in ("astp_fused", "astp_pool"):
        r = astp_reference(c, e_exp)
        return [("mean", r["mean"], r["dmean"]), ("sd", r["sd"], (r["sd_down"], r["sd_up"]))]
    if op == "frame_stats":
        r = frame_stats_reference(c)
        return [("mean", r["mean"], r["dmean"])] + ([("std", r["std"], (r["std_down"], r["std_up"]))] if c["with_std"] else [])
    if op == "small_linear":
        return [("out",) + small_linear_reference(c, e_act)]
    if op == "residual_scale":
        return [("out",) + residual_scale_reference(c)]
    r = gemm_reference(c)
    if op == "gate":
        return [("out", r["out"], r["allow"])]
    s32 = r["sum"].astype(np.float32)
    return [("out", r["out"], r["allow"]), ("sum", s32.astype(np.float64), np.spacing(np.abs(s32)).astype(np.float64))]


def ratios(refs, got):
    """{label: (max |err| / allowance, max |err|)} over the outputs of a case (`got` in the order of `refs`).
    An allowance is an array or, for the square roots, a pair (below, above) of the reference."""
    out = {}
    assert len(refs) == len(got)
    for (label, want, allow), g in zip(refs, got):
        g = np.asarray(g, np.float64)
        assert g.shape == want.shape, (label, g.shape, want.shape)
        assert np.isfinite(g).all(), label
        err = np.abs(g - want)
        if isinstance(allow, tuple):
            allow = np.where(g < want, allow[0], allow[1])
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(err == 0.0, 0.0, err / allow)
        out[label] = (float(q.max()), float(err.max()))
    return out


def ratio(refs, got):
    """max |err| / allowance over all outputs of a case, and max |err|."""
    r = ratios(refs, got).values()
    return max(q for q, _ in r), max(e for _, e in r)


def ceiling(allow):
    """The largest distance an allowance admits."""
    return float(max(a.max() for a in allow)) if isinstance(allow, tuple) else float(allow.max())
