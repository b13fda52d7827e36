"""Op-level conformance of the ReDimNet kernels (redimnet.hip) against float64, through
tools/redimnet_oprun, which launches the shipped launchers and holds no reference arithmetic.  One
runner process serves all tests.  Guard rows and the columns past the payload of a row must come back
bit-untouched; utterances next to the one under test are filled with 100 ("hot"), so a tap or a key
that leaves its utterance shows at once.

Every kernel here is a chain of f32 fmaf on f32 storage: none of them forms a bf16x3 product, so the
bound of tests/conv_gemm_ref.py (imported: EPS24 = 2^-24 = u, its unit) enters only through that
unit; the GEMMs the model runs between these kernels are test_gpu_conv_gemm_op.py's subject.

Rules used below (first order in u, one extra u for the second-order terms):
  chain   y = b + sum_{i<n} w_i x_i as n fmaf from b: |dy| <= (n + 2) u S,  S = |b| + sum |w_i||x_i|,
          plus sum |w_i| dx_i for inputs that carry an error dx of their own.
  gelu    g = gelu_as(a) (common.h: A&S 7.1.26 erf): the rule of tests/ssl_op_ref.py, with its measured
          device part GELU_DEVICE_ERR imported:  dg = 1.13 da + 0.5 |a| 1.5e-7 + U4 |g| + GELU_DEVICE_ERR.
  norm    LayerNorm over D values y (error dy) with `depth` roundings in each of its two sums (stem: 16
          sequential adds + the 1/16; rows: 8 per lane + 6 butterfly levels + the 1/D):
            dmu  = mean(dy) + depth u mean|y|
            dd   = dy + dmu + u |d|                                   d = y - mu
            dvar = 2 mean(|d| dd) + depth u var
            dout = |gamma| rstd dd + |gamma||z| (dvar / (2 (var + eps)) + 4 u) + 2 u |out|

stem      chain n = 9 per channel, then norm (D = 16, depth 17).
entry     x = sum_i sw_i in_i is a chain of n fmaf from 0; out = chain over gw with dx carried.
block2d   a = chain n = 36; g = gelu(a); o = chain n = c with dg carried; out = o + x: + u |out|.
block1d   the same with n = k taps (those inside the utterance) and n = C.
layernorm x' = x + add rounds once (u |x'|), then norm (depth 15).
attention q' = q * scale rounds once; s_ij = chain n = dh from 0 over q'_i k_j:
            ds_ij = (dh + 3) u sum |q'_i||k_j|
          the weight of key j is exp(s_ij - m) with m the running maximum at its step; the later
          rescales multiply numerator and denominator by the same alpha, so only their roundings stay
          (one per step of 8 keys).  With w = softmax(s_i) in float64 and R_i = max_j s_ij - min_j s_ij,
            rho_ij = ds_ij + u R_i + 2 u + E_EXP           (argument, one ulp of exp, the device part)
            dout_id = sum_j w_ij rho_ij (|v_jd| + |out_id|) + (T + T / 8 + 4) u (sum_j w_ij |v_jd| + |out_id|)
newgelu   arg = c (x + 0.044715 x^3) in four roundings: darg = 4 u |arg|; tanh has slope <= 1:
            dt = darg (1 - t^2) + 2 u |t| + E_TANH;  out = 0.5 x (1 + t): dout = 0.5 |x| (dt + 3 u (1 + t)).

E_EXP / E_TANH are the device parts of expf / tanhf: 4 x the largest excess over the allowance without
them, measured on the MI355X against float64 of the same f32 arguments (the tests print the excess).
Both excesses measured 0, so E_EXP = E_TANH = 0 ship.

Measured on an MI355X (these seeds), max |err| / allowance:
stem .057, entry .438, block2d .029, block1d .043, layernorm .117, attention .035 (staircases .065),
newgelu .496.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import op_runner  # noqa: E402
from conv_gemm_ref import EPS24  # noqa: E402
from op_runner import untouched as _untouched  # noqa: E402
from ssl_op_ref import GELU_DEVICE_ERR, U4  # noqa: E402

pytestmark = pytest.mark.gpu

MAGIC = 0x44505357
NH, OWN, NARRAYS = 8, 0, 1  # tools/redimnet_oprun.cpp's Layout
STEM, ENTRY, B2D, B1D, LN, ATTN, NGELU = 1, 2, 3, 4, 5, 6, 7
W = 1152
HOT = np.float32(100.0)
MEASURED_EXP_EXCESS = 0.0   # largest excess over the attention allowance without E_EXP (MI355X)
MEASURED_TANH_EXCESS = 0.0  # the same for the NewGELU allowance without E_TANH
E_EXP, E_TANH = 4.0 * MEASURED_EXP_EXCESS, 4.0 * MEASURED_TANH_EXCESS
LN_EPS = 1e-6
# the six (c, F) views a stage's entry reads and the (stride) it applies; the blocks run at (s c, F / s)
STAGE_IN = [(16, 72, 1), (16, 72, 2), (32, 36, 1), (32, 36, 2), (64, 18, 1), (64, 18, 2)]
TS = (1, 2, 3, 33)


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).double()


def _randn(rng, *shape, amp=1.0):
    return (amp * rng.standard_normal(shape)).astype(np.float32)


def _hot_rows(rng, B, T, ld, width):
    """[B T][ld] rows, random in utterance 1 of 3 (or in the only one), 100 in its neighbours and in
    the pad columns of every row"""
    x = np.full((B, T, ld), HOT, np.float32)
    x[B // 2, :, :width] = _randn(rng, T, width)
    return x.reshape(B * T, ld)


# ------------------------------------------------------------------------------ cases --
def stem_case(seed, B, T, ldo):
    rng = np.random.default_rng(seed)
    x = np.full((B, T, 72), HOT, np.float32)
    x[B // 2] = _randn(rng, T, 72)
    c = dict(op=STEM, hdr=[B, T, ldo], B=B, T=T, ldo=ldo, rows=B * T, x=x, w=_randn(rng, 9, 16, amp=1 / 3),
             b=_randn(rng, 16, amp=0.05), g=rng.uniform(0.8, 1.2, 16).astype(np.float32), be=_randn(rng, 16, amp=0.1))
    c["arrays"] = [x, c["w"], c["b"], c["g"], c["be"]]
    return c


def entry_case(seed, rows, n, gw, ld_in=W, ldo=W):
    rng = np.random.default_rng(seed)
    x = np.full((n, rows, ld_in), HOT, np.float32)
    x[:, :, :W] = _randn(rng, n, rows, W)
    sw = torch.softmax(_t(_randn(rng, n, W)), 0).float().numpy()
    c = dict(op=ENTRY, hdr=[rows, n, gw, ld_in, ldo], rows=rows, n=n, gw=gw, ldo=ldo, x=x, sw=sw)
    c["arrays"] = [x, sw]
    if gw:
        c["wt"], c["b"] = _randn(rng, gw, gw, amp=gw ** -0.5), _randn(rng, gw, amp=0.05)
        c["arrays"] += [c["wt"], c["b"]]
    return c


def block_case(op, seed, B, T, C, taps, width, ldx=None, ldo=None, **kw):
    """2-D (width 1152, taps 36, C = c) or 1-D (width C, taps k) ConvNeXt block"""
    rng = np.random.default_rng(seed)
    ldx, ldo = ldx or width, ldo or width
    c = dict(op=op, B=B, T=T, C=C, taps=taps, width=width, ldx=ldx, ldo=ldo, rows=B * T, x=_hot_rows(rng, B, T, ldx, width),
             wd=_randn(rng, taps, C, amp=(36 if op == B2D else taps) ** -0.5), bd=_randn(rng, C, amp=0.3),
             wp=_randn(rng, C, C, amp=C ** -0.5), bp=_randn(rng, C, amp=0.05), **kw)
    c["hdr"] = [B, T, kw["F"], C, ldx, ldo] if op == B2D else [B, T, C, taps, ldx, ldo]
    c["arrays"] = [c["x"], c["wd"], c["bd"], c["wp"], c["bp"]]
    return c


def ln_case(seed, M, D, add, ldx=None, ldo=None):
    rng = np.random.default_rng(seed)
    ldx, ldo = ldx or D, ldo or D
    x = np.full((M, ldx), HOT, np.float32)
    x[:, :D] = _randn(rng, M, D) * rng.uniform(0.01, 10.0, (M, 1)).astype(np.float32) + _randn(rng, M, 1)
    c = dict(op=LN, hdr=[M, D, int(add), ldx, ldx, ldo], rows=M, D=D, ldo=ldo, x=x, add=None,
             g=rng.uniform(0.8, 1.2, D).astype(np.float32), be=_randn(rng, D, amp=0.1))
    if add:
        c["add"] = np.full((M, ldx), HOT, np.float32)
        c["add"][:, :D] = _randn(rng, M, D)
    c["arrays"] = [x] + ([c["add"]] if add else []) + [c["g"], c["be"]]
    return c


def attn_case(seed, T, dh, kind="random", H=4):
    """B = 2: utterance 0 under test, utterance 1 with q, k random and v = 100; pad columns 100"""
    rng = np.random.default_rng(seed)
    B, D = 2, H * dh
    ld, ldo = 3 * D + 8, D + 4
    q, k, v = (_randn(rng, B, T, H, dh) for _ in range(3))
    if kind != "random":
        # the chunk maxima under control: q = [rate_i / scale, 0, noise], k = [step(j), ., noise], so
        # s_ij = rate_i step(j) + noise, step = the key's 8-key step of the running maximum.  Even
        # queries move by 1.5 natural units per step, odd ones by 0.8; "fall" runs the other way, so
        # the maximum is set in the first step and never moves again
        j = np.arange(T)
        rate = np.where(j % 2 == 0, 1.5, 0.8).astype(np.float32) * (1.0 if kind == "rise" else -1.0)
        q *= np.float32(0.3)
        k *= np.float32(0.3)
        q[0, :, :, 0] = (rate * np.float32(math.sqrt(dh)))[:, None]
        k[0, :, :, 0] = (j // 8).astype(np.float32)[:, None]
        v[0] = np.float32(0.1) * v[0] + ((j * 37) % 101 / 50.0 - 1.0).astype(np.float32)[:, None, None]
    v[1] = HOT
    qkv = np.full((B, T, ld), HOT, np.float32)
    for i, t in enumerate((q, k, v)):
        qkv[:, :, i * D:(i + 1) * D] = t.reshape(B, T, D)
    return dict(op=ATTN, hdr=[B, T, H, dh, ld, ldo], B=B, T=T, H=H, dh=dh, ld=ld, ldo=ldo, rows=B * T, kind=kind,
                q=q, k=k, v=v, arrays=[qkv.reshape(B * T, ld)])


def ngelu_case(seed, M, D, ldx):
    rng = np.random.default_rng(seed)
    x = np.full((M, ldx), HOT, np.float32)
    x[:, :D] = _randn(rng, M, D, amp=2.5)
    x[0, :8] = np.array([0.0, -0.0, 1e-30, -1e-30, 12.0, -12.0, 40.0, -40.0], np.float32)
    return dict(op=NGELU, hdr=[M, D, ldx], rows=M, D=D, ldx=ldx, x=x, arrays=[x])


CASES = []
for ti, T in enumerate(TS):
    CASES.append(stem_case(10 + ti, 3, T, W + (8 if T == 3 else 0)))
CASES.append(stem_case(15, 1, 5, W))
for si, (cin, Fin, s) in enumerate(STAGE_IN):  # stage si weights si + 1 inputs
    for ri, rows in enumerate(TS):
        wide = rows == 3
        CASES.append(entry_case(100 + 10 * si + ri, rows, si + 1, s * cin, W + (4 if wide else 0), W + (8 if wide else 0)))
CASES.append(entry_case(170, 33, 7, 0, W + 4, W + 8))  # the backbone's output: the weighted sum alone
CASES.append(entry_case(171, 2, 7, 0))
for ci, (c, Fq) in enumerate(sorted({(s * cin, Fin // s) for cin, Fin, s in STAGE_IN})):
    for ti, T in enumerate(TS):  # T = 33: nine 4-frame tiles, the last with one frame
        wide = T == 3
        CASES.append(block_case(B2D, 200 + 10 * ci + ti, 3, T, c, 36, W, W + (4 if wide else 0), W + (8 if wide else 0), F=Fq))
CASES.append(block_case(B2D, 250, 1, 6, 16, 36, W, F=72))
for ki, k in enumerate((7, 19, 31, 59)):
    for ti, T in enumerate((k // 2, k // 2 + 1, 2 * k)):  # no tap / one tap / every tap reaches past the far end
        C = (96, 144, 288)[(ki + ti) % 3]
        CASES.append(block_case(B1D, 300 + 10 * ki + ti, 3, T, C, k, C, (C + 63) // 64 * 64, (C + 63) // 64 * 64 + 4))
for ti, T in enumerate(TS):
    CASES.append(block_case(B1D, 350 + ti, 3, T, (96, 144, 288, 96)[ti], 59, (96, 144, 288, 96)[ti]))
for di, D in enumerate((96, 144, 288)):
    for mi, M in enumerate(TS):
        CASES.append(ln_case(400 + 10 * di + mi, M, D, add=mi % 2 == 1, ldx=D + (32 if M == 3 else 0), ldo=D + (36 if M == 3 else 0)))
for di, dh in enumerate((24, 36, 72)):
    for ti, T in enumerate((1, 2, 31, 32, 33, 257, 300)):
        CASES.append(attn_case(500 + 10 * di + ti, T, dh))
    CASES.append(attn_case(540 + di, 300, dh, "rise"))
    CASES.append(attn_case(550 + di, 300, dh, "fall"))
for di, D in enumerate((96, 144, 288)):
    CASES.append(ngelu_case(600 + di, 33, D, D + 4 * di))


@pytest.fixture(scope="module")
def res(tmp_path_factory):
    """One runner process for all cases (op_runner.run's table has no entry for this runner)."""
    d = tmp_path_factory.mktemp("redimnet_op")
    fin, fout = os.path.join(str(d), "cases.bin"), os.path.join(str(d), "results.bin")
    op_runner.write_cases(fin, MAGIC, [(c["op"], c["hdr"], c["arrays"]) for c in CASES], NH)
    p = op_runner.launch("redimnet_oprun", fin, fout)
    assert p.returncode == 0, f"runner status {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}"
    out = op_runner.read_results(fout, len(CASES), OWN, NARRAYS)
    return [dict(r, out=r["arrays"][0] if r["status"] == 0 else None) for r in out]


def _of(res, op):
    for c, r in zip(CASES, res):
        if c["op"] == op:
            assert r["status"] == 0, f"case {c['hdr']} refused: {r['message']}"
            yield c, r


def _payload(c, r, width, tag):
    """The rows written, after checking that nothing else was."""
    M, ldo = c["rows"], c["ldo"]
    raw = r["out"].reshape(M + 8, ldo)
    assert _untouched(raw[M:]), f"{tag}: guard rows written"
    assert _untouched(raw[:M, width:]), f"{tag}: guard columns written"
    got = _t(raw[:M, :width])
    assert torch.isfinite(got).all(), tag
    return got


def _check(tag, got, want, allow, rows=None):
    err, allow = (got - want).abs(), allow
    if rows is not None:
        err, allow = err[rows], allow[rows]
    ratio = float((err / allow).max())
    assert ratio <= 1.0, f"{tag}: |err| / allowance = {ratio:.3f}"
    return ratio


def chain(n, S):
    return (n + 2) * EPS24 * S


def gelu64(a):
    return 0.5 * a * (1.0 + torch.erf(a / math.sqrt(2.0)))


def gelu_rule(a, da):
    g = gelu64(a)
    return g, 1.13 * da + 0.5 * a.abs() * 1.5e-7 + U4 * g.abs() + GELU_DEVICE_ERR


def norm_rule(y, dy, gamma, beta, depth):
    """LayerNorm over the last axis, float64, with the `norm` allowance of the docstring."""
    u = EPS24
    mu = y.mean(-1, keepdim=True)
    d = y - mu
    var = (d * d).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + LN_EPS)
    z = d * rstd
    out = z * gamma + beta
    dmu = dy.mean(-1, keepdim=True) + depth * u * y.abs().mean(-1, keepdim=True)
    dd = dy + dmu + u * d.abs()
    dvar = 2.0 * (d.abs() * dd).mean(-1, keepdim=True) + depth * u * var
    dout = gamma.abs() * rstd * dd + gamma.abs() * z.abs() * (dvar / (2.0 * (var + LN_EPS)) + 4 * u) + 2 * u * out.abs()
    return out, dout


# ------------------------------------------------------------------------------ tests --
def test_stem(res):
    worst = 0.0
    for c, r in _of(res, STEM):
        tag = f"stem {c['hdr']}"
        got = _payload(c, r, W, tag)
        B, T = c["B"], c["T"]
        x = _t(c["x"]).transpose(1, 2).unsqueeze(1)              # (B, 1, F, T)
        w = _t(c["w"]).t().reshape(16, 1, 3, 3)                  # [tap][16], tap = kf * 3 + kt
        b = _t(c["b"])
        y = F.conv2d(x, w, b, padding=1)
        S = F.conv2d(x.abs(), w.abs(), b.abs(), padding=1)
        cl = lambda v: v.permute(0, 3, 2, 1)                     # noqa: E731  (B, T, F, 16)
        want, allow = norm_rule(cl(y), chain(9, cl(S)), _t(c["g"]), _t(c["be"]), 17)
        rows = slice((B // 2) * T, (B // 2 + 1) * T)             # the hot utterances' rows are O(100): checked too
        worst = max(worst, _check(tag, got, want.reshape(B * T, W), allow.reshape(B * T, W)))
        assert float(got[rows].abs().max()) < 10.0
    print(f"\nstem: max |err| / allowance {worst:.3f}")
    assert worst > 0.0


def test_stage_entry(res):
    worst = 0.0
    for c, r in _of(res, ENTRY):
        tag = f"entry {c['hdr']}"
        got = _payload(c, r, W, tag)
        n, gw, rows = c["n"], c["gw"], c["rows"]
        xin, sw = _t(c["x"])[:, :, :W], _t(c["sw"])[:, None, :]
        x, Sx = (sw * xin).sum(0), (sw * xin.abs()).sum(0)
        dx = (n + 1) * EPS24 * Sx
        if gw == 0:
            want, allow = x, dx
        else:
            wt, b = _t(c["wt"]), _t(c["b"])
            g = lambda v: v.reshape(rows, W // gw, gw)           # noqa: E731
            want = (g(x) @ wt + b).reshape(rows, W)
            allow = (chain(gw, g(x.abs()) @ wt.abs() + b.abs()) + g(dx) @ wt.abs()).reshape(rows, W)
        worst = max(worst, _check(tag, got, want, allow))
    print(f"\nentry: max |err| / allowance {worst:.3f}")
    assert worst > 0.0


def _block_reference(c):
    """(want, allowance) [rows][width] of a ConvNeXt block case."""
    B, T, C, taps, width = c["B"], c["T"], c["C"], c["taps"], c["width"]
    xr = _t(c["x"])[:, :width]
    wp, bp, bd = _t(c["wp"]), _t(c["bp"]), _t(c["bd"])
    if c["op"] == B2D:
        Fq = c["F"]
        x = xr.reshape(B, T, Fq, C).permute(0, 3, 2, 1)          # (B, c, F, T)
        wd = _t(c["wd"]).reshape(3, 3, 4, C).permute(3, 2, 0, 1)  # [(kf, kt, ci)][co] -> (co, ci, kf, kt)
        conv = lambda v, w, b: F.conv2d(v, w, b, padding=1, groups=C // 4).permute(0, 3, 2, 1).reshape(B * T, Fq, C)  # noqa: E731
        n1 = 36
    else:
        x = xr.reshape(B, T, C).transpose(1, 2)                  # (B, C, T)
        wd = _t(c["wd"]).t().reshape(C, 1, taps)
        conv = lambda v, w, b: F.conv1d(v, w, b, padding=taps // 2, groups=C).transpose(1, 2).reshape(B * T, 1, C)  # noqa: E731
        n1 = taps
    a, Sa = conv(x, wd, bd), conv(x.abs(), wd.abs(), bd.abs())
    g, dg = gelu_rule(a, chain(n1, Sa))
    o = g @ wp + bp
    want = o.reshape(B * T, width) + xr
    allow = (chain(C, g.abs() @ wp.abs() + bp.abs()) + dg @ wp.abs()).reshape(B * T, width) + EPS24 * want.abs()
    return want, allow


def _test_blocks(res, op, name):
    worst = 0.0
    for c, r in _of(res, op):
        tag = f"{name} {c['hdr']}"
        got = _payload(c, r, c["width"], tag)
        want, allow = _block_reference(c)
        B, T = c["B"], c["T"]
        rows = slice((B // 2) * T, (B // 2 + 1) * T)
        worst = max(worst, _check(tag, got, want, allow))
        # the utterance under test is O(1): a tap into a hot neighbour would put O(100 |w|) there
        assert float((got[rows] - want[rows]).abs().max()) < 1e-4, tag
    print(f"\n{name}: max |err| / allowance {worst:.3f}")
    assert worst > 0.0


def test_block2d(res):
    _test_blocks(res, B2D, "block2d")


def test_block1d(res):
    _test_blocks(res, B1D, "block1d")


def test_layernorm(res):
    worst = 0.0
    for c, r in _of(res, LN):
        tag = f"layernorm {c['hdr']}"
        D = c["D"]
        got = _payload(c, r, D, tag)
        y = _t(c["x"])[:, :D]
        dy = torch.zeros_like(y)
        if c["add"] is not None:
            y = y + _t(c["add"])[:, :D]
            dy = EPS24 * y.abs()
        want, allow = norm_rule(y, dy, _t(c["g"]), _t(c["be"]), 15)
        worst = max(worst, _check(tag, got, want, allow))
    print(f"\nlayernorm: max |err| / allowance {worst:.3f}")
    assert worst > 0.0


def _attn_reference(c, e_exp):
    """(want, allowance) [B][T][H][dh]"""
    T, dh, u = c["T"], c["dh"], EPS24
    scale = float(np.float32(1.0) / np.sqrt(np.float32(dh)))
    q, k, v = (_t(t).permute(0, 2, 1, 3) for t in (c["q"], c["k"], c["v"]))  # (B, H, T, dh)
    q = q * scale
    s = q @ k.transpose(-1, -2)
    ds = (dh + 3) * u * (q.abs() @ k.abs().transpose(-1, -2))
    w = torch.softmax(s, -1)
    out = w @ v
    R = s.max(-1, keepdim=True).values - s.min(-1, keepdim=True).values
    rho = w * (ds + u * R + 2 * u + e_exp)
    A = w @ v.abs()
    dout = rho @ v.abs() + rho.sum(-1, keepdim=True) * out.abs() + (T + T / 8 + 4) * u * (A + out.abs())
    return out.permute(0, 2, 1, 3), dout.permute(0, 2, 1, 3)


def _check_attention(res, kinds):
    worst, excess = 0.0, 0.0
    for c, r in _of(res, ATTN):
        if c["kind"] not in kinds:
            continue
        tag = f"attention {c['kind']} {c['hdr']}"
        B, T, H, dh = c["B"], c["T"], c["H"], c["dh"]
        got = _payload(c, r, H * dh, tag).reshape(B, T, H, dh)
        want, allow0 = _attn_reference(c, 0.0)
        _, allow = _attn_reference(c, E_EXP)
        err = (got - want).abs()
        excess = max(excess, float((err - allow0).max()))
        assert float((got[1] - float(HOT)).abs().max()) < 1e-3, tag  # the hot utterance averages 100s
        assert float(got[0].abs().max()) < 10.0, tag
        ratio = float((err / allow).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{tag}: |err| / allowance = {ratio:.3f}"
    print(f"\nattention {sorted(kinds)}: max |err| / allowance {worst:.3f}; excess without E_EXP {max(excess, 0.0):.3e}")
    assert worst > 0.0


def test_attention_lengths(res):
    _check_attention(res, {"random"})


def test_attention_staircases(res):
    """The running maximum rises at every step of 8 keys (rise) or is set in the first one (fall)."""
    for c in CASES:
        if c["op"] == ATTN and c["kind"] != "random":
            s = (_t(c["q"][0]).permute(1, 0, 2) @ _t(c["k"][0]).permute(1, 2, 0)) / math.sqrt(c["dh"])  # (H, T, T)
            step_max = s[:, :, :296].reshape(c["H"], c["T"], 37, 8).max(-1).values
            moves = (step_max[:, :, 1:] > step_max[:, :, :-1].cummax(-1).values).double().mean()
            assert (moves == 1.0) if c["kind"] == "rise" else (moves == 0.0), (c["kind"], float(moves))
    _check_attention(res, {"rise", "fall"})


def test_newgelu(res):
    worst, excess, u = 0.0, 0.0, EPS24
    for c, r in _of(res, NGELU):
        tag = f"newgelu {c['hdr']}"
        M, D, ldx = c["rows"], c["D"], c["ldx"]
        raw = r["out"].reshape(M, ldx)
        assert np.array_equal(raw[:, D:].view(np.uint32), c["x"][:, D:].view(np.uint32)), f"{tag}: pad columns written"
        got, x = _t(raw[:, :D]), _t(c["x"])[:, :D]
        arg = math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)
        t = torch.tanh(arg)
        want = 0.5 * x * (1.0 + t)
        dt0 = 4 * u * arg.abs() * (1.0 - t * t) + 2 * u * t.abs()
        allow0 = 0.5 * x.abs() * (dt0 + 3 * u * (1.0 + t)) + 1e-45
        allow = allow0 + 0.5 * x.abs() * E_TANH
        err = (got - want).abs()
        excess = max(excess, float((err - allow0).max()))
        ratio = float((err / allow).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{tag}: |err| / allowance = {ratio:.3f}"
    print(f"\nnewgelu: max |err| / allowance {worst:.3f}; excess without E_TANH {max(excess, 0.0):.3e}")
    assert worst > 0.0
