"""The references, allowances and cases of tests/test_gpu_ssl_op.py discriminate (no GPU needed).

Each float64 reference of tests/ssl_op_ref.py is checked against a naive loop at a tiny shape.  The
two attention kernels are emulated in numpy f32 -- bf16 hi / lo splits with three products, 32-key
chunks inside halves of 128 keys, the natural-domain online softmax for pipe = 0 and the log2-domain
lazy maximum with the `> m + 8` rule for pipe = 1 -- and the faithful emulation must stay inside the
allowance on every attention case, while each of eight wrong emulations must exceed it on a named case.  The
same for LayerNorm (two-pass against one-pass E[x^2] - mu^2), and the construction of the staircase
cases is asserted from the float64 scores.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import op_runner  # noqa: E402
import ssl_op_cases as cases  # noqa: E402
import ssl_op_ref as ref  # noqa: E402
from ssl_op_ref import DH, REL_MAX, REL_STRIDE, t64  # noqa: E402

F32 = np.float32
FLT_MAX = F32(np.finfo(np.float32).max)
LOG2E = F32(1.4426950408889634)
E_EXP_CPU = 2 * 2.0 ** -23  # numpy's exp / exp2 stand in for the device's: 2 f32 ulps
ATTN = cases.attention_cases(8)
BY_NAME = {c["name"]: c for c in ATTN}


# ------------------------------------------------------------------------ emulations --
def bf16(x):
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32)
    return ((u + (((u >> 16) & 1) + 0x7FFF)) & 0xFFFF0000).astype(np.uint32).view(F32)


def split(x):
    hi = bf16(x)
    return hi, bf16(x - hi)


def mm3(a, b):
    """hi * hi + hi * lo + lo * hi with f32 accumulation."""
    ah, al = a
    bh, bl = b
    return (al @ bh + ah @ bl + ah @ bh).astype(F32)


# k order of the S^T accumulators (register e of half hh holds key (e & 3) + 8 (e >> 2) + 4 hh)
# against the plain order 16 (e >> 3) + 8 hh + (e & 7) a P fragment would have without it
_E, _HH = np.meshgrid(np.arange(16), np.arange(2), indexing="ij")
ACC_KEY = ((_E & 3) + 8 * (_E >> 2) + 4 * _HH).reshape(-1)
PLAIN_KEY = (16 * (_E >> 3) + 8 * _HH + (_E & 7)).reshape(-1)


def emulate(q, k, v, pipe, table=None, gate=None, fault=None):
    """One (utterance, head) of attn_kernel (pipe 0) / attn_pipe_kernel (pipe 1) in numpy f32.
    Returns (out [T][64], how often `cmax > m + 8` fired after a row's first chunk)."""
    T = q.shape[0]
    sc = F32(0.125) * LOG2E if pipe else F32(0.125)
    qs = split((q * sc).astype(F32))
    tb = None
    if table is not None:
        tb = (table * LOG2E).astype(F32) if pipe else table.astype(F32)
        g = gate.astype(F32)
        if fault == "gate_row":
            g = g[np.minimum(np.arange(T) + 1, T - 1)]
    m, l, o = np.full(T, -FLT_MAX, F32), np.zeros(T, F32), np.zeros((T, DH), F32)
    fires = 0
    i = np.arange(T)[:, None]
    with np.errstate(over="ignore", invalid="ignore"):
        for h0 in range(0, T, 128):  # a staged half (zeros past T); pipe 0 stages two at a time
            kh = np.zeros((128, DH), F32)
            vh = np.zeros((128, DH), F32)
            nk = min(128, T - h0)
            kh[:nk], vh[:nk] = k[h0:h0 + nk], v[h0:h0 + nk]
            ks, vs = split(kh), split(vh)
            for c0 in range(0, nk, 32):
                st = mm3(qs, (ks[0][c0:c0 + 32].T, ks[1][c0:c0 + 32].T))
                j = h0 + c0 + np.arange(32)[None, :]
                if tb is not None:
                    d = (i - j if fault == "sign" else j - i) + REL_MAX
                    d = d % REL_STRIDE if fault == "unclamped" else np.clip(d, 0, 2 * REL_MAX)
                    st = (g[:, None].astype(np.float64) * tb[d] + st).astype(F32)  # one fma
                live = (c0 + np.arange(32) < nk + (1 if fault == "mask" else 0))[None, :]
                st = np.where(live, st, -FLT_MAX)
                cmax = st.max(axis=1)
                if pipe:
                    up = cmax > m + F32(8.0)
                    if h0 + c0 > 0:
                        fires += int(up.sum())
                    mn = np.where(up, cmax, m)
                    corr = np.exp2(m - mn).astype(F32)
                    if fault == "mn_wave":  # every lane of a firing wave takes cmax, rescaled or not
                        pad = np.concatenate([up, np.zeros(-T % 32, bool)]).reshape(-1, 32)
                        mn = np.where(np.repeat(pad.any(axis=1), 32)[:T], cmax, m)
                    m = mn
                    if fault != "skip_rescale":
                        l = l * corr
                        if fault != "l_only":
                            o = o * corr[:, None]
                    p = np.exp2(st - m[:, None]).astype(F32)
                    l = l + p.sum(axis=1, dtype=F32)
                else:
                    mn = np.maximum(m, cmax)
                    corr = np.exp(m - mn).astype(F32)
                    p = np.where(live, np.exp(st - mn[:, None]), 0).astype(F32)
                    m = mn
                    l = l * (F32(1) if fault == "skip_rescale" else corr) + p.sum(axis=1, dtype=F32)
                    if fault not in ("skip_rescale", "l_only"):
                        o = o * corr[:, None]
                if fault == "perm":
                    pp = np.zeros_like(p)
                    pp[:, PLAIN_KEY] = p[:, ACC_KEY]
                    p = pp
                o = o + mm3(split(p), (vs[0][c0:c0 + 32], vs[1][c0:c0 + 32]))
    return (o * (F32(1) / l)[:, None]).astype(F32), fires


def emulate_case(c, pipe, fault=None):
    H, D = c["H"], c["H"] * DH
    out = np.zeros((c["rows"], D), F32)
    fires = 0
    for b in range(c["B"]):
        r0, r1 = int(c["seg"][b]), int(c["seg"][b + 1])
        for h in range(H):
            q, k, v = (c["qkv"][r0:r1, j * D + h * DH:j * D + (h + 1) * DH] for j in range(3))
            tab = gate = None
            if c["table"] is not None:
                tab, gate = c["table"][h], c["gate"][r0:r1, h]
            out[r0:r1, h * DH:(h + 1) * DH], f = emulate(q, k, v, pipe, tab, gate, fault)
            fires += f
    return out, fires


_REF = {}


def attn_ref(c):
    if c["name"] not in _REF:
        _REF[c["name"]] = ref.attn_reference(c)
    return _REF[c["name"]]


def attn_ratio(c, pipe, fault=None):
    want, allow, A = attn_ref(c)
    got, fires = emulate_case(c, pipe, fault)
    assert np.isfinite(got).all() or fault is not None
    err = (t64(got) - want).abs()
    return float(torch.nan_to_num(err / (allow + 2 * E_EXP_CPU * A), nan=float("inf")).max()), fires


# ------------------------------------------------------------------- attention tests --
@pytest.mark.parametrize("pipe", [1, 0])
def test_faithful_emulation_inside_allowance(pipe):
    for c in ATTN:
        ratio, _ = attn_ratio(c, pipe)
        assert ratio <= 1.0, f"{c['name']} pipe {pipe}: |err| / allowance = {ratio:.3f}"


# fault -> (the named case that must expose it, the kernels it applies to)
FAULTS = {
    "skip_rescale": ("stair_rise", (1, 0)),  # the rescale skipped when the maximum rises
    "l_only": ("stair_rise", (1, 0)),        # l rescaled but o not
    "perm": ("selector", (1, 0)),            # keys of P in accumulator order against V in plain order
    "mask": ("len33", (1, 0)),               # the mask off by one in the last partial chunk
    "sign": ("bias257", (1, 0)),             # the bias taken at i - j
    "unclamped": ("bias1000", (1, 0)),       # the table index unclamped beyond +-778
    "gate_row": ("bias33", (1, 0)),          # the gate of row q taken from row q + 1
    # a wrong mn on lanes that do not raise while their wave does: they take cmax as their maximum
    # but keep the l and o of the old one.  (mn = cmax with its own corr = exp2(m - cmax) on every
    # lane is no fault: the online softmax is exact for any sequence of maxima.)
    "mn_wave": ("stair_rise", (1,)),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_wrong_emulation_exceeds_allowance(fault):
    name, pipes = FAULTS[fault]
    for pipe in pipes:
        ratio, _ = attn_ratio(BY_NAME[name], pipe, fault)
        assert ratio > 1.0, f"{fault} on {name} pipe {pipe} stays inside the allowance ({ratio:.3f})"


def test_rescale_faults_show_on_the_biased_staircase_too():
    for fault in ("skip_rescale", "l_only"):
        assert attn_ratio(BY_NAME["stair_brise"], 1, fault)[0] > 1.0


def _scores(c, h=0):
    """float64 scores of head h of a one-utterance case, natural units."""
    D = c["H"] * DH
    qkv = t64(c["qkv"])
    q, k = qkv[:, h * DH:(h + 1) * DH], qkv[:, D + h * DH:D + (h + 1) * DH]
    tab = gate = None
    if c["table"] is not None:
        tab, gate = t64(c["table"])[h, :ref.REL_N], t64(c["gate"])[:, h]
    return ref.attn_scores(q, k, tab, gate)[0].numpy()


def _log2_scores(c, h=0):
    return _scores(c, h) / math.log(2.0)


def _lazy_walk(s):
    """The lazy maximum over 32-key chunks in float64: (raised [chunks][T] after the first chunk,
    the largest weight exponent reached)."""
    T = s.shape[0]
    m = s[:, :32].max(axis=1)
    raised, top = [], 0.0
    for c0 in range(32, T, 32):
        cmax = s[:, c0:c0 + 32].max(axis=1)
        up = cmax > m + 8.0
        raised.append(up)
        m = np.where(up, cmax, m)
        top = max(top, float((s[:, c0:c0 + 32] - m[:, None]).max()))
    return np.array(raised), top


def test_staircase_construction():
    for name in ("stair_rise", "stair_lazy", "stair_lazy2", "stair_fall", "stair_last", "stair_brise"):
        for h in range(BY_NAME[name]["H"]):
            assert np.abs(_scores(BY_NAME[name], h)).max() <= 100.0, name  # natural units
    for name in ("stair_rise", "stair_brise"):
        c = BY_NAME[name]
        s = _log2_scores(c)
        raised, _ = _lazy_walk(s)
        T = s.shape[0]
        mixed = [raised[ch, w:w + 32].any() and not raised[ch, w:w + 32].all()
                 for ch in range(raised.shape[0]) for w in range(0, T, 32)]
        assert any(mixed), f"{name}: no wave takes the branch while some of its lanes keep their m"
        assert emulate_case(c, 1)[1] > 0, name
    for name in ("stair_lazy", "stair_lazy2"):
        c = BY_NAME[name]
        s = _log2_scores(c)
        raised, top = _lazy_walk(s)
        assert not raised.any() and 7.0 < top <= 8.0, f"{name}: raised {int(raised.sum())}, top weight 2^{top:.2f}"
        assert emulate_case(c, 1)[1] == 0
    # lazy2 is at its top from the third chunk on: most keys of a row weigh more than 2^7
    s = _log2_scores(BY_NAME["stair_lazy2"])
    assert ((s - s[:, :32].max(axis=1, keepdims=True)) > 7.0).mean() > 0.6
    s = _log2_scores(BY_NAME["stair_fall"])
    assert (s[:, -1] - s.max(axis=1)).max() < -100.0  # later weights underflow (2^-100 and below)
    s = _scores(BY_NAME["stair_last"])
    assert (s.argmax(axis=1) == s.shape[1] - 1).all() and abs(np.median(s) + 40.0) < 0.5 and s.shape[1] % 32 != 0
    assert emulate_case(BY_NAME["stair_last"], 1)[1] > 0


def test_selector_construction():
    c = BY_NAME["selector"]
    pi = cases.selector_perm()
    T = len(pi)
    assert sorted(pi) == list(range(T)) and T - 1 in pi
    same = (pi // 32 == np.arange(T) // 32) & (pi != np.arange(T))
    assert same.any()  # moved inside a 32-key chunk
    assert ((np.arange(T) < 128) & (pi >= 128)).any() and ((np.arange(T) < 256) & (pi == 256)).any()
    for h in range(c["H"]):
        s = _log2_scores(c, h) * math.log(2.0)
        top = s[np.arange(T), pi]
        s[np.arange(T), pi] = -np.inf
        assert (top - s.max(axis=1)).min() >= 60.0
    want, allow, _ = attn_ref(c)
    v = t64(c["qkv"])[:, 2 * c["H"] * DH:3 * c["H"] * DH]
    assert ((want - v[pi]).abs() <= allow).all()  # the output is v[pi(i)] within the allowance


def test_attention_reference_against_a_naive_loop():
    c = cases.attn_random("tiny", [3, 2], 7, bias=True)
    want = ref.attn_reference(c)[0].numpy()
    H, D = c["H"], c["H"] * DH
    x = c["qkv"].astype(np.float64)
    for b in range(2):
        r0, r1 = c["seg"][b], c["seg"][b + 1]
        for h in range(H):
            for i in range(r0, r1):
                s = []
                for j in range(r0, r1):
                    dot = sum(x[i, h * DH + d] * x[j, D + h * DH + d] for d in range(DH)) / 8.0
                    s.append(dot + float(c["gate"][i, h]) * float(c["table"][h, (j - i) + REL_MAX]))
                p = [math.exp(e - max(s)) for e in s]
                for d in range(DH):
                    o = sum(p[j - r0] * x[j, 2 * D + h * DH + d] for j in range(r0, r1)) / sum(p)
                    assert abs(o - want[i, h * DH + d]) < 1e-12


# ----------------------------------------------------------------- the other kernels --
def test_gate_reference_against_a_naive_loop():
    c = cases.gate_case(3, 2, 3)
    want, allow, args = ref.gate_reference(c)
    x, w = c["x"].astype(np.float64), c["w"].astype(np.float64)
    for r in range(2):
        for h in range(3):
            a = sum(x[r, h * DH + d] * w[d] for d in range(DH)) + w[128]
            b = sum(x[r, h * DH + d] * w[DH + d] for d in range(DH)) + w[129]
            ga, gb = 1 / (1 + math.exp(-a)), 1 / (1 + math.exp(-b))
            assert abs(ga * (gb * w[130 + h] - 1) + 2 - float(want[r, h])) < 1e-12
    # not vacuous: with the arguments scaled to reach |12| the dot products' sum |x| |w| is about 25, so
    # 72 * 2^-24 * 25 = 1.1e-4 is the size of the largest term; the gate itself lies in [1, 2.5]
    assert (allow > 0).all() and float(allow.max()) < 2e-4
    # the pre-sigmoid arguments span [-12, 12]: each dot product of each case reaches |12| and none
    # passes it; the largest case comes near both ends
    for g in cases.GATE_CASES:
        args = ref.gate_reference(g)[2]
        assert float(args.abs().max()) <= 12.0, g["name"]
        assert float(args[0].abs().max()) > 11.99 and float(args[1].abs().max()) > 11.99, g["name"]
    big = ref.gate_reference(cases.GATE_CASES[-1])[2]
    assert float(big.min()) < -10.0 and float(big.max()) > 10.0


def test_walk_batches_change_head_and_length():
    """On the MI355X's 256 CUs (and on the small count the emulations use) blocks of the persistent
    kernel meet a head change and a 33 / 1 length change between consecutive items; no other
    attention case walks at all."""
    for ncu, cs in ((256, cases.attention_cases(256)), (8, ATTN)):
        for c in cs:
            heads, lens = cases.walk_changes(c, ncu)
            if c["name"] in ("walk", "bias_walk"):
                assert heads >= 8 and lens >= 8, f"{c['name']} on {ncu} CUs: {heads} head / {lens} length changes"
                assert set(c["lens"]) == {33, 1}
            elif ncu == 256:
                assert heads == lens == 0, c["name"]


def test_pos_conv_reference_against_a_naive_loop():
    c = cases.pos_case(5, [3, 2], hot=1)
    pre, S, _ = ref.pos_conv_pre(c["x"], c["seg"], c["w"], c["bias"], c["gout"])
    x, w = c["x"].astype(np.float64), c["w"].astype(np.float64)
    for (row, r0, T) in ((0, 0, 3), (2, 0, 3), (4, 3, 2)):
        for g, n in ((0, 0), (7, 13), (15, 47)):
            y = float(c["bias"][g * 64 + n])
            for tap in range(128):
                t = row - r0 + tap - 64
                if 0 <= t < T:  # taps that leave the utterance read zero, not the neighbour
                    y += sum(x[r0 + t, 48 * g + ch] * w[g * 64 + n, ch, tap] for ch in range(48))
            assert abs(y - float(pre[row, g, n])) < 1e-9
    want, allow = ref.pos_conv_reference(c)
    assert float(want[:3].abs().max()) < 3.0 and float((allow[:3] / (S[:3] + 1)).max()) < 1e-3


def wave_sum(x):
    x = x.astype(F32).copy()
    for o in (32, 16, 8, 4, 2, 1):
        x = (x + x[np.arange(64) ^ o]).astype(F32)
    return x[0]


def ln_emulate(c, one_pass=False):
    """layernorm_kernel's rows in numpy f32: lane l owns channels 4 l + 256 i."""
    D, V4 = c["D"], c["D"] // 256
    x = c["x"][:, :D].astype(F32)
    if c["add"] is not None:
        col = np.arange(D)
        x = (x + c["add"][:, (col // c["gin"]) * c["gout"] + col % c["gin"]]).astype(F32)
    out = np.zeros_like(x)
    inv = F32(1.0) / F32(D)
    for r in range(x.shape[0]):
        v = x[r].reshape(V4, 64, 4)
        s = np.zeros(64, F32)
        for i in range(V4):
            s = (s + ((v[i, :, 0] + v[i, :, 1]) + (v[i, :, 2] + v[i, :, 3]))).astype(F32)
        mean = F32(wave_sum(s) * inv)
        if one_pass:
            q = np.zeros(64, F32)
            for i in range(V4):
                for e in range(4):
                    q = (q + v[i, :, e] * v[i, :, e]).astype(F32)
            var = F32(max(F32(wave_sum(q) * inv) - mean * mean, F32(0)))
        else:
            q = np.zeros(64, F32)
            for i in range(V4):
                for e in range(4):
                    d = (v[i, :, e] - mean).astype(F32)
                    q = (d.astype(np.float64) * d + q).astype(F32)
            var = F32(wave_sum(q) * inv)
        rstd = F32(1.0) / np.sqrt(F32(var + F32(c["eps"])))
        out[r] = ((x[r] - mean).astype(F32) * rstd * c["gamma"] + c["beta"]).astype(F32)
    return out


def test_layernorm_emulations():
    exposed = False
    for c in cases.LN_CASES:
        r = ref.ln_reference(c)
        ratio = float(((t64(ln_emulate(c)) - r["out"]).abs() / r["allow"]).max())
        assert ratio <= 1.0, f"{c['name']}: two-pass |err| / allowance = {ratio:.3f}"
        if c["kind"] == "offset":
            bad = float(((t64(ln_emulate(c, one_pass=True)) - r["out"]).abs() / r["allow"]).max())
            assert bad > 1.0, f"{c['name']}: one-pass E[x^2] - mu^2 stays inside the allowance ({bad:.3f})"
            exposed = True
        if c["kind"] == "constant":  # variance 0: the output is beta
            assert float((r["out"] - t64(c["beta"])).abs().max()) < 1e-12
    assert exposed


def test_layernorm_reference_against_a_naive_loop():
    c = cases.LN_CASES[-1]  # segmented [3, 1, 5] -> [4, 1, 4], with add, accumulating
    r = ref.ln_reference(c)
    D = c["D"]
    rows = []
    for m in range(c["M"]):
        x = [float(c["x"][m, d]) + float(c["add"][m, d // 48 * 64 + d % 48]) for d in range(D)]
        mu = sum(x) / D
        var = sum((e - mu) ** 2 for e in x) / D
        rows.append([(x[d] - mu) / math.sqrt(var + 1e-5) * float(c["gamma"][d]) + float(c["beta"][d]) for d in range(D)])
    assert float((t64(np.array(rows)) - r["out"]).abs().max()) < 1e-10
    src = [0, 1, 2, 2, 3, 4, 5, 6, 7]  # [3, 1, 5] -> [4, 1, 4]: the last frame replicated, the tail trimmed
    want = 0.37 * np.array(rows)[src]
    fw = float(np.float32(0.37))
    assert float((t64(fw / 0.37 * want + c["prior"].astype(np.float64)) - r["feat"]).abs().max()) < 1e-10
    assert bool(r["written"].all())


def test_conv0_reference_against_a_naive_loop():
    c = cases.conv0_case(9, [23, 10], segmented=True)
    want, allow = ref.conv0_reference(c)
    assert want.shape == (3 + 1, 512)
    x, w = c["utts"][0].astype(np.float64), c["w"].astype(np.float64)
    for ch in (0, 100, 511):
        y = [sum(w[ch, k] * x[5 * t + k] for k in range(10)) for t in range(3)]
        mu = sum(y) / 3
        var = sum((e - mu) ** 2 for e in y) / 3
        for t in range(3):
            z = (y[t] - mu) / math.sqrt(var + 1e-5) * float(c["gamma"][ch]) + float(c["beta"][ch])
            assert abs(0.5 * z * (1 + math.erf(z / math.sqrt(2))) - float(want[t, ch])) < 1e-12
    # one frame: variance 0, the output is GELU(beta); so is an all-zero utterance's
    b = t64(c["beta"])
    assert float((want[3] - ref.gelu64(b)).abs().max()) < 1e-12
    z = cases.conv0_case(811, [400, 400], kind="zero")
    assert float((ref.conv0_reference(z)[0][:79] - ref.gelu64(t64(z["beta"]))).abs().max()) < 1e-12
    assert float(allow.max()) < 1e-2


def test_case_files_round_trip(tmp_path):
    """Every case serialises with the counts its header promises (the runner checks them again)."""
    cs = [dict(ATTN[0], pipe=1), dict(BY_NAME["bias_ragged"], pipe=0)] + cases.GATE_CASES[:1] + cases.POS_CASES[:1] \
        + cases.LN_CASES[-2:] + cases.CONV0_CASES[-1:] + [dict(c, pipe=1) for c, _ in cases.refused_cases()]
    p = tmp_path / "cases.bin"
    sent = [cases.op_case(c) for c in cs]
    nh = op_runner.LAYOUT["ssl_run"][0]
    op_runner.write_cases(str(p), cases.MAGIC, sent, nh)
    assert p.stat().st_size == 12 + sum(4 + 4 * nh + sum(4 + 4 * np.size(a) for a in arrs) for _, _, arrs in sent)
