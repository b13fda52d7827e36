"""The references, allowances and cases of tests/test_gpu_ecapa_op.py discriminate (no GPU needed).

1. Each float64 reference of tests/ecapa_op_ref.py agrees to 1e-12 with a naive loop written from the
   header comments (res2_chain.h, astp_fused.h, kernels.h) at a tiny shape.
2. A numpy float32 emulation of each kernel's arithmetic order -- bf16 hi / lo splits with three
   products and f32 accumulation for the chain, the logits and the gated GEMMs; the online softmax in
   32-frame chunks with the two half-wave partials merged at the end (fused) or four waves of every
   fourth frame (unfused, both forms); both frame_stats forms; small_linear's 16 waves and its split-K
   slices -- stays inside the allowance on every case of its op (the long-strip case by a
   3-utterance stand-in).
3. Wrong emulations exceed the allowance on a named case.  Two wrong variants that belong on such a
   list cannot be caught as one would first state them, and the tests assert what does hold instead:
   * "the bias omitted" (ASTP): bias2[c] is added to every frame's logit of channel c and the softmax
     runs over frames, so the bias cancels exactly; an emulation without it stays inside the allowance
     (test_astp_bias_cancels).
   * "a halo one row short, caught only at lengths > rout": the chain's windows tile the batch's rows, not
     each utterance, so what shields a row from a short halo is an utterance boundary within the 7d rows
     the seven convs reach (6d of window halo and d of the image's pad rows).  With random weights of gain
     below 1 per step a row 7d away contributes far less than the allowance, so the fault is shown on
     one-sided operands that carry it at full strength: caught on the ragged batch, inside the
     allowance on a batch whose utterances are all at most 7d long (test_res2_short_halo).
4. Outside the named cancellation regimes (ASTP x regimes c and d, frame_stats' offset columns) the largest
   allowance of every case is below 1e-5, the std of the peaked softmaxes included.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ecapa_op_cases as cases  # noqa: E402
import ecapa_op_ref as ref  # noqa: E402

F32 = np.float32
SPECS = [s for s in cases.all_cases(big=False) if s["refuse"] is None]
BY_NAME = {s["name"]: s for s in SPECS}
# the stand-in of the long-strip case: same width, variant, dilation and leading dimensions, 3 utterances
STAND_IN = cases.res2_case(10_000, cases.BIG["w"], cases.BIG["variant"], cases.BIG["dil"], [cases.BIG["T"]] * 3, True,
                           "strips-stand-in", "res2 long strips", ldx=8 * cases.BIG["w"])


def _get(name):
    return cases.materialize(BY_NAME[name])


# ------------------------------------------------------------------------------ helpers --
def bf16(x):
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32)
    return ((u + (((u >> 16) & 1) + 0x7FFF)) & 0xFFFF0000).astype(np.uint32).view(F32)


def split(x):
    hi = bf16(x)
    return hi, bf16((x - hi).astype(F32))


def mm3(a, b, cross=True):
    """lo * hi + hi * lo + hi * hi with f32 accumulation."""
    ah, al = a
    bh, bl = b
    r = al @ bh
    if cross:
        r = r + ah @ bl
    return (r + ah @ bh).astype(F32)


def fma(a, b, c):
    """One rounding: the product of two f32 is exact in f64."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def _seg(c):
    return ref.seg_of(c)


# --------------------------------------------------------------------------- res2_chain --
def emulate_res2(c, fault=None, ranges=None):
    """The chain in f32 on the row ranges [lo, hi) (default: the utterances; rows outside a range read
    zero, as rows outside the utterance do).  A tap is valid inside the range and the utterance."""
    w, d, M = c["w"], c["dil"], c["M"]
    seg = _seg(c)
    utt = np.repeat(np.arange(len(seg) - 1), np.diff(seg))
    x = c["x"][:, :8 * w]
    W = c["W"].reshape(7, w, w, 3)
    bias, scale, shift = (c[k].reshape(7, w) for k in ("bias", "scale", "shift"))
    out = np.zeros((M, 7 * w), F32)
    if ranges is None:
        ranges = [(0, M, 0, M)] if fault == "neighbour" else [(seg[b], seg[b + 1], seg[b], seg[b + 1]) for b in range(len(seg) - 1)]
    for lo, hi, own0, own1 in ranges:  # compute rows [lo, hi), keep rows [own0, own1)
        idx = np.arange(lo, hi)
        X = x[lo:hi, :w].copy()
        for i in range(7):
            cols = []
            for j in range(3):
                src = idx + (j - 1) * d
                ok = (src >= lo) & (src < hi)
                if fault != "neighbour":
                    ok &= utt[np.clip(src, 0, M - 1)] == utt[idx]
                cols.append(np.where(ok[:, None], X[np.clip(src - lo, 0, hi - lo - 1)], F32(0)))
            A = np.concatenate(cols, axis=1)  # k = tap * w + c
            Wk = W[i].transpose(0, 2, 1).reshape(w, 3 * w)
            acc = mm3(split(A), tuple(p.T for p in split(Wk)), cross=fault != "cross")
            pre = (acc + bias[i]).astype(F32)
            if fault == "bn_first":
                y = np.maximum((pre * scale[i]).astype(F32) + shift[i], F32(0)).astype(F32)
            else:
                y = ((np.maximum(pre, F32(0)) * scale[i]).astype(F32) + shift[i]).astype(F32)
            out[own0:own1, i * w:(i + 1) * w] = y[own0 - lo:own1 - lo]
            if i < 6:
                k = i if fault == "addend" else i + 1
                X = (y + x[lo:hi, k * w:(k + 1) * w]).astype(F32)
    return [out]


def res2_windows(c, short=0, short_right=0):
    """The 128-row windows of variants 0 / 2 / 3: a block owns rout = 128 - 12 d rows and computes 6 d rows
    of halo on each side; X_0 is also loaded on the image's pad rows beyond the window, which the first
    conv reads, so the seven convs see 7 d rows to each side (`short` / `short_right` rows fewer)."""
    d, M = c["dil"], c["M"]
    rout = 128 - 12 * d
    return [(max(0, o - 7 * d + short), min(M, min(M, o + rout) + 7 * d - short_right), o, min(M, o + rout))
            for o in range(0, M, rout)]


# ---------------------------------------------------------------------------------- astp --
_R = np.arange(16)
HALF_ROWS = np.stack([(_R & 3) + 8 * (_R >> 2), (_R & 3) + 8 * (_R >> 2) + 4])  # [half][register] -> frame of the chunk


def emulate_astp_fused(c, fault=None):
    C = c["C"]
    seg = _seg(c)
    floor = F32(c["var_floor"])
    w2 = tuple(p.T for p in split(c["w2"]))
    bias = np.zeros(C, F32) if fault == "no_bias" else c["bias2"]
    mean, sd = np.zeros((len(seg) - 1, C), F32), np.zeros((len(seg) - 1, C), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(len(seg) - 1):
            T = int(seg[b + 1] - seg[b])
            att, x = c["att"][seg[b]:seg[b + 1]], c["x"][seg[b]:seg[b + 1], :C]
            m = np.full((2, C), -np.inf, F32)
            s, a1, a2 = (np.zeros((2, C), F32) for _ in range(3))
            for t0 in range(0, T, 32):
                ac = np.zeros((32, 128), F32)
                xc = np.zeros((32, C), F32)
                n = min(32, T - t0)
                ac[:n], xc[:n] = att[t0:t0 + n], x[t0:t0 + n]
                logit = (mm3(split(ac), w2) + bias).astype(F32)
                live = np.arange(32) < n
                dead = F32(0) if fault == "dead0" else F32(-np.inf)
                ev = np.where(live[:, None], logit, dead)[HALF_ROWS]  # [2][16][C]
                xv = xc[HALF_ROWS]
                mc = ev.max(axis=1)
                fire = mc != -np.inf
                m1 = np.maximum(m, mc)
                sc = np.where(fire, np.exp(m - m1), F32(1)).astype(F32)
                if fault != "skip_rescale":
                    s, a1 = (s * sc).astype(F32), (a1 * sc).astype(F32)
                    if fault != "s_only":
                        a2 = (a2 * sc).astype(F32)
                for r in range(16):
                    pe = np.where(fire, np.exp(ev[:, r] - m1), F32(0)).astype(F32)
                    s = (s + pe).astype(F32)
                    a1 = fma(pe, xv[:, r], a1)
                    a2 = fma((pe * xv[:, r]).astype(F32), xv[:, r], a2)
                m = np.where(fire, m1, m)
            Mx = np.maximum(m[0], m[1])
            f = np.where(m == -np.inf, F32(0), np.exp(m - Mx)).astype(F32)
            S = ((s[0] * f[0]).astype(F32) + (s[1] * f[1]).astype(F32)).astype(F32)
            A1 = ((a1[0] * f[0]).astype(F32) + (a1[1] * f[1]).astype(F32)).astype(F32)
            A2 = ((a2[0] * f[0]).astype(F32) + (a2[1] * f[1]).astype(F32)).astype(F32)
            mu = (A1 / S).astype(F32)
            var = ((A2 / S).astype(F32) - (mu * mu).astype(F32)).astype(F32)
            mean[b] = mu
            if fault == "floor_after":
                sd[b] = np.maximum(np.sqrt(np.maximum(var, F32(0))), floor)
            else:
                sd[b] = np.sqrt(np.maximum(var, floor))
    return [mean, sd]


def emulate_astp_pool(c):
    """Four waves of every fourth frame; C % 4 == 0 and aligned operands take the branch-free vector
    form (`__expf` twice per element), the others the branching scalar form."""
    C = c["C"]
    seg = _seg(c)
    floor = F32(c["var_floor"])
    vec = C % 4 == 0 and c["eoff"] == 0
    mean, sd = np.zeros((len(seg) - 1, C), F32), np.zeros((len(seg) - 1, C), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(len(seg) - 1):
            T = int(seg[b + 1] - seg[b])
            e, x = c["e"][seg[b]:seg[b + 1]], c["x"][seg[b]:seg[b + 1]]
            n = (T + 3) // 4
            ep = np.full((4 * n, C), -np.inf, F32)
            xp = np.zeros((4 * n, C), F32)
            ep[:T], xp[:T] = e, x
            mx = np.full((4, C), -np.inf, F32)
            se, a1, a2 = (np.zeros((4, C), F32) for _ in range(3))
            for i in range(n):
                ev, xv = ep[4 * i:4 * i + 4], xp[4 * i:4 * i + 4]
                live = (4 * i + np.arange(4) < T)[:, None]
                if vec:
                    m1 = np.maximum(mx, ev)
                    sc = np.exp(mx - m1).astype(F32)
                    pe = np.exp(ev - m1).astype(F32)
                    px = (pe * xv).astype(F32)
                    n_se, n_a1, n_a2 = fma(se, sc, pe), fma(a1, sc, px), fma(a2, sc, (px * xv).astype(F32))
                else:
                    up = ev > mx
                    sc = np.exp(mx - ev).astype(F32)
                    pe = np.exp(ev - mx).astype(F32)
                    n_se = np.where(up, (se * sc).astype(F32) + F32(1), se + pe).astype(F32)
                    n_a1 = np.where(up, (a1 * sc).astype(F32) + xv, fma(pe, xv, a1)).astype(F32)
                    n_a2 = np.where(up, (a2 * sc).astype(F32) + (xv * xv).astype(F32), fma((pe * xv).astype(F32), xv, a2)).astype(F32)
                    m1 = np.where(up, ev, mx)
                mx, se, a1, a2 = (np.where(live, new, old) for new, old in ((m1, mx), (n_se, se), (n_a1, a1), (n_a2, a2)))
            Mx = mx.max(axis=0)
            f = np.where(mx == -np.inf, F32(0), np.exp(mx - Mx)).astype(F32)
            S, A1, A2 = (np.zeros(C, F32) for _ in range(3))
            for w in range(4):
                S, A1, A2 = ((acc + (v[w] * f[w]).astype(F32)).astype(F32) for acc, v in ((S, se), (A1, a1), (A2, a2)))
            mu = (A1 / S).astype(F32)
            mean[b] = mu
            sd[b] = np.sqrt(np.maximum(((A2 / S).astype(F32) - (mu * mu).astype(F32)).astype(F32), floor))
    return [mean, sd]


# --------------------------------------------------------------------------- frame_stats --
def emulate_frame_stats(c, fault=None, vector=None):
    C = c["C"]
    seg = _seg(c)
    vec = ref.frame_stats_vector(c) if vector is None else vector
    mean, std = np.zeros((len(seg) - 1, C), F32), np.zeros((len(seg) - 1, C), F32)
    for b in range(len(seg) - 1):
        x = c["x"][seg[b]:seg[b + 1], :C]
        T = x.shape[0]
        if vec:
            m = (x.astype(np.float64).sum(axis=0) / T).astype(F32)
            dd = (x - m).astype(F32).astype(np.float64)
            v = ((dd * dd).sum(axis=0) / max(T - 1, 1)).astype(F32)
        else:
            n = (T + 3) // 4
            xp = np.zeros((4 * n, C), F32)
            xp[:T] = x
            live = (np.arange(4 * n) < T).reshape(n, 4, 1)
            xw = xp.reshape(n, 4, C)
            s = np.zeros((4, C), F32)
            for i in range(n):
                s = np.where(live[i], (s + xw[i]).astype(F32), s)
            m = ((((s[0] + s[1]).astype(F32) + s[2]).astype(F32) + s[3]).astype(F32) / F32(T)).astype(F32)
            q = np.zeros((4, C), F32)
            for i in range(n):
                if fault == "one_pass":
                    q = np.where(live[i], fma(xw[i], xw[i], q), q)
                else:
                    dd = (xw[i] - m).astype(F32)
                    q = np.where(live[i], fma(dd, dd, q), q)
            tot = (((q[0] + q[1]).astype(F32) + q[2]).astype(F32) + q[3]).astype(F32)
            if fault == "one_pass":
                tot = (tot - (F32(T) * (m * m).astype(F32)).astype(F32)).astype(F32)
            v = (tot / F32(max(T - 1, 1))).astype(F32)
        mean[b] = m
        std[b] = np.sqrt((np.maximum(v, F32(0)) if fault else v) + F32(1e-7)).astype(F32)
    return [mean, std] if c["with_std"] else [mean]


# -------------------------------------------------------------------------- small_linear --
def _waves16(a, wt, kb, ke):
    """16 waves split [kb, ke) and sum their chains in wave order (both small_linear kernels)."""
    kq = -(-(ke - kb) // 16)
    acc = np.zeros((16,) + (a.shape[0], wt.shape[1]), F32)
    for j in range(kq):  # the 16 waves' chains advance together, one k each
        k = kb + np.arange(16) * kq + j
        ok = k < ke
        kk = np.minimum(k, ke - 1)
        step = fma(a[:, kk].T[:, :, None], wt[kk][:, None, :], acc)
        acc = np.where(ok[:, None, None], step, acc)
    y = np.zeros(acc.shape[1:], F32)
    for w in range(16):
        y = (y + acc[w]).astype(F32)
    return y


def emulate_small_linear(c, fault=None):
    K = c["K"] - (c["K"] % 4 if fault == "tail" else 0)
    a, wt = c["in"][:, :c["K"]], c["wt"]
    if c["scratch"] == 1 and c["K"] >= 4096:
        ks = max(256, (-(-c["K"] // 32) + 63) // 64 * 64)
        y = np.zeros((c["R"], c["N"]), F32)
        for kb in range(0, K, ks):
            y = (y + _waves16(a, wt, kb, min(K, kb + ks))).astype(F32)
    else:
        y = _waves16(a, wt, 0, K)
    if c["bias"] is not None:
        y = (y + c["bias"]).astype(F32)
    if c["act"] == 1:
        y = np.maximum(y, F32(0))
    elif c["act"] == 2:
        y = np.tanh(y).astype(F32)
    elif c["act"] == 3:
        y = (F32(1) / (F32(1) + np.exp(-y).astype(F32))).astype(F32)
    return [y]


# ------------------------------------------------- residual_scale, gated tail and seam --
def emulate_residual_scale(c, fault=None):
    u = ref.rows_utterance(c)
    if fault == "next_gate":  # the last row of an utterance takes the next one's gate
        last = np.asarray(_seg(c)[1:-1]) - 1
        u = u.copy()
        u[last] += 1
    hg = (c["h"] * c["g"][u]).astype(F32)
    return [hg if c["x"] is None else (c["x"] + hg).astype(F32)]


def emulate_gemm(c, fault=None):
    K, k0 = c["K"], c["gate_k0"]
    g = c["gate"][:, :K - k0]
    if fault == "gate_k0":  # the gate read as if it began at column 128
        g = np.roll(g, 128, axis=1)
    g = g[ref.rows_utterance(c)]
    a = c["a"][:, :K].copy()
    outs = []
    if c["op_name"] == "seam":
        a = fma(c["h"][:, :K], g, a)
        outs = [a]
    else:
        a[:, k0:] = (a[:, k0:] * g).astype(F32)
    acc = mm3(split(a), tuple(p.T for p in split(c["w"])))
    y = ((np.maximum((acc + c["bias"]).astype(F32), F32(0)) * c["scale"]).astype(F32) + c["shift"]).astype(F32)
    return [y] + outs


EMULATE = dict(res2=emulate_res2, astp_fused=emulate_astp_fused, astp_pool=emulate_astp_pool, frame_stats=emulate_frame_stats,
               small_linear=emulate_small_linear, residual_scale=emulate_residual_scale, gate=emulate_gemm, seam=emulate_gemm)


# ------------------------------------------------------- 2 and 4: every case of every op --
@pytest.mark.parametrize("name", [s["name"] for s in SPECS] + [STAND_IN["name"]])
def test_emulation_inside_and_allowance_tight(name):
    c = cases.materialize(STAND_IN if name == STAND_IN["name"] else BY_NAME[name])
    refs = ref.reference(c)
    got = EMULATE[c["op_name"]](c)
    if c["op_name"] == "res2" and c["variant"] != 4:  # the windows' 6d halo recomputation is enough for the owned rows
        assert ref.ratio(refs, emulate_res2(c, ranges=res2_windows(c)))[0] <= 1.0
    q, err = ref.ratio(refs, got)
    print(f"{name}: emulation max |err| / allowance {q:.3f}, max |err| {err:.3e}")
    assert q <= 1.0
    if cases.exempt(c):
        return
    for label, _, allow in refs:
        if label == "sum":
            continue  # 1 ulp of the stored sum, not an allowance of this file's making
        if isinstance(allow, tuple):
            allow = np.maximum(*allow)
        a = allow[:, ~cases.offset_columns(c["C"])] if c["op_name"] == "frame_stats" else allow
        assert a.max() < 1e-5, f"{name} {label}: allowance {a.max():.3e} could hide a tenth of the 1e-4 parity bar"


def test_case_lists():
    """The covering sets cover: every regime, form and branch the cases are there for."""
    all_specs = cases.all_cases()
    assert len({s["name"] for s in all_specs}) == len(all_specs)
    refused = [s["name"] for s in all_specs if s["refuse"]]
    assert len(refused) == 5 + 1 + 1 + 2 + 3 + 3
    fused = [cases.materialize(s) for s in SPECS if s["op_name"] == "astp_fused"]
    assert {(c["logits"], c["xreg"]) for c in fused} >= {(a, b) for a in cases.LOGITS for b in ("a", "c")}
    assert {c["xreg"] for c in fused} == set(cases.XREG) and {c["var_floor"] for c in fused} == {1e-7, 1e-5}
    for C in (256, 512, 1536):
        assert {c["T"] for c in fused if c["C"] == C and c["seg"] is None} >= set(cases.ASTP_T)
    pool = [cases.materialize(s) for s in SPECS if s["op_name"] == "astp_pool"]
    for C, eoff in ((260, 0), (1536, 0), (6, 0), (256, 1)):
        sub = [c for c in pool if c["C"] == C and c["eoff"] == eoff]
        assert {c["T"] for c in sub if c["seg"] is None} == set(cases.POOL_T) and any(c["seg"] is not None for c in sub)
        assert {c["logits"] for c in sub} == set(cases.LOGITS) and {c["xreg"] for c in sub} == set(cases.XREG)
    stats = [cases.materialize(s) for s in SPECS if s["op_name"] == "frame_stats"]
    for C, ldx in ((260, 268), (1536, 1544), (6, 14), (260, 266)):
        sub = [c for c in stats if c["C"] == C and c["ldx"] == ldx]
        assert ref.frame_stats_vector(sub[0]) == (ldx % 4 == 0 and C % 4 == 0)
        assert {(c["with_std"], c["std_off"] - C) for c in sub} == {(1, 0), (1, 2), (0, 0)}
        assert {c["T"] for c in sub if c["seg"] is None} == set(cases.STATS_T) | {1}
    sl = [s for s in all_specs if s["op_name"] == "small_linear"]
    assert len(sl) <= 60
    sl = [cases.materialize(s) for s in sl if not s["refuse"]]
    assert {c["R"] for c in sl} == set(cases.SL_R) and {c["K"] for c in sl} == set(cases.SL_K)
    assert {c["N"] for c in sl} == set(cases.SL_N) and {c["act"] for c in sl} == {0, 1, 2, 3}
    assert {c["bias"] is None for c in sl} == {True, False}
    for K in (4096, 4097, 20480):
        assert {c["scratch"] for c in sl if c["K"] == K} == {0, 1}


def test_staircases_fire():
    """The rising staircases raise the running maximum in every chunk, the falling ones only in the first,
    and the single maxima sit where their names say (from the float64 logits)."""
    for T in (97, 225, 64, 96, 128, 224):
        nch = (T + 31) // 32
        for logits in ("rise", "fall", "last", "first") if T % 32 == 1 else ("rise", "fall"):
            c = _get(f"astp_fused-stair-t{T}-{logits}-xa")
            e, _ = ref.astp_logits(c)
            e = e[:T]
            cmax = np.stack([e[t0:t0 + 32].max(axis=0) for t0 in range(0, T, 32)])
            if logits == "rise":
                assert (np.diff(cmax, axis=0) > 8.0).all() and (np.diff(cmax, axis=0) < 16.0).all()
            elif logits == "fall":
                assert (np.diff(cmax, axis=0) < -8.0).all()
            else:
                at = T - 1 if logits == "last" else 0
                assert (e.argmax(axis=0) == at).all() and (e[at] - np.delete(e, at, axis=0).max(axis=0) > 20.0).all()
            assert cmax.shape[0] == nch


# --------------------------------------------------------------- 3: wrong emulations --
def _exceeds(c, got):
    q, _ = ref.ratio(ref.reference(c), got)
    return q


@pytest.mark.parametrize("fault", ["cross", "neighbour", "bn_first", "addend"])
def test_res2_wrong(fault):
    c = _get("res2-w128-v3-d2-ragged")
    q = _exceeds(c, emulate_res2(c, fault=fault))
    print(f"res2 {fault}: {q:.2f}")
    assert q > 1.0


@pytest.mark.parametrize("side", [0, 2])
def test_res2_short_halo(side):
    """Caught on the one-sided cases (ecapa_op_cases.res2_case), which the GPU test runs for every width
    and variant; the same fault on the random weights of the same batch passes, which is why they exist."""
    short = dict(short=1) if side == 0 else dict(short_right=1)
    c = _get(f"res2-w64-v0-d4-ragged-tap{side}")
    q = _exceeds(c, emulate_res2(c, ranges=res2_windows(c, **short)))
    print(f"res2 halo one row short on side {side}, one-sided ragged batch: {q:.2f}")
    assert q > 1.0
    r = _get("res2-w64-v0-d4-ragged")
    assert _exceeds(r, emulate_res2(r, ranges=res2_windows(r, **short))) <= 1.0
    # utterances of at most 7d rows never reach past a halo one row short of 7d
    d = 4
    s = cases.res2_case(10_001, 64, 0, d, [7 * d, 5, 7 * d, 1, 17] * 6, False, "short-utterances", "res2 one-sided w64", side=side)
    c = cases.materialize(s)
    q = _exceeds(c, emulate_res2(c, ranges=res2_windows(c, **short)))
    print(f"res2 halo one row short on side {side}, utterances <= 7d: {q:.3f}")
    assert q <= 1.0


@pytest.mark.parametrize("fault,name", [("skip_rescale", "astp_fused-stair-t96-rise-xa"), ("s_only", "astp_fused-stair-t224-rise-xa"),
                                        ("dead0", "astp_fused-stair-t97-last-xa"), ("floor_after", "astp_fused-c256-t32-uniform-fall-xd")])
def test_astp_wrong(fault, name):
    c = _get(name)
    q = _exceeds(c, emulate_astp_fused(c, fault=fault))
    print(f"astp {fault} on {name}: {q:.2f}")
    assert q > 1.0


def test_astp_bias_cancels():
    """bias2 is constant over the frames the softmax runs over: omitting it changes no weight."""
    for name in ("astp_fused-stair-t97-rise-xa", "astp_fused-c1536-t31-uniform-sd1-xa"):
        c = _get(name)
        assert np.abs(c["bias2"]).max() > 1.0
        q = _exceeds(c, emulate_astp_fused(c, fault="no_bias"))
        print(f"astp without the bias on {name}: {q:.3f}")
        assert q <= 1.0


def test_frame_stats_wrong():
    c = _get("frame_stats-c260-ldx266-t498-ragged-std1-off0")
    refs = ref.reference(c)
    off = cases.offset_columns(c["C"])
    got = emulate_frame_stats(c, fault="one_pass")
    err = np.abs(got[1].astype(np.float64) - refs[1][1]) / np.maximum(*refs[1][2])
    print(f"frame_stats one pass: offset columns {err[:, off].max():.1f}, others {err[:, ~off].max():.2f}")
    assert err[:, off].max() > 1.0
    # both forms are emulated on every scalar case's operands too: the vector arithmetic is the more accurate
    assert ref.ratio(refs, emulate_frame_stats(c, vector=True))[0] <= 1.0


def test_small_linear_wrong():
    c = _get("small_linear-r4-k15-n192-act2-bias")
    assert c["K"] % 4 == 3
    q = _exceeds(c, emulate_small_linear(c, fault="tail"))
    print(f"small_linear without the last K % 4 terms: {q:.1f}")
    assert q > 1.0


def test_residual_scale_wrong():
    c = _get("residual_scale-c512-x-rows130-ragged")
    q = _exceeds(c, emulate_residual_scale(c, fault="next_gate"))
    print(f"residual_scale with the next utterance's gate at a boundary row: {q:.1f}")
    assert q > 1.0


def test_seam_wrong():
    c = _get("seam-b3-t257-n768-k320")
    q = _exceeds(c, emulate_gemm(c, fault="gate_k0"))
    print(f"seam with the gate indexed from 128: {q:.1f}")
    assert q > 1.0


# ------------------------------------------------------ 1: references against naive loops --
def test_res2_reference_naive():
    w, d = 4, 2
    rng = np.random.default_rng(7)
    lens = [1, 5, 9]
    M = sum(lens)
    c = dict(w=w, dil=d, B=3, T=9, seg=np.concatenate([[0], np.cumsum(lens)]), x=rng.standard_normal((M, 8 * w + 4)),
             W=rng.standard_normal((7, w, w, 3)), bias=rng.standard_normal((7, w)), scale=rng.standard_normal((7, w)),
             shift=rng.standard_normal((7, w)))
    out, _ = ref.res2_reference(c)
    want = np.zeros((M, 7 * w))
    r0 = 0
    for L in lens:
        for i in range(7):
            for t in range(L):
                for n in range(w):
                    acc = c["bias"][i, n]
                    for j in range(3):
                        tt = t + (j - 1) * d
                        if 0 <= tt < L:
                            for ch in range(w):
                                xin = c["x"][r0 + tt, i * w + ch] + (want[r0 + tt, (i - 1) * w + ch] if i else 0.0)
                                acc += xin * c["W"][i, n, ch, j]
                    want[r0 + t, i * w + n] = max(acc, 0.0) * c["scale"][i, n] + c["shift"][i, n]
        r0 += L
    assert np.abs(out - want).max() < 1e-12


@pytest.mark.parametrize("op_name", ["astp_fused", "astp_pool"])
def test_astp_reference_naive(op_name):
    rng = np.random.default_rng(8)
    lens, C = [3, 1, 4], 3
    rows = sum(lens)
    c = dict(op_name=op_name, C=C, B=3, T=4, seg=np.concatenate([[0], np.cumsum(lens)]), var_floor=1e-7,
             att=rng.uniform(-1, 1, (rows, 128)), w2=0.2 * rng.standard_normal((C, 128)), bias2=rng.standard_normal(C),
             x=rng.standard_normal((rows, C + 2)), e=rng.standard_normal((rows, C)))
    r = ref.astp_reference(c)
    r0 = 0
    for b, L in enumerate(lens):
        for ch in range(C):
            e = [c["e"][r0 + t, ch] if op_name == "astp_pool" else
                 c["bias2"][ch] + sum(c["att"][r0 + t, k] * c["w2"][ch, k] for k in range(128)) for t in range(L)]
            z = sum(np.exp(v) for v in e)
            mu = sum(np.exp(e[t]) / z * c["x"][r0 + t, ch] for t in range(L))
            m2 = sum(np.exp(e[t]) / z * c["x"][r0 + t, ch] ** 2 for t in range(L))
            assert abs(r["mean"][b, ch] - mu) < 1e-12 and abs(r["var"][b, ch] - (m2 - mu * mu)) < 1e-12
            assert abs(r["sd"][b, ch] - np.sqrt(max(m2 - mu * mu, float(F32(1e-7))))) < 1e-12
            assert r["sd_down"][b, ch] > 0 and r["sd_up"][b, ch] > 0
        r0 += L


def test_frame_stats_reference_naive():
    rng = np.random.default_rng(9)
    lens, C = [2, 5], 3
    c = dict(C=C, B=2, T=5, ldx=C + 1, ldo=12, with_std=1, seg=np.array([0, 2, 7]), x=rng.standard_normal((7, C + 1)))
    r = ref.frame_stats_reference(c)
    r0 = 0
    for b, L in enumerate(lens):
        for ch in range(C):
            m = sum(c["x"][r0 + t, ch] for t in range(L)) / L
            v = sum((c["x"][r0 + t, ch] - m) ** 2 for t in range(L)) / (L - 1)
            assert abs(r["mean"][b, ch] - m) < 1e-12
            assert abs(r["std"][b, ch] - np.sqrt(v + 1e-7)) < 1e-12
            assert 0 < r["std_down"][b, ch] < 1e-6 and 0 < r["std_up"][b, ch] < 1e-6
        r0 += L


def test_small_linear_residual_gemm_reference_naive():
    rng = np.random.default_rng(10)
    for act in range(4):
        c = dict(K=5, act=act, bias=rng.standard_normal(3))
        c["in"], c["wt"] = rng.standard_normal((2, 7)), rng.standard_normal((5, 3))
        out, _ = ref.small_linear_reference(c)
        for r in range(2):
            for n in range(3):
                y = c["bias"][n] + sum(c["in"][r, k] * c["wt"][k, n] for k in range(5))
                y = [y, max(y, 0.0), np.tanh(y), 1.0 / (1.0 + np.exp(-y))][act]
                assert abs(out[r, n] - y) < 1e-12
    seg = np.array([0, 2, 3])
    c = dict(B=2, T=2, seg=seg, x=rng.standard_normal((3, 4)), h=rng.standard_normal((3, 4)), g=rng.uniform(0, 1, (2, 4)))
    out, _ = ref.residual_scale_reference(c)
    for m in range(3):
        for ch in range(4):
            assert abs(out[m, ch] - (c["x"][m, ch] + c["h"][m, ch] * c["g"][0 if m < 2 else 1, ch])) < 1e-12
    for op_name, k0 in (("gate", 2), ("seam", 0)):
        c = dict(op_name=op_name, B=2, T=2, seg=seg, K=4, gate_k0=k0, a=rng.standard_normal((3, 6)), h=rng.standard_normal((3, 5)),
                 gate=rng.uniform(0, 1, (2, 4 - k0 + 1)), w=rng.standard_normal((3, 4)), bias=rng.standard_normal(3),
                 scale=rng.standard_normal(3), shift=rng.standard_normal(3))
        r = ref.gemm_reference(c)
        for m in range(3):
            b = 0 if m < 2 else 1
            for n in range(3):
                acc = c["bias"][n]
                for k in range(4):
                    if op_name == "seam":
                        av = c["a"][m, k] + c["gate"][b, k] * c["h"][m, k]
                    else:
                        av = c["a"][m, k] * (c["gate"][b, k - k0] if k >= k0 else 1.0)
                    acc += av * c["w"][n, k]
                assert abs(r["out"][m, n] - (max(acc, 0.0) * c["scale"][n] + c["shift"][n])) < 1e-12
