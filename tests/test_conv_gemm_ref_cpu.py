"""CPU checks of the conv-GEMM op test's own parts (tests/conv_gemm_ref.py, conv_gemm_cases.py).

1. The float64 reference (torch conv1d / conv2d) agrees to 1e-12 with a naive loop written
   straight from the kernels.h formula (k = tap * cin + c; 2-D tap j = kf * kw + kt; group g reads
   channels [g * gcin, g * gcin + cin); the sc2d row map) on tiny shapes: 1-D, dilated, strided,
   ragged, grouped, concat, added operand, 2-D and sc2d.
2. The error bound is neither vacuous nor too tight: a numpy emulation of bf16x3 (bf16 hi / lo
   split, three products, float32 accumulation in k order, float32 epilogue) passes it on the
   inputs of GPU groups 1, 2, 3 and 14, and deliberately wrong emulations fail it:
     * a cross term dropped (a_lo * w_hi; in the "A exact" probe of group 14, where a_lo is zero,
       a_hi * w_lo)                                        -- caught by groups 1, 2, 3 and 14
     * the last 32-wide k-tile that holds data skipped     -- caught by groups 1, 2, 3 and 14
     * one tap shifted by a frame                          -- caught by groups 1, 2, 3 and 14
     * padding that reads the neighbouring utterance instead of zero
                                                           -- caught by groups 2 and 3 (groups 1
       and 14 are 1x1 GEMMs without padding: the mutation does not change them)
3. The case-file writer and the Python reader of the format agree.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import conv_gemm_cases as cases  # noqa: E402
import conv_gemm_ref as ref  # noqa: E402
from conv_gemm_ref import make_case, rand_a, rand_w  # noqa: E402


# ------------------------------------------------------- 1. naive loop --
def naive_y(c):
    """sum_j sum_c A(...) * W[n][j * cin + c], float64, straight from kernels.h."""
    M, N, cin, taps = c["M"], c["N"], c["cin"], c["taps"]
    w = np.asarray(c["w"], dtype=np.float64).reshape(N, cin, taps)  # W[n][k = j * cin + c] = w[n][c][j]
    a = [None if x is None else np.asarray(x, dtype=np.float64) for x in c["a"]]
    off, cs = c["aoff"], c["cseg"]

    def A(row, ch, seg1_row=None):
        if c["amode"] == 1:
            return a[0][row, off[0] + ch] + a[1][row, off[1] + ch]
        s = max(i for i in range(3) if cs[i] <= ch)
        if seg1_row is not None and s == 1:
            row = seg1_row
        return a[s][row, off[s] + ch - cs[s]]

    y = np.zeros((M, N))
    G = N // c["gcols"] if c["gcols"] else 1
    cols = N // G
    stride = max(c["stride"], 1)
    for m in range(M):
        if c["sc2d"]:
            plane = c["Fo"] * c["To"]
            b, fo, to = m // plane, (m % plane) // c["To"], m % c["To"]
            r1 = (b * c["Fi"] + fo * stride) * c["Ti"] + to * stride
            for ch in range(cin):
                y[m] += A(m, ch, r1) * w[:, ch, 0]
            continue
        if c["conv2d"]:
            plane = c["Fo"] * c["To"]
            b, fo, to = m // plane, (m % plane) // c["To"], m % c["To"]
            for j in range(taps):
                kf, kt = j // c["kw"], j % c["kw"]
                fi, ti = fo * stride + kf - c["pad"], to * stride + kt - c["pad"]
                if 0 <= fi < c["Fi"] and 0 <= ti < c["Ti"]:
                    for ch in range(cin):
                        y[m] += A((b * c["Fi"] + fi) * c["Ti"] + ti, ch) * w[:, ch, j]
            continue
        if c["seg"] is not None:
            seg = c["seg"]
            iseg = seg if c["iseg"] is None else c["iseg"]
            b = max(i for i in range(len(seg) - 1) if seg[i] <= m)
            t, base, length = m - seg[b], iseg[b], iseg[b + 1] - iseg[b]
        else:
            Ti = c["Ti"] if c["Ti"] > 0 else c["T"]
            b, t = divmod(m, c["T"])
            base, length = b * Ti, Ti
        for j in range(taps):
            f = t * stride + j * c["dil"] - c["pad"]
            if 0 <= f < length:
                for g in range(G):
                    for ch in range(cin):
                        x = a[0][base + f, off[0] + g * c["gcin"] + ch] if c["gcols"] else A(base + f, ch)
                        y[m, g * cols:(g + 1) * cols] += x * w[g * cols:(g + 1) * cols, ch, j]
    return y


def _tiny_cases():
    rng = np.random.default_rng(7)
    A, W = (lambda r, ld: rand_a(rng, r, ld)), (lambda *s: rand_w(rng, *s))
    seg = np.array([0, 7, 8, 20], dtype=np.int32)
    out = [
        make_case(name="1x1", a=[A(24, 12)], aoff=[4, 0, 0], w=W(32, 8, 1), M=24, T=8),
        make_case(name="k3 dilated", a=[A(24, 8)], w=W(32, 8, 3), M=24, T=6, dil=2, pad=2),
        make_case(name="k5 pad 1 (asymmetric)", a=[A(24, 4)], w=W(32, 4, 5), M=24, T=12, dil=1, pad=1),
        make_case(name="k3 s2", a=[A(3 * 11, 8)], w=W(32, 8, 3), M=15, T=5, Ti=11, stride=2),
        make_case(name="k2 s2", a=[A(3 * 10, 8)], w=W(32, 8, 2), M=15, T=5, Ti=10, stride=2),
        make_case(name="1x1 Ti > T", a=[A(3 * 9, 8)], w=W(32, 8, 1), M=15, T=5, Ti=9),
        make_case(name="ragged k3", a=[A(20, 8)], w=W(32, 8, 3), M=20, T=12, seg=seg, dil=2, pad=2),
        make_case(name="ragged strided", a=[A(15 + 3 + 25, 8)], w=W(32, 8, 3), M=20, T=12, Ti=25, stride=2, seg=seg,
                  iseg=np.array([0, 15, 18, 43], dtype=np.int32)),
        make_case(name="grouped k4", a=[A(20, 20)], w=W(32, 8, 4), M=20, T=12, seg=seg, pad=2, gcols=16, gcin=8),
        make_case(name="grouped overlapping", a=[A(24, 12)], w=W(32, 8, 3), M=24, T=8, pad=1, gcols=16, gcin=4),
        make_case(name="concat 3", a=[A(24, 4), A(24, 12), A(24, 8)], aoff=[0, 4, 4], cseg=[0, 4, 8, 12],
                  w=W(32, 12, 3), M=24, T=8, pad=1),
        make_case(name="added", a=[A(24, 8), A(24, 12)], aoff=[0, 4, 0], amode=1, w=W(32, 8, 3), M=24, T=8, dil=2,
                  pad=2),
        make_case(name="2-D 3x3 s1", a=[A(2 * 3 * 4, 4)], w=W(32, 4, 3, 3), M=24, T=24, B=2, conv2d=1, Fi=3, Ti=4,
                  Fo=3, To=4, stride=1, kw=3, pad=1),
        make_case(name="2-D 3x3 s2", a=[A(2 * 5 * 6, 4)], w=W(32, 4, 3, 3), M=18, T=18, B=2, conv2d=1, Fi=5, Ti=6,
                  Fo=3, To=3, stride=2, kw=3, pad=1),
        make_case(name="2-D 1x1 s2", a=[A(2 * 5 * 6, 8)], w=W(32, 8, 1, 1), M=18, T=18, B=2, conv2d=1, Fi=5, Ti=6,
                  Fo=3, To=3, stride=2, kw=1, pad=0),
        make_case(name="2-D 1x3", a=[A(2 * 3 * 4, 4)], w=W(32, 4, 1, 3), M=12, T=12, B=2, conv2d=1, Fi=3, Ti=4,
                  Fo=3, To=2, stride=1, kw=3, pad=0),
        make_case(name="sc2d s2", a=[A(18, 4), A(2 * 5 * 6, 8)], cseg=[0, 4, 12, 12], w=W(32, 12, 1), M=18, T=18, B=2,
                  sc2d=1, Fi=5, Ti=6, Fo=3, To=3, stride=2),
        make_case(name="sc2d s1", a=[A(24, 4), A(2 * 3 * 4, 4)], cseg=[0, 4, 8, 8], w=W(32, 8, 1), M=24, T=24, B=2,
                  sc2d=1, Fi=3, Ti=4, Fo=3, To=4, stride=1),
    ]
    return out


@pytest.mark.parametrize("c", _tiny_cases(), ids=lambda c: c["name"])
def test_reference_matches_naive_loop(c):
    assert c["M"] <= 24 and c["N"] == 32 and c["cin"] <= 12
    y, S = ref.conv_y_S(c)
    want = naive_y(c)
    assert np.abs(want).max() > 1e-3
    assert np.abs(y.numpy() - want).max() <= 1e-12
    absolute = ref.with_(c, a=[None if x is None else np.abs(x) for x in c["a"]], w=np.abs(c["w"]))
    if c["amode"] == 1:  # S is taken of the sum the kernel forms before it splits: |a0 + a1| |w|
        o, n = c["aoff"], c["cin"]
        both = c["a"][0][:, o[0]:o[0] + n].astype(np.float64) + c["a"][1][:, o[1]:o[1] + n].astype(np.float64)
        absolute = ref.with_(absolute, amode=0, a=[np.abs(both), None, None], aoff=[0, 0, 0])
    assert np.abs(S.numpy() - naive_y(absolute)).max() <= 1e-12
    assert (S.numpy() >= np.abs(want) - 1e-12).all()


def test_reference_epilogue():
    rng = np.random.default_rng(8)
    B, T, N = 3, 4, 32
    c = make_case(a=[rand_a(rng, B * T, 8)], w=rand_w(rng, N, 8, 1), M=B * T, T=T,
                  bias=rng.uniform(-1, 1, N).astype(np.float32),
                  row_bias=rng.uniform(-1, 1, (B, N)).astype(np.float32),
                  scale=rng.uniform(0.5, 1.5, N).astype(np.float32), shift=rng.uniform(-1, 1, N).astype(np.float32))
    y = naive_y(c)
    pre = y + c["bias"].astype(np.float64) + np.repeat(c["row_bias"].astype(np.float64), T, axis=0)
    from math import erf
    for act, fn in ((ref.ACT_NONE, lambda v: v), (ref.ACT_RELU, lambda v: max(v, 0.0)), (ref.ACT_TANH, np.tanh),
                    (ref.ACT_GELU, lambda v: 0.5 * v * (1.0 + erf(v / np.sqrt(2.0))))):
        want = np.vectorize(fn)(pre) * c["scale"].astype(np.float64) + c["shift"].astype(np.float64)
        got = ref.reference(ref.with_(c, act=act))
        assert np.abs(got["out"].numpy() - want).max() <= 1e-12
    res = rand_a(rng, B * T, N + 4)
    got = ref.reference(ref.with_(c, row_bias=None, res=res, ldres=N + 4))
    want = (y + c["bias"] + res[:, :N].astype(np.float64)) * c["scale"].astype(np.float64) + c["shift"]
    assert np.abs(got["out"].numpy() - want).max() <= 1e-12
    # the f32 kernel's bound has no bf16x3 product term
    b1, b0 = got["bound"], ref.reference(ref.with_(c, row_bias=None, res=res, precision=0))["bound"]
    assert (b0 < b1).all() and (b0 > 0).all()


# --------------------------------------------------- 2. bf16x3 emulation --
def im2col(c, shift_tap=None, leak=False):
    """A[m][k = j * cin + c] of a uniform 1-D single-operand case, float32, from the contract.
    shift_tap: that tap reads one frame later; leak: a tap that leaves its utterance reads the
    neighbouring utterance's row instead of zero (both deliberate errors)."""
    assert c["seg"] is None and not c["conv2d"] and c["amode"] == 0 and c["cseg"][1] == c["cin"]
    M, T, cin, taps = c["M"], c["T"], c["cin"], c["taps"]
    x = np.asarray(c["a"][0])[:, c["aoff"][0]:c["aoff"][0] + cin]
    col = np.zeros((M, taps * cin), dtype=np.float32)
    m = np.arange(M)
    b, t = m // T, m % T
    for j in range(taps):
        f = t + j * c["dil"] - c["pad"] + (1 if j == shift_tap else 0)
        inside = (f >= 0) & (f < T)
        rows = b * T + f
        ok = ((rows >= 0) & (rows < x.shape[0])) if leak else inside
        col[ok, j * cin:(j + 1) * cin] = x[rows[ok]]
    return col


def _split(x):
    hi = ref.to_bf16(x)
    return hi, ref.to_bf16(x - hi)


def emulate(c, col, drop=None, skip_last_tile=False):
    """bf16x3 on the device's number formats: products of bf16 pairs are exact in float32, the
    accumulator is float32 and takes the three terms of each k in turn; float32 epilogue."""
    N, K = c["N"], col.shape[1]
    wk = np.ascontiguousarray(np.asarray(c["w"]).reshape(N, c["cin"], c["taps"]).transpose(0, 2, 1)).reshape(N, K)
    ahi, alo = _split(col)
    whi, wlo = _split(wk)
    acc = np.zeros((col.shape[0], N), dtype=np.float32)
    kend = 32 * ((K - 1) // 32) if skip_last_tile else K
    for k in range(kend):
        if drop != "alo_whi":
            acc += alo[:, k:k + 1] * whi[None, :, k]
        if drop != "ahi_wlo":
            acc += ahi[:, k:k + 1] * wlo[None, :, k]
        acc += ahi[:, k:k + 1] * whi[None, :, k]
    assert acc.dtype == np.float32
    y = acc + (c["bias"] if c["bias"] is not None else np.float32(0))
    if c["act"] == ref.ACT_RELU:
        y = np.maximum(y, np.float32(0))
    else:
        assert c["act"] == ref.ACT_NONE
    if c["scale"] is not None:
        y = y * c["scale"] + c["shift"]
    assert y.dtype == np.float32
    return y


def _emulated_groups():
    out = []
    for gname, fn in (("1", cases.group1), ("2", cases.group2), ("3", cases.group3), ("14", cases.group14)):
        for c in fn():
            out.append(pytest.param(gname, c, id=c["name"]))
    return out


_REF = {}


def _reference(c):  # computed once per case, shared by the tests below
    if c["name"] not in _REF:
        _REF[c["name"]] = ref.reference(c)
    return _REF[c["name"]]


def _ratio(c, y):
    r = _reference(c)
    return float((torch.from_numpy(y).double() - r["out"]).abs().div(r["bound"]).max())


@pytest.mark.parametrize("group,c", _emulated_groups())
def test_bound_holds_for_bf16x3_and_fails_for_wrong_kernels(group, c):
    good = im2col(c)
    ratio = _ratio(c, emulate(c, good))
    assert ratio <= 1.0, f"the faithful emulation misses the bound: {ratio}"
    assert ratio > 1e-3, f"the bound is vacuous: {ratio}"
    drop = "ahi_wlo" if c["name"] == "g14 A exact" else "alo_whi"
    assert _ratio(c, emulate(c, good, drop=drop)) > 1.0, "a dropped cross term passes"
    assert _ratio(c, emulate(c, good, skip_last_tile=True)) > 1.0, "a skipped k-tile passes"
    assert _ratio(c, emulate(c, im2col(c, shift_tap=c["taps"] - 1))) > 1.0, "a shifted tap passes"
    if group in ("2", "3"):
        assert _ratio(c, emulate(c, im2col(c, leak=True))) > 1.0, "a leak across utterances passes"
    else:
        assert c["pad"] == 0 and np.array_equal(im2col(c, leak=True), good)


def test_split_probes_have_one_exact_operand():
    a_exact, w_exact = cases.group14()
    assert np.array_equal(ref.to_bf16(a_exact["a"][0]), a_exact["a"][0])
    assert not np.array_equal(ref.to_bf16(a_exact["w"]), a_exact["w"])
    assert np.array_equal(ref.to_bf16(w_exact["w"]), w_exact["w"])
    assert not np.array_equal(ref.to_bf16(w_exact["a"][0]), w_exact["a"][0])
    assert a_exact["prod_exp"] == w_exact["prod_exp"] == 17


def test_layernorm_fold_cases_are_the_layers_they_fold():
    """Group 12: the folded operands (W gamma, b + W beta, ln_in, ln_cs) describe the plain layer
    LayerNorm(A; gamma, beta) W^T + b, and reference_ln's bound keeps the cancelling terms."""
    for c in cases.group12():
        r = ref.reference_ln(c)
        assert (r["bound"] > 0).all() and torch.isfinite(r["out"]).all()
        if c["lnmode"] != 2:
            continue
        A = ref.operand(c)
        width = A.shape[1]
        ln = torch.nn.functional.layer_norm(A, (width,), torch.from_numpy(c["ln_gamma"]).double(),
                                            torch.from_numpy(c["ln_beta"]).double(), eps=c["ln_eps"])
        plain = ln @ torch.from_numpy(c["ln_w"]).t() + torch.from_numpy(c["ln_b0"]).double()
        plain = ref.act_f64(plain, c["act"])
        # W gamma and b + W beta were rounded to f32 once: 2^-24 relative on each term
        slack = ref.EPS24 * (ln.abs() @ torch.from_numpy(np.abs(c["ln_w"])).t() + plain.abs() + 1.0)
        assert ((plain - r["out"]).abs() <= slack).all()
        # the statistics handed to the kernel are those of A, and rows sit at mean ~ 3 sigma
        parts = c["ln_in"].reshape(c["M"], c["ln_parts"], 2).astype(np.float64)
        assert np.abs(parts[:, :, 0].mean(axis=1) - A.mean(dim=1).numpy()).max() < 1e-6
        ratio = (A.mean(dim=1) / A.std(dim=1)).numpy()
        assert 1.5 < ratio.min() and ratio.max() < 5.0
        cs = np.asarray(c["w"], dtype=np.float64).reshape(c["N"], width).sum(axis=1)
        assert np.abs(cs - c["ln_cs"]).max() <= 2.0 ** -17 * np.abs(c["w"]).sum(axis=1).max()


# ----------------------------------------------------- 3. the case format --
def test_case_file_round_trip(tmp_path):
    group = [cases.group4()[0], cases.group6()[1], cases.group7()[0], cases.group9()[1], cases.group11()[0],
             cases.group13()[0]]
    group = cases.expand(group)
    path = str(tmp_path / "cases.bin")
    ref.write_cases(path, group)
    back = ref.read_cases(path)
    assert len(back) == len(group)
    for c, r in zip(group, back):
        for k in ("variant", "precision", "cin", "taps", "dil", "pad", "M", "T", "N", "ldres", "ldo", "act", "amode",
                  "conv2d", "Fi", "Ti", "Fo", "To", "stride", "kw", "sc2d", "gcols", "gcin", "lnmode", "ln_parts", "B",
                  "colsum"):
            assert r[k] == c[k], (c["name"], k)
        assert [r[f"cseg{i}"] for i in range(4)] == list(c["cseg"])
        assert [r[f"aoff{i}"] for i in range(3)] == list(c["aoff"])
        for i in range(3):
            assert (r["a"][i] is None) == (c["a"][i] is None)
            if c["a"][i] is not None:
                assert np.array_equal(r["a"][i], c["a"][i])
        assert np.array_equal(r["w"], np.asarray(c["w"]).reshape(c["N"], c["cin"], c["taps"]))
        for k in ("bias", "row_bias", "res", "scale", "shift", "seg", "iseg"):
            assert (r[k] is None) == (c[k] is None), (c["name"], k)
            if c[k] is not None:
                assert np.array_equal(r[k], c[k]), (c["name"], k)
    with open(path, "ab") as f:
        f.write(b"\0")
    with pytest.raises(AssertionError):
        ref.read_cases(path)
