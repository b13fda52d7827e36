"""The references, allowances and cases of tests/test_gpu_resnet_op.py discriminate (no GPU needed).

1. A numpy float32 emulation of each kernel's arithmetic -- bf16 hi / lo splits with three products and
   f32 accumulation for conv3x3, the tail's conv2 / conv3 / next conv1 (y2 and `out` split again from their
   f32 values) and the in-tail shortcut; nine f32 FMAs for the stem; f64 moments, f32 mean / var / k and the
   f32 gate for SimAM -- stays inside the allowance on every case.  Its index arithmetic (flat positions,
   k = (kf * 3 + kt) * C + c) is written independently of the float64 reference, which is torch's conv2d.
2. Wrong emulations exceed the allowance on a named case: a halo column that keeps data at a partial tile, a
   halo row read from the neighbouring utterance, kf and kt swapped, two of y2's channels swapped on the way
   into conv3 (what a wrong kAcc order does), the in-tail shortcut read 16 channels off, the residual added
   after the ReLU, SimAM with the divisor n, without the 1e-4 and with f32 moments in the mean-30 regime, the
   stem with T and F exchanged.
3. Conditions on the inputs: in every conv and tail ReLU case at least a quarter of the reference values are
   strictly positive and at least a quarter are cut; SimAM's sigmoid argument spans [0.5, 8] on every case
   with rows >= 63 (with two rows d^2 / var is 1 / 2 whatever the data: the argument is 0.625 there).
4. The case file round-trips through op_runner.write_cases / read_cases.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import op_runner  # noqa: E402
import resnet_op_cases as cases  # noqa: E402
import resnet_op_ref as ref  # noqa: E402

F32 = np.float32
ALL = cases.all_cases()
RUN = [c for c in ALL if c["refuse"] is None]
BY_NAME = {c["name"]: c for c in RUN}


# ------------------------------------------------------------------------------ helpers --
def bf16(x):
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32)
    return ((u + (((u >> 16) & 1) + 0x7FFF)) & 0xFFFF0000).astype(np.uint32).view(F32)


def split(x):
    hi = bf16(x)
    return hi, bf16((x - hi).astype(F32))


def mm3(a, w):
    """a [M][K] times w [N][K] transposed: lo * hi + hi * lo + hi * hi with f32 accumulation."""
    ah, al = split(a)
    wh, wl = (p.T for p in split(w))
    return ((al @ wh + ah @ wl).astype(F32) + ah @ wh).astype(F32)


def fma(a, b, c):
    """One rounding: the product of two f32 is exact in f64."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def patches(x, fault=None):
    """x [B][F][T][C] -> the implicit GEMM's A [B F T][9 C], k = (kf * 3 + kt) * C + c, zeros outside the
    utterance.  Faults: `halo_col` the column t = T keeps column T - 1 where the last time tile is partial;
    `neighbour` a frequency row outside the utterance is read from the neighbouring one."""
    B, Fq, T, C = x.shape
    flat = x.reshape(B * Fq * T, C)
    b, f, t = np.unravel_index(np.arange(B * Fq * T), (B, Fq, T))
    cols = []
    for kf in range(3):
        for kt in range(3):
            ff, tt = f + kf - 1, t + kt - 1
            ok_f, ok_t = (ff >= 0) & (ff < Fq), (tt >= 0) & (tt < T)
            if fault == "halo_col" and T % 32 != 0:
                tt = np.where(tt == T, T - 1, tt)
                ok_t = tt >= 0
            src = (b * Fq + ff) * T + tt
            ok = ok_f & ok_t
            if fault == "neighbour":
                ok = ok_t & (src >= 0) & (src < B * Fq * T)
            cols.append(np.where(ok[:, None], flat[np.clip(src, 0, B * Fq * T - 1)], F32(0)))
    return np.concatenate(cols, axis=1)


def kmajor(W, fault=None):
    """torch [N][C][3][3] -> [N][9 C] with k = (kf * 3 + kt) * C + c."""
    if fault == "swap_kfkt":
        W = W.transpose(0, 1, 3, 2)
    return np.ascontiguousarray(W.transpose(0, 2, 3, 1)).reshape(W.shape[0], -1)


# -------------------------------------------------------------------------- emulations --
def emulate_conv3x3(c, fault=None):
    y = (mm3(patches(c["x"], fault), kmajor(c["W"], fault)) + c["bias"]).astype(F32)
    res = None if c["res"] is None else c["res"].reshape(y.shape)
    if res is not None and fault != "res_after_relu":
        y = (y + res).astype(F32)
    if c["relu"]:
        y = np.maximum(y, F32(0))
    if res is not None and fault == "res_after_relu":
        y = (y + res).astype(F32)
    if c["scale"] is not None:
        y = ((y * c["scale"]).astype(F32) + c["shift"]).astype(F32)
    return [y.reshape(c["x"].shape)]


def emulate_tail(c, fault=None):
    C, shape = c["C"], c["y1"].shape[:3]
    y2 = np.maximum((mm3(patches(c["y1"], fault), kmajor(c["W2"])) + c["b2"]).astype(F32), F32(0))
    if fault == "swap_y2":  # kPlain puts channel 4 where kAcc has channel 8
        y2[:, [4, 8]] = y2[:, [8, 4]]
    a = y2
    if c["xsc"]:
        xs = c["xs"].reshape(-1, C)
        a = np.concatenate([y2, np.roll(xs, 16, axis=1) if fault == "xsc_offset" else xs], axis=1)
    y = (mm3(a, c["W3"]) + c["b3"]).astype(F32)
    if c["res"] is not None:
        y = (y + c["res"].reshape(y.shape)).astype(F32)
    out = np.maximum(y, F32(0))
    got = [out.reshape(shape + (4 * C,))]
    if c["fuse1"]:
        y1n = np.maximum((mm3(out, c["W1"]) + c["b1"]).astype(F32), F32(0))
        got.append(y1n.reshape(shape + (c["c1n"],)))
    return got


def emulate_stem(c, fault=None):
    B, T, Fq, C0 = c["B"], c["T"], c["F"], c["C0"]
    img = c["feats"].reshape(B, Fq, T) if fault == "swap_tf" else c["feats"].transpose(0, 2, 1)
    x = patches(np.ascontiguousarray(img)[..., None])  # [B F T][9]
    a = np.broadcast_to(c["bias"], (x.shape[0], C0)).astype(F32)
    for q in range(9):
        a = fma(x[:, q:q + 1], c["w"][None, :, q], a)
    return [np.maximum(a, F32(0)).reshape(B, Fq, T, C0)]


def emulate_simam(c, fault=None):
    z, res = c["z"], c["res"]
    n = z.shape[1]
    if fault == "f32_moments":
        s1 = np.cumsum(z, axis=1, dtype=F32)[:, -1:].astype(np.float64)
        s2 = np.cumsum((z * z).astype(F32), axis=1, dtype=F32)[:, -1:].astype(np.float64)
    else:
        z64 = z.astype(np.float64)
        s1, s2 = z64.sum(axis=1, keepdims=True), (z64 * z64).sum(axis=1, keepdims=True)
    mean = s1 / n
    var = np.maximum(s2 - s1 * mean, 0.0) / (n if fault == "divisor_n" else n - 1)
    lam = 0.0 if fault == "no_lambda" else 1e-4
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        k = (1.0 / (4.0 * (var.astype(F32).astype(np.float64) + lam))).astype(F32)
        d = (z - mean.astype(F32)).astype(F32)
        ei = (((d * d).astype(F32) * k).astype(F32) + F32(0.5)).astype(F32)
        g = (F32(1) / (F32(1) + np.exp(-ei).astype(F32)).astype(F32)).astype(F32)
        return [np.maximum(fma(z, g, res), F32(0)), mean.astype(F32)[:, 0], k[:, 0]]


def emulate_tfc(c):
    return [np.ascontiguousarray(c["x"].transpose(0, 2, 1, 3))]


EMULATE = dict(conv3x3=emulate_conv3x3, tail=emulate_tail, stem=emulate_stem, simam=emulate_simam, tfc=emulate_tfc)


def _ratio(c, got):
    return ref.ratio(ref.reference(c, got), got)


# ----------------------------------------------------------------- 1: every case inside --
@pytest.mark.parametrize("name", [c["name"] for c in RUN])
def test_emulation_inside(name):
    c = BY_NAME[name]
    q, err = _ratio(c, EMULATE[c["op_name"]](c))
    print(f"{name}: emulation max |err| / allowance {q:.3f}, max |err| {err:.3e}")
    assert q <= 1.0


# ------------------------------------------------------------- 2: wrong emulations out --
@pytest.mark.parametrize("op,fault,name", [
    ("conv3x3", "halo_col", "conv3x3-c64-v0-f5-t33-b2-relu"),
    ("conv3x3", "halo_col", "conv3x3-c32-v0-f4-t70-b2-scale"),
    ("conv3x3", "neighbour", "conv3x3-c32-v0-f3-t31-b2-res"),
    ("conv3x3", "neighbour", "conv3x3-c128-v3-f9-t65-b2-norelu"),
    ("conv3x3", "swap_kfkt", "conv3x3-c128-v0-f4-t32-b3-scale"),
    ("conv3x3", "res_after_relu", "conv3x3-c64-v0-f9-t65-b2-res"),
    ("tail", "halo_col", "tail-c32-c1-f3-t33"),
    ("tail", "neighbour", "tail-c128-alone-f11-t45"),
    ("tail", "swap_y2", "tail-c64-c1-f3-t33"),
    ("tail", "swap_y2", "tail-c128-alone-f9-t70"),
    ("tail", "xsc_offset", "tail-c32-xsc-f9-t70"),
    ("simam", "divisor_n", "simam-b3-r2-c4-normal"),
    ("simam", "divisor_n", "simam-b3-r129-c64-normal-all"),
    ("simam", "no_lambda", "simam-b3-r129-c64-offset-all"),
    ("simam", "no_lambda", "simam-b3-r129-c64-constant-all"),
    ("simam", "f32_moments", "simam-b40-r200-c64-offset-3chunks"),
    ("stem", "swap_tf", "stem-c32-t37-f24"),
])
def test_wrong_emulation_outside(op, fault, name):
    c = BY_NAME[name]
    refs = ref.reference(c, EMULATE[op](c))  # the next conv1 stays referred to the right kernel's out
    got = EMULATE[op](c, fault=fault)
    worst = 0.0
    for (label, want, allow), g in zip(refs, got):
        err = np.abs(g.astype(np.float64) - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(err == 0.0, 0.0, err / allow)
        worst = max(worst, float(np.nan_to_num(q, nan=np.inf).max()))  # a NaN output is as wrong as can be
    print(f"{op} {fault} on {name}: {worst:.1f}")
    assert worst > 1.0


def test_f32_moments_only_fail_where_they_cancel():
    """On N(0, 1) the f32 moment sums leave `out` inside its allowance and show in the kernel's own mean alone:
    what catches them at the output is the mean-30 regime."""
    c = BY_NAME["simam-b3-r129-c64-normal-all"]
    got = emulate_simam(c, fault="f32_moments")
    per = ref.ratios(ref.reference(c, got), got)
    assert per["out"][0] <= 1.0 and per["mean"][0] > 1.0


# ------------------------------------------------------- 3: conditions on the inputs --
def _fractions(pre):
    return float((pre > 0).mean()), float((pre < 0).mean())


@pytest.mark.parametrize("name", [c["name"] for c in RUN if c["op_name"] in ("conv3x3", "tail", "stem")])
def test_relu_cuts_and_keeps(name):
    c = BY_NAME[name]
    if c["op_name"] == "conv3x3":
        if not c["relu"]:
            return
        pres = [ref.conv3x3_reference(c)[2]]
    elif c["op_name"] == "stem":
        pres = [ref.stem_reference(c)[2]]
    else:
        r = ref.tail_reference(c)
        pres = [r["pre2"], r["pre3"]] + ([ref.next_conv1_reference(c, r["out"])[2]] if c["fuse1"] else [])
    for pre in pres:
        pos, neg = _fractions(pre)
        assert pos >= 0.25 and neg >= 0.25, (name, pos, neg)


@pytest.mark.parametrize("name", [c["name"] for c in RUN if c["op_name"] == "simam"])
def test_simam_argument_spans(name):
    c = BY_NAME[name]
    r = ref.simam_reference(c)
    if c["rows"] == 2:  # d^2 / var = 1 / 2 whatever the data: the 1e-4 can only lower the argument
        assert 0.5 <= r["e"].min() and r["e"].max() <= 0.625 + 1e-12
    else:
        assert r["e"].min() <= 0.51 and r["e"].max() >= 8.0, (name, r["e"].min(), r["e"].max())
    pos, neg = _fractions(r["pre"])
    assert pos >= 0.2 and neg >= 0.25, (name, pos, neg)
    if c["regime"] == "constant":
        cc = cases.constant_channels(c["C"])
        assert (r["var"][:, 0, cc] == 0.0).all() and (r["e"][:, :, cc] == 0.5).all()
    if c["regime"] == "offset":  # the cancellation (2e-5: the outlier at two rows)
        assert (r["var"] / (r["mean"] ** 2)).max() < 2e-5


def test_case_lists():
    names = [c["name"] for c in ALL]
    assert len(set(names)) == len(names)
    assert all(c["B"] >= 2 for c in RUN if c["op_name"] != "simam" or c["rows"] < 200)
    refused = [c["name"] for c in ALL if c["refuse"]]
    assert len(refused) == 2 + 4 + 2 + 1
    conv = [c for c in RUN if c["op_name"] == "conv3x3"]
    assert {(c["C"], c["variant"]) for c in conv} == set(cases.CONV_CONFIGS)
    for C, v in cases.CONV_CONFIGS:
        sub = [c for c in conv if (c["C"], c["variant"]) == (C, v)]
        assert {c["F"] for c in sub} == {1, 3, 4, 5, 9} and {c["T"] for c in sub} == {1, 31, 32, 33, 64, 65, 70}
        assert {(c["relu"], c["res"] is not None, c["scale"] is not None) for c in sub} == \
            {(1, False, False), (1, True, False), (0, False, False), (1, False, True)}
        assert {c["gv"] for c in sub} == {4, 5, 7}
    tail = [c for c in RUN if c["op_name"] == "tail"]
    assert {(c["C"], c["form"]) for c in tail} == {(32, "alone"), (32, "c1"), (32, "c2"), (32, "xsc"), (64, "alone"),
                                                   (64, "c1"), (64, "c2"), (128, "alone"), (128, "c1")}
    for c in tail:
        assert c["both"] == int(c["form"] in ("c1", "c2"))
    sim = [c for c in RUN if c["op_name"] == "simam"]
    assert {(c["C"], c["rows"]) for c in sim if c["B"] == 3} >= {(C, r) for C in cases.SIMAM_C for r in cases.SIMAM_ROWS}
    assert {c["regime"] for c in sim} == set(cases.SIMAM_REGIMES)
    assert max(c["B"] * c["F"] * c["T"] for c in conv + tail) <= 5000


# ------------------------------------------------------------------- 4: the case file --
def test_case_file_round_trip(tmp_path):
    nh = op_runner.LAYOUT["resnet_run"][0]
    path = str(tmp_path / "cases.bin")
    op_runner.write_cases(path, cases.MAGIC, [cases.op_case(c) for c in ALL], nh)
    back = op_runner.read_cases(path, cases.MAGIC, nh, cases.narrays)
    assert len(back) == len(ALL)
    for c, (op, hdr, arrays) in zip(ALL, back):
        assert op == c["op"] and hdr == [int(v) for v in c["hdr"]] + [0] * (nh - len(c["hdr"]))
        assert len(arrays) == len(c["arrays"])
        for a, b in zip(c["arrays"], arrays):
            assert np.array_equal(np.ascontiguousarray(a, dtype=F32).reshape(-1).view(np.uint32), b.view(np.uint32))
