"""Op-level conformance of the implicit-GEMM conv kernels against float64.

Each test writes the case file of one operand group (tests/conv_gemm_cases.py), runs
tools/conv_gemm_run ONCE (it launches the shipped dispatchers of libwsp_hip.so and holds no
reference arithmetic) and holds every output element to the bound derived in
tests/conv_gemm_ref.py: |out - ref| <= bound element-wise, guard rows and guard columns
untouched bit for bit, every in-range output finite, and the tile the runner reports equal to the
one the case was written for.  `max(|err| / bound)` per tile is printed (pytest -s).

tanh / GELU are checked in two steps (conv_gemm_ref.act_expected): the act-none twin of the case
against the bound, then the activation output against the float64 activation of the kernel's own
act-none output.  The allowance is A&S 7.1.26's 0.5 |y| 1.5e-7 (GELU) + 4 f32 ulps + DEVICE_ERR,
where DEVICE_ERR is 4 x the largest excess over those documented parts measured on an MI355X over
the inputs of groups 6, 8, 12 and 13 (|y| <= 6.3); it must stay below 1e-6.

Measured (MI355X, the seeds of conv_gemm_cases.py):
  tanh  max |device - float64| 8.2e-8, excess over 4 ulps 0        -> DEVICE_ERR 0
  GELU  max |device - float64| 4.6e-7, excess over A&S + 4 ulps 2.785e-8 (group 13; 2.378e-8 in
        group 12, 0 in groups 6 and 8)                              -> DEVICE_ERR 1.114e-7
  max |err| / bound per group and tile (x3 tiles 128x32, 128x64, 256x64, 128x128, 256x128,
  256x256, 256x256 on 16x16x32 MFMAs = "mf16", family 7 = "g256"; f32 tiles "f128", "f64"):
     1: 128x32 .113  128x64 .148  128x128 .171  256x128 .171  256x256 .115  mf16 .115  g256 .115
        f128 .040  f64 .032
     2: 128x128 .198  256x128 .198  256x256 .198  mf16 .198  g256 .198  f128 .022
     3: 128x64 .032  128x128 .163  256x128 .163  256x256 .044  mf16 .045  g256 .045  f128 .046
        f64 .007
     4: 128x128 .080  256x128 .080  256x256 .080  mf16 .080  g256 .080  f128 .021
     5: 128x64 .062  128x128 .075  256x128 .075  256x256 .075  mf16 .075  f128 .017  f64 .022
     6: 128x128 .407  256x128 .407  256x256 .407  mf16 .463  g256 .463  f128 .390
     7: 128x64 .142  128x128 .250  256x128 .250  256x256 .250  mf16 .250  g256 .250  f128 .059
        f64 .049
     8: 128x32 .363  128x64 .471  256x64 .471  f64 .454
     9: 128x32 .371  128x64 .268  128x128 .314  256x128 .314  256x256 .310  mf16 .310
    10: g256 .110
    11: 128x64 .149  128x128 .231  256x128 .231  256x256 .181  mf16 .182  g256 .182; means .043
    12: g256 .742; ln_out .067 of its tolerance; statistics probes .099
    13: every tile (128x128, 256x128, 256x256, mf16, g256, f128) .755 (the GELU step)
    14: 128x128 .149  256x128 .149  256x256 .149  mf16 .149  g256 .149  f128 .044

Group 12 holds the mean and rstd the kernel merges from ln_in (g_ln_row, shared by modes 2, 4
and 5) to 8 f32 ulps through its statistics probes: W = 0, no bias, ln_g = 1, ln_b = 0 leave
out = (res - mu) rstd, S = 0, and the bound is those 8 ulps plus the f32 epilogue.  In the
other fold cases the same 8 ulps are one term of the bound beside the GEMM terms.  The fold
implements no activation and GELU only: ReLU / tanh used to be dropped silently and are now
refused by the library, which the test asserts, as it does for the f32 kernel given a fold.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import conv_gemm_cases as cases  # noqa: E402
import conv_gemm_ref as ref  # noqa: E402
import op_runner  # noqa: E402
from conv_gemm_ref import ACT_GELU, ACT_NONE, ACT_TANH  # noqa: E402

pytestmark = pytest.mark.gpu

# Largest |device activation - float64 activation of the same f32 input| in excess of the
# documented parts (A&S + 4 ulps), measured over groups 6, 8, 12 and 13 on an MI355X, and the
# allowance chosen from it (4 x, so that other seeds fit; the issue's ceiling is 1e-6).
MEASURED = {ACT_TANH: 0.0, ACT_GELU: 2.785e-8}
DEVICE_ERR = {k: 4.0 * v for k, v in MEASURED.items()}
assert all(v < 1e-6 for v in DEVICE_ERR.values())


def _run(tmp_path, launches, timeout=60):
    return ref.results_of(op_runner.run("conv_gemm_run", ref.MAGIC, ref.op_cases(launches), tmp_path, timeout), launches)


class _Group:
    """One group's launches: every case under its variants, act-none twins of the tanh / GELU
    cases, one reference per base case."""

    def __init__(self, base, variants=cases.X3_VARIANTS, f32=True):
        self.launches, self.twin = [], {}
        self._ys, self._tw = {}, {}
        for c in cases.expand(base, variants, f32):
            if c["act"] in (ACT_TANH, ACT_GELU):
                # cases that differ only in activation and scale / shift share one twin (`twin_key`,
                # set by the group builder); otherwise one twin per base case
                key = (c.get("twin_key", ("base", c["base"])), c["variant"], c["precision"])
                if key not in self._tw:
                    self._tw[key] = len(self.launches)
                    self.launches.append(ref.with_(c, act=ACT_NONE, scale=None, shift=None, name=c["name"] + " twin"))
                self.twin[len(self.launches)] = self._tw[key]
            self.launches.append(c)
        self.ratios = {}
        self.measured = {}
        self.failures = []  # reported after every case has been measured

    def y_S(self, c):
        key = c["base"]
        if key not in self._ys:
            self._ys[key] = ref.conv_y_S(c)
        return self._ys[key]

    def check(self, results, expect_tile=cases.expected_tile):
        for i, (c, r) in enumerate(zip(self.launches, results)):
            tag = f"{c['name']} variant {c['variant']} precision {c['precision']}"
            assert r["status"] == 0, f"{tag}: refused: {r['message']}"
            assert r["tile"] == expect_tile(c), f"{tag}: served by {r['tile']}, written for {expect_tile(c)}"
            M, N = c["M"], c["N"]
            raw = r["out"].view(np.uint32)
            assert (raw[M:] == ref.FILL).all(), f"{tag}: guard rows written"
            assert (raw[:M, N:] == ref.FILL).all(), f"{tag}: guard columns written"
            out = r["out"][:M, :N]
            assert np.isfinite(out).all(), f"{tag}: non-finite output"
            got = torch.from_numpy(np.ascontiguousarray(out)).double()
            if i in self.twin:
                y_none = results[self.twin[i]]["out"][:M, :N]
                want, tol = ref.act_expected(y_none, c, DEVICE_ERR[c["act"]])
                if c["scale"] is None:  # the device activation's own deviation, for the record
                    _, doc = ref.act_expected(y_none, c, 0.0)
                    excess = float(((got - want).abs() - doc).clamp(min=0).max())
                    m = self.measured.setdefault(c["act"], [0.0, 0.0, 0.0])
                    m[0] = max(m[0], excess)
                    m[1] = max(m[1], float((got - want).abs().max()))
                    m[2] = max(m[2], float(np.abs(y_none).max()))
            else:
                rr = ref.reference_ln(c) if c["lnmode"] else ref.reference(c, self.y_S(c))
                want, tol = rr["out"], rr["bound"]
            err = (got - want).abs()
            ratio = float((err / tol).max())
            self.ratios[r["tile"]] = max(self.ratios.get(r["tile"], 0.0), ratio)
            if ratio > 1.0:
                m, n = np.unravel_index(int((err / tol).argmax()), err.shape)
                self.failures.append(f"{tag} tile {r['tile']}: |err| / bound = {ratio:.3f} at row {m} column {n}: "
                                     f"got {float(got[m, n])!r}, want {float(want[m, n])!r}, "
                                     f"bound {float(tol[m, n]):.3e}")
            yield c, r, got

    def report(self, name):
        print(f"\n{name}: max |err| / bound per tile: " + ", ".join(f"{t} {v:.3f}" for t, v in sorted(self.ratios.items())))
        for act, (excess, dev, ymax) in sorted(self.measured.items()):
            print(f"{name}: act {act}: max excess over the documented error {excess:.3e}, max deviation {dev:.3e}, "
                  f"max |y| {ymax:.2f}")
        assert not self.failures, f"{len(self.failures)} case(s) miss the bound:\n" + "\n".join(self.failures[:20])


def _simple(tmp_path, name, base, tiles, variants=cases.X3_VARIANTS, f32=True):
    g = _Group(base, variants, f32)
    results = _run(tmp_path, g.launches)
    for _ in g.check(results):
        pass
    g.report(name)
    assert tiles <= set(g.ratios), f"{name}: tiles never reached: {sorted(tiles - set(g.ratios))}"
    return g, results


ALL_X3 = {"128x32", "128x64", "128x128", "256x128", "256x256", "256x256mf16", "g256"}
WIDE = {"128x128", "256x128", "256x256", "256x256mf16", "g256"}


def test_group01_dense_1x1(tmp_path):
    _simple(tmp_path, "group 1", cases.group1(), ALL_X3 | {"f32_128x128", "f32_128x64"})


def test_group02_dilated(tmp_path):
    _simple(tmp_path, "group 2", cases.group2(), WIDE | {"f32_128x128"})


def test_group03_ktiles_straddle_taps(tmp_path):
    _simple(tmp_path, "group 3", cases.group3(), WIDE | {"128x64", "f32_128x128", "f32_128x64"})


def test_group04_concat(tmp_path):
    _simple(tmp_path, "group 4", cases.group4(), WIDE | {"f32_128x128"})


def test_group05_added_operand(tmp_path):
    g, _ = _simple(tmp_path, "group 5", cases.group5(), (WIDE - {"g256"}) | {"128x64", "f32_128x128", "f32_128x64"})
    assert "g256" not in g.ratios  # family 7 hands the added operand to family 6


def test_group06_strided(tmp_path):
    _simple(tmp_path, "group 6", cases.group6(), {"128x128", "256x128", "256x256", "256x256mf16", "g256",
                                                  "f32_128x128"})


def test_group07_ragged(tmp_path):
    _simple(tmp_path, "group 7", cases.group7(), {"128x64", "128x128", "256x128", "256x256", "256x256mf16", "g256",
                                                  "f32_128x128", "f32_128x64"})


def test_group08_grouped_columns(tmp_path):
    g, results = _simple(tmp_path, "group 8", cases.group8(), {"128x32", "128x64", "256x64", "f32_128x64"})
    for c, r in zip(g.launches, results):
        if c["precision"] and c["gcols"] == 64:
            assert r["tile"] == ("128x64" if c["variant"] in (3, 4) else "256x64")


def test_group09_conv2d(tmp_path):
    _simple(tmp_path, "group 9", cases.group9(), {"128x32", "128x64", "128x128", "256x128", "256x256",
                                                  "256x256mf16"}, variants=(3, 4, 5, 6), f32=False)


def test_group10_conv3_shortcut(tmp_path):
    base = cases.group10()
    g = _Group(base, variants=(7,), f32=False)
    refused = [ref.with_(c, variant=v, precision=1) for c in base for v in (3, 4, 5, 6)]
    refused += [ref.with_(c, variant=0, precision=0) for c in base]
    results = _run(tmp_path, g.launches + refused)
    for _ in g.check(results[:len(g.launches)]):
        pass
    g.report("group 10")
    assert set(g.ratios) == {"g256"}
    for c, r in zip(refused, results[len(g.launches):]):
        assert r["status"] == 1 and r["message"], f"{c['name']} variant {c['variant']} precision {c['precision']} ran"


def test_group11_column_sums(tmp_path):
    g = _Group(cases.group11(), f32=False)
    results = _run(tmp_path, g.launches)
    worst = 0.0
    for c, r, _ in g.check(results):
        B, T, N = c["B"], c["T"], c["N"]
        assert r["block_rows"] == (128 if N % 128 or c["variant"] == 3 else 256)
        rr = ref.reference(c, g.y_S(c))
        mean = rr["out"].reshape(B, T, N).mean(dim=1)
        bound = rr["bound"].reshape(B, T, N).mean(dim=1) + ref.EPS24 * mean.abs()
        got = torch.from_numpy(r["means"].reshape(B, N).copy()).double()
        assert torch.isfinite(got).all()
        ratio = float(((got - mean).abs() / bound).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{c['name']} variant {c['variant']}: column means |err| / bound = {ratio:.3f}"
    g.report("group 11")
    print(f"group 11: column means max |err| / bound {worst:.3f}")
    assert ALL_X3 - {"128x32"} <= set(g.ratios)


def test_group12_layernorm_fold(tmp_path):
    base = cases.group12()
    g = _Group(base, variants=(7,), f32=False)
    refused = [ref.with_(c, variant=6, precision=1) for c in base[:4]]
    refused += [ref.with_(c, variant=0, precision=0) for c in base[:4]]  # the f32 kernel has no fold
    # the fold implements no activation and GELU: anything else must be refused, not ignored
    refused += [ref.with_(c, variant=7, precision=1, act=act) for c in base if c["lnmode"] == 2 and c["act"] == ACT_NONE
                for act in (ref.ACT_RELU, ACT_TANH)]
    results = _run(tmp_path, g.launches + refused)
    worst = 0.0
    for c, r, _ in g.check(results[:len(g.launches)]):
        if c["lnmode"] & 1:  # the emitted (mean, M2) partials against the kernel's own y
            ratio = ref.ln_out_ratio(r["out"][:c["M"], :c["N"]], r["ln_out"])
            worst = max(worst, ratio)
            assert ratio <= 1.0, f"{c['name']}: ln_out |err| / tolerance = {ratio:.3f}"
        else:
            assert r["ln_out"].size == 0
    probes = 0.0  # the statistics probes: out = (res - mu) rstd against the 8-ulp bound
    for c, r in zip(g.launches, results):
        if c.get("stats_probe"):
            rr = ref.reference_ln(c)
            assert float(rr["S"].abs().max()) == 0.0  # nothing but the statistics and the epilogue in the bound
            got = torch.from_numpy(r["out"][:c["M"], :c["N"]].copy()).double()
            probes = max(probes, float(((got - rr["out"]).abs() / rr["bound"]).max()))
    g.report("group 12")
    print(f"group 12: ln_out max |err| / tolerance {worst:.3f}; statistics probes max |err| / bound {probes:.3f}")
    assert 0.0 < probes <= 1.0
    assert set(g.ratios) == {"g256"}
    for c, r in zip(refused, results[len(g.launches):]):
        assert r["status"] == 1 and ("family 7" in r["message"] or "LayerNorm fold" in r["message"]), (
            f"{c['name']} variant {c['variant']} act {c['act']} ran: {r['message']}")


def test_group13_epilogue_matrix(tmp_path):
    g, _ = _simple(tmp_path, "group 13", cases.group13(), {"128x128", "256x128", "256x256", "256x256mf16", "g256",
                                                           "f32_128x128"})
    assert set(g.measured) == {ACT_TANH, ACT_GELU}
    for act, (excess, _, ymax) in g.measured.items():
        assert ymax > 4.0  # the activations see more than their linear range
        assert 4.0 * excess < 1e-6, f"act {act}: device deviation {excess:.3e} is a finding (ceiling 1e-6 / 4)"


def test_group14_split_term_probes(tmp_path):
    _simple(tmp_path, "group 14", cases.group14(), {"128x128", "256x128", "256x256", "256x256mf16", "g256",
                                                    "f32_128x128"})


def test_group15_prefetched_residual(tmp_path):
    _simple(tmp_path, "group 15", cases.group15(), ALL_X3 | {"f32_128x128", "f32_128x64"})
