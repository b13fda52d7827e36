"""Op-level conformance of ECAPA's own kernels against float64 (tools/ecapa_run).

The runner launches the shipped launch_res2_chain, launch_astp_fused, launch_astp_pool,
launch_frame_stats, launch_small_linear, launch_residual_scale and, for the gated A tail and the
SE-Res2Block seam, launch_conv_gemm_x3 of libwsp_hip.so and holds no arithmetic of its own; every
case runs in ONE runner process whose results the tests share.  The cases are
tests/ecapa_op_cases.py's, the float64 references and the allowances (formulas in its docstring)
tests/ecapa_op_ref.py's; tests/test_ecapa_op_ref_cpu.py shows without a GPU that the allowances hold
an emulation of each kernel and reject wrong ones.  Each case prints max |err| / allowance and
asserts it is at most 1; guard rows and guard columns must come back bit-untouched; the cases marked
`refuse` must be refused by a WSP_CHECK and no other case may be.

Device parts (ecapa_op_ref.E_EXP for `__expf` / `expf` in the ASTP kernels, E_ACT for `tanhf` / `expf`
in small_linear), measured on the MI355X with both terms at 0: no element of any case exceeds its
allowance, the measured excess is 0 and 0 ships for both.

max |err| / allowance per case group on the MI355X (test_zz_groups prints them):
  chain            w64 .190 / .224 / .226 (variants 0 / 2 / 3), w128 .207 / .225 / .201 / .205 (0 / 2 / 3 / 4),
                   long strips (66-row strips on 256 CUs) .151, one-sided w64 .139, w128 .080
  astp_fused       mean .082 / .454 / .048 / .057, sd .142 / .142 / 1.0 / .142 (x regimes a / b / c / d);
                   staircases mean .032, sd .142; full-top staircases mean .022, sd .037.  (.142 is
                   float32(sqrt(floor)) against the float64 one, in the 2 ulps below it.)  Regime c: the
                   kernel's E[x^2] - mu^2 cancels to the floor, which is the interval's lower end, so 1.0
                   is reached by construction.
  astp_pool        vector mean .109 / .239 / .118 / .103, scalar mean .076 / .123 / .108 / .108; sd as above
  frame_stats      scalar mean .302, std .240; vector mean 1.0 (a correctly rounded mean just above a
                   power of two is u |mean| off, the allowance), std .409
  small_linear     one pass .187, split-K .063
  residual_scale   .988 (one rounding against an allowance of one rounding)
  gated tail       .168 (parent commit, measured on half of the grid: 3007 - 8700 on the twelve cases with
                   K - gate_k0 in {128, 384}, whose gate rows the kernel staged in 256-column pieces;
                   fixed in conv_gemm_x3_t6.hip)
  seam             .148, seam_out bit-equal to float32(fma(h, g, x))
"""
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ecapa_op_cases as cases  # noqa: E402
import ecapa_op_ref as ref  # noqa: E402
import op_runner  # noqa: E402
from op_runner import untouched  # noqa: E402

pytestmark = pytest.mark.gpu

SPECS = cases.all_cases()
GROUPS = {}  # group -> largest max |err| / allowance of its cases, filled as the cases are checked


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """One runner process for all cases: [(case, result record)]."""
    built = [cases.materialize(s) for s in SPECS]
    out = op_runner.run("ecapa_run", cases.MAGIC, [cases.op_case(c) for c in built], tmp_path_factory.mktemp("ecapa_op"),
                        timeout=600)
    return list(zip(built, out))


def _rows(raw, rows, ld, front, back, width, what):
    """The written block [rows][width] of a result buffer [(front + rows + back)][ld], guards checked."""
    raw = raw.reshape(front + rows + back, ld)
    assert untouched(raw[:front]) and untouched(raw[front + rows:]), f"{what}: guard rows written"
    assert untouched(raw[front:front + rows, width:]), f"{what}: guard columns written"
    return raw[front:front + rows, :width]


def outputs(c, arrays):
    """The kernel's outputs in the order of ref.reference(c)."""
    op = c["op_name"]
    if op == "res2":
        return [_rows(arrays[0], c["M"], c["ldo"], 4, 4, 7 * c["w"], "out")]
    if op in ("astp_fused", "astp_pool"):
        o = _rows(arrays[0], c["B"], 2 * c["C"], 1, 1, 2 * c["C"], "out")
        return [o[:, :c["C"]], o[:, c["C"]:]]
    if op == "frame_stats":
        C, so = c["C"], c["std_off"]
        o = _rows(arrays[0], c["B"], c["ldo"], 1, 1, c["ldo"], "out")
        written = np.zeros(c["ldo"], bool)
        written[:C] = True
        if c["with_std"]:
            written[so:so + C] = True
        assert untouched(o[:, ~written]), "columns outside the mean and the std written"
        return [o[:, :C]] + ([o[:, so:so + C]] if c["with_std"] else [])
    if op == "small_linear":
        return [_rows(arrays[0], c["R"], c["ldo"], 1, 1, c["N"], "out")]
    if op == "residual_scale":
        return [_rows(arrays[0], c["M"], c["C"], 1, 1, c["C"], "out")]
    got = [_rows(arrays[0], c["M"], c["ldo"], 4, 4, c["N"], "out")]
    if op == "seam":
        got.append(_rows(arrays[1], c["M"], c["ldso"], 4, 4, c["K"], "seam_out"))
    return got


@pytest.mark.parametrize("i", range(len(SPECS)), ids=[s["name"] for s in SPECS])
def test_case(results, i):
    c, r = results[i]
    own = struct.unpack("<2I", r["own"])
    if c["refuse"]:
        assert r["status"] == 1 and c["refuse"] in r["message"], f"not refused: {r}"
        if c["op_name"] in ("gate", "seam"):
            assert own[0] == 0, "conv_gemm_x3_gate_ok / _seam_ok said yes to a launch that was refused"
        print(f"refused: {r['message']}")
        return
    assert r["status"] == 0, f"refused: {r['message']}"
    if c["op_name"] in ("gate", "seam"):
        assert own[0] == 1, "conv_gemm_x3_gate_ok / _seam_ok said no to a launch that ran"
    if c["op_name"] == "res2":
        rout, ncu = own
        if c["variant"] == 4:
            assert rout == max(64, -(-c["M"] // (2 * ncu)))
        else:
            assert rout == 128 - 12 * c["dil"]
        if c["group"] == "res2 long strips":
            assert rout == -(-c["M"] // (2 * ncu)) and rout > 64, f"strips of {rout} rows on {ncu} CUs: not the long-strip path"
    per = ref.ratios(ref.reference(c), outputs(c, r["arrays"]))
    for label, (q, err) in per.items():
        key = c["group"] if label == "out" else f"{c['group']} {label}"
        GROUPS[key] = max(GROUPS.get(key, 0.0), q)
        print(f"{label}: max |err| / allowance {q:.4f}   max |err| {err:.3e}")
    assert max(q for q, _ in per.values()) <= 1.0


def test_zz_split_k_is_its_own_path(results):
    """The split-K twins ran on the same operands as their one-pass cases and sum in another order: they
    agree within the sum of the allowances, and at least one pair differs in some bit."""
    by_name = {c["name"]: (c, r) for c, r in results}
    differ = 0
    for name, (c, r) in by_name.items():
        if c["op_name"] != "small_linear" or c["scratch"] != 1 or c["refuse"]:
            continue
        c1, r1 = by_name[name.replace("splitk", "onepass")]
        assert np.array_equal(c["wt"], c1["wt"]) and np.array_equal(c["in"], c1["in"])
        a, b = outputs(c, r["arrays"])[0], outputs(c1, r1["arrays"])[0]
        _, allow = ref.small_linear_reference(c)
        assert (np.abs(a.astype(np.float64) - b) <= 2 * allow).all()
        differ += int(not np.array_equal(a, b))
    assert differ > 0


def test_zz_groups():
    """Prints the largest ratio per case group (the figures DESIGN.md section 4 records)."""
    for g in sorted(GROUPS):
        print(f"{g}: {GROUPS[g]:.4f}")
    assert all(v <= 1.0 for v in GROUPS.values())
