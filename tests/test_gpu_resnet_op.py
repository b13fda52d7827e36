"""Op-level conformance of the ResNet / SimAM-ResNet kernels against float64 (tools/resnet_run).

The runner launches the shipped launch_conv3x3_img, launch_bottleneck_tail (every form: the tail alone,
with the next conv1 C -> C and C -> 2C, with the in-tail shortcut), launch_resnet_stem, launch_simam and
launch_nhwc_to_tfc of libwsp_hip.so, packs the torch-layout weights with the library's own packers as
resnet_model.cpp does, and holds no arithmetic of its own; every case runs in ONE runner process whose
results the tests share.  The cases are tests/resnet_op_cases.py's, the float64 references and the
allowances (derived in its docstring) tests/resnet_op_ref.py's; tests/test_resnet_op_ref_cpu.py shows
without a GPU that the allowances hold an emulation of each kernel and reject wrong ones.  Each case prints
max |err| / allowance over EVERY element of every output and asserts it is at most 1; the guard rows on
either side of every output must come back bit-untouched; the cases marked `refuse` must be refused by
their WSP_CHECK and no other case may be.

Two bit-equalities are asserted at op level: conv3x3_img against the implicit GEMM (launch_conv_gemm_x3 in
conv2d mode, tile families 4 / 5 / 7 in turn, the same conv_kmajor + split weights), which is the claim of
conv3x3_img.hip's header, and tail2_kernel's `out` against bottleneck_tail_kernel's on the same operands.

Device part (resnet_op_ref.E_EXP for `expf` in SimAM's sigmoid), measured on the MI355X with the term at 0:
no element of any case exceeds its allowance, the measured excess is 0 and 0 ships.

No case failed on the parent commit's kernels: this change adds no kernel fix.

max |err| / allowance per case group on the MI355X (test_zz_groups prints them; 198 cases, 0.4 s of runner
time, 3.3 s for the module):
  conv3x3          c32 .097, c64 .047, c128 .018 (variant 0) / .021 (variant 3); every case bit-equal to the
                   implicit GEMM
  tail alone       c32 .027, c64 .009, c128 .002
  tail + conv1     out c32 .025, c64 .006, c128 .003; y1n c32 .148, c64 .082, c128 .038; `out` bit-equal to
                   bottleneck_tail_kernel's on all 20 cases
  tail + conv1 2C  out c32 .019, c64 .007; y1n c32 .163, c64 .084
  tail xsc (c32)   out .064, y1n .166
  stem             c32 .296, c64 .301
  simam            normal .949, offset .580, constant .973, relu .963 (the numpy emulation of
                   tests/test_resnet_op_ref_cpu.py reaches the same .973: the allowance is four single roundings
                   -- exp, 1 + E, the division, the fmaf -- budgeted at one rounding each, and among 10^5
                   elements some come close to all of them at once); the kernel's own coefficients: mean
                   .999 / .534 / .983 / 1.0, k .813 / .688 / .732 / .732 (one f32 rounding of a value just above a
                   power of two against an allowance of one rounding)
  nhwc_to_tfc      bit-equal
The conv and tail ratios are small because (K + 8) u S is a worst-case bound on K = 288 .. 1152 f32
additions and the tail's out carries conv2's allowance through sum |W3|; tests/test_resnet_op_ref_cpu.py shows
that every wrong kernel it lists still exceeds them by a factor of 45 or more.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import op_runner  # noqa: E402
import resnet_op_cases as cases  # noqa: E402
import resnet_op_ref as ref  # noqa: E402
from op_runner import untouched  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = cases.all_cases()
GROUPS = {}  # group -> largest max |err| / allowance of its cases, filled as the cases are checked


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """One runner process for all cases: [(case, result record)]."""
    out = op_runner.run("resnet_run", cases.MAGIC, [cases.op_case(c) for c in CASES], tmp_path_factory.mktemp("resnet_op"),
                        timeout=300)
    return list(zip(CASES, out))


def _rows(raw, shape, what):
    """The written block of a result buffer [(GUARD + rows + GUARD)][width], shaped `shape`, guards checked."""
    width = shape[-1]
    rows = int(np.prod(shape[:-1]))
    raw = raw.reshape(rows + 2 * cases.GUARD, width)
    assert untouched(raw[:cases.GUARD]) and untouched(raw[cases.GUARD + rows:]), f"{what}: guard rows written"
    return raw[cases.GUARD:cases.GUARD + rows].reshape(shape)


def outputs(c, arrays):
    """The kernel's outputs in the order of ref.reference(c), then what the bit-equalities compare."""
    op = c["op_name"]
    if op == "conv3x3":
        shape = (c["B"], c["F"], c["T"], c["C"])
        return [_rows(arrays[0], shape, "out")], [_rows(arrays[1], shape, "implicit GEMM out")]
    if op == "tail":
        shape = (c["B"], c["F"], c["T"])
        got = [_rows(arrays[0], shape + (4 * c["C"],), "out")]
        if c["fuse1"]:
            got.append(_rows(arrays[1], shape + (c["c1n"],), "y1n"))
        return got, [_rows(arrays[2], shape + (4 * c["C"],), "bottleneck_tail_kernel out")] if c["both"] else []
    if op == "stem":
        return [_rows(arrays[0], (c["B"], c["F"], c["T"], c["C0"]), "out")], []
    if op == "simam":
        coef = arrays[1].reshape(c["B"], 2, c["C"])  # the kernel's own mean and k
        return [_rows(arrays[0], (c["B"], c["rows"], c["C"]), "out"), coef[:, 0], coef[:, 1]], []
    return [_rows(arrays[0], (c["B"], c["T"], c["F"], c["C"]), "out")], []


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_case(results, i):
    c, r = results[i]
    if c["refuse"]:
        assert r["status"] == 1 and c["refuse"] in r["message"], f"not refused: {r['status']} {r['message']}"
        print(f"refused: {r['message']}")
        return
    assert r["status"] == 0, f"refused: {r['message']}"
    got, _ = outputs(c, r["arrays"])
    per = ref.ratios(ref.reference(c, got), got)
    for label, (q, err) in per.items():
        key = c["group"] if label == "out" else f"{c['group']} {label}"
        GROUPS[key] = max(GROUPS.get(key, 0.0), q)
        print(f"{label}: max |err| / allowance {q:.4f}   max |err| {err:.3e}")
    assert max(q for q, _ in per.values()) <= 1.0


def test_zz_conv3x3_bit_equal_to_implicit_gemm(results):
    n = 0
    for c, r in results:
        if c["op_name"] != "conv3x3" or c["refuse"] or r["status"] != 0:
            continue
        got, twin = outputs(c, r["arrays"])
        differ = int((_bits(got[0]) != _bits(twin[0])).sum())
        assert differ == 0, f"{c['name']} (tile family {c['gv']}): {differ} words differ"
        n += 1
    assert n == len(cases.CONV_CONFIGS) * len(cases.CONV_SHAPES) * len(cases.CONV_OPTIONS)


def test_zz_tail2_bit_equal_to_bottleneck_tail(results):
    n = 0
    for c, r in results:
        if c["op_name"] != "tail" or not c["both"] or c["refuse"] or r["status"] != 0:
            continue
        got, plain = outputs(c, r["arrays"])
        differ = int((_bits(got[0]) != _bits(plain[0])).sum())
        assert differ == 0, f"{c['name']}: {differ} words differ"
        n += 1
    assert n == 5 * len(cases.TAIL_SHAPES)  # C = 32 / 64 with the next conv1 C -> C and C -> 2C, C = 128 C -> C


def test_zz_groups():
    """Prints the largest ratio per case group (the figures DESIGN.md section 4 records)."""
    for g in sorted(GROUPS):
        print(f"{g}: {GROUPS[g]:.4f}")
    assert all(v <= 1.0 for v in GROUPS.values())
