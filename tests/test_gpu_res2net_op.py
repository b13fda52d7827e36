"""Op-level conformance of the Res2Net kernels against float64 (tools/res2net_oprun).

The runner launches the shipped launchers of libwsp_hip.so (launch_res2_tail, launch_eres_pw with
EresConvArgs::ksplit, launch_eres_conv3x3 for one refusal) and holds no reference arithmetic; one run
serves all tests.  Cases: tests/res2net_op_cases.py; float64 references and the derived allowances:
tests/res2net_op_ref.py (its docstring has the derivation; tests/test_res2net_op_ref_cpu.py shows on
the CPU that they pass a faithful emulation and reject the wrong kernels).  Every output element is
held to its allowance; guard rows, guard columns and the columns beside the slice written must come
back as the untouched NaN fill; the four refusals come back with status 1 and their message.

Measured (MI355X, these seeds), max |err| / allowance per case group:
res2_tail w = 16: .279 (hot case .188); w = 32: .094 (.085); w = 64: .050 (.050); w = 128: .017 (.017);
w = 256: .004 (.004) -- the (K + 8) 2^-24 S term is a worst case that grows with both products' K;
eres_pw with ksplit: .317.  No element exceeds its allowance.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import op_runner  # noqa: E402
import res2net_op_ref as R  # noqa: E402
from op_runner import untouched as _untouched  # noqa: E402
from res2net_op_cases import (CASES, CLAMP, MAGIC, NARRAYS, NH, OP_PW, OP_TAIL, OWN, PW_CASES, REFUSED,  # noqa: E402
                              TAIL_CASES, WIDTHS)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def res(tmp_path_factory):
    """One runner process for all cases (op_runner.run's table has no entry for this runner)."""
    d = tmp_path_factory.mktemp("res2net_op")
    fin, fout = os.path.join(str(d), "cases.bin"), os.path.join(str(d), "results.bin")
    op_runner.write_cases(fin, MAGIC, [(c["op"], c["hdr"], c["arrays"]) for c in CASES], NH)
    p = op_runner.launch("res2net_oprun", fin, fout)
    assert p.returncode == 0, f"runner status {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}"
    out = op_runner.read_results(fout, len(CASES), OWN, NARRAYS)
    return [dict(r, out=r["arrays"][0] if r["status"] == 0 else None) for r in out]


def _check(c, r, want):
    """Guards untouched, every element within its allowance; returns max |err| / allowance."""
    tag = f"op {c['op']} {c['hdr']}"
    assert r["status"] == 0, f"{tag} refused: {r['message']}"
    M, N, ldo, ooff = c["M"], c["N"], c["ldo"], c["ooff"]
    raw = r["out"].reshape(M + 8, ldo)
    assert _untouched(raw[M:]), f"{tag}: guard rows written"
    assert _untouched(raw[:M, :ooff]) and _untouched(raw[:M, ooff + N:]), f"{tag}: columns beside the slice written"
    got = torch.from_numpy(np.ascontiguousarray(raw[:M, ooff:ooff + N])).double()
    assert torch.isfinite(got).all(), tag
    if c["op"] == OP_TAIL or c["act"] == CLAMP:
        assert float(got.min()) >= 0.0 and float(got.max()) <= 20.0, tag
    ratio = R.ratio(got, want)
    assert ratio <= 1.0, f"{tag}: |err| / allowance = {ratio:.3f}"
    return ratio


@pytest.mark.parametrize("w", WIDTHS)
def test_fused_tail(res, w):
    worst = hot = 0.0
    for c, r in zip(CASES, res):
        if c["op"] == OP_TAIL and c["w"] == w:
            ratio = _check(c, r, R.tail_reference(c))
            if c["hot"]:
                hot = ratio
                assert bool((r["out"].reshape(c["M"] + 8, c["ldo"])[:c["M"]] == 20.0).any())
            worst = max(worst, ratio)
    print(f"\nres2_tail w = {w}: max |err| / allowance {worst:.3f} (hot case {hot:.3f})")
    assert worst > 0.0


def test_pointwise_conv_over_the_concatenated_operand(res):
    worst = 0.0
    for c, r in zip(PW_CASES, res[len(TAIL_CASES):]):
        assert c["op"] == OP_PW
        worst = max(worst, _check(c, r, R.pw_reference(c)))
    print(f"\neres_pw with ksplit: max |err| / allowance {worst:.3f}")
    assert worst > 0.0


def test_refusals(res):
    n = len(TAIL_CASES) + len(PW_CASES)
    for (c, msg), r in zip(REFUSED, res[n:]):
        assert r["status"] == 1 and msg in r["message"], (c["hdr"], r["status"], r["message"])
