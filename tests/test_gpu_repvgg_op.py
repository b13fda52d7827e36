"""Op-level conformance of the RepVGG / RepSPK kernels against float64 (tools/repvgg_oprun).

The runner launches the shipped launchers of libwsp_hip.so (launch_rsbb_conv, launch_repvgg_stem) and holds
no reference arithmetic; one run serves all tests.  Cases: tests/repvgg_op_cases.py; float64 references and
the derived allowances: tests/repvgg_op_ref.py (its docstring has the derivation;
tests/test_repvgg_op_ref_cpu.py shows on the CPU that they pass a faithful emulation and reject seven wrong
kernels).  Every output element is held to its allowance; the pad channels of the padded widths must be
exact zeros; guard rows, guard columns and the columns beside the slice written must come back as the
untouched NaN fill; the four refusals come back with status 1 and their message.

Measured (MI355X, these seeds), max |err| / allowance per case group:
rsbb_conv 32 -> 32 s1: .063; 32 -> 64 s2: .052; 64 -> 128 s2: .024; 128 -> 256 s2: .013; the padded widths
48 -> 48 (as 64 -> 64) s1: .031, 48 -> 96 (as 64 -> 128) s2: .024 -- the (K + 8) 2^-24 S term is a worst case
that grows with K = 17 cin; repvgg_stem 9 taps: .020, 17 taps: .015, 25 taps: .008.  No element exceeds its
allowance; the pad channels are exact zeros.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import op_runner  # noqa: E402
import repvgg_op_ref as R  # noqa: E402
from op_runner import untouched as _untouched  # noqa: E402
from repvgg_op_cases import (BLOCK_CASES, CASES, MAGIC, NARRAYS, NH, OP_BLOCK, OWN, REFUSED, STEM_CASES,  # noqa: E402
                             WIDTHS)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def res(tmp_path_factory):
    """One runner process for all cases (op_runner.run's table has no entry for this runner)."""
    d = tmp_path_factory.mktemp("repvgg_op")
    fin, fout = os.path.join(str(d), "cases.bin"), os.path.join(str(d), "results.bin")
    op_runner.write_cases(fin, MAGIC, [(c["op"], c["hdr"], c["arrays"]) for c in CASES], NH)
    p = op_runner.launch("repvgg_oprun", fin, fout)
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
    assert torch.isfinite(got).all() and float(got.min()) >= 0.0, tag
    ratio = R.ratio(got, want)
    print(f"  {tag}: |err| / allowance = {ratio:.3f}")
    assert ratio <= 1.0, f"{tag}: |err| / allowance = {ratio:.3f}"
    return ratio


@pytest.mark.parametrize("cin,N,stride,real", WIDTHS, ids=[f"{w[0]}to{w[1]}s{w[2]}{'pad' if w[3] else ''}" for w in WIDTHS])
def test_rsbb_block(res, cin, N, stride, real):
    worst = 0.0
    for c, r in zip(CASES, res):
        if c["op"] == OP_BLOCK and c in BLOCK_CASES and (c["cin"], c["N"], c["stride"], c["real"]) == (cin, N, stride, real):
            worst = max(worst, _check(c, r, R.reference(c)))
            if real:  # the pad channels stay exact zeros
                raw = r["out"].reshape(c["M"] + 8, c["ldo"])[:c["M"], c["ooff"] + real[1]:c["ooff"] + N]
                assert not raw.any()
    print(f"\nrsbb_conv {cin} -> {N} stride {stride}: max |err| / allowance {worst:.3f}")
    assert worst > 0.0


def test_stem(res):
    worst = {9: 0.0, 17: 0.0, 25: 0.0}
    for c, r in zip(STEM_CASES, res[len(BLOCK_CASES):]):
        worst[c["taps"]] = max(worst[c["taps"]], _check(c, r, R.reference(c)))
    print(f"\nrepvgg_stem: max |err| / allowance 9 taps {worst[9]:.3f}, 17 taps {worst[17]:.3f}, 25 taps {worst[25]:.3f}")
    assert min(worst.values()) > 0.0


def test_refusals(res):
    n = len(BLOCK_CASES) + len(STEM_CASES)
    for (c, msg), r in zip(REFUSED, res[n:]):
        assert r["status"] == 1 and msg in r["message"], (c["hdr"], r["status"], r["message"])
