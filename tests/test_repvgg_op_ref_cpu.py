"""The RepVGG op-level reference and allowance (tests/repvgg_op_ref.py) without a GPU: a faithful CPU
emulation of each kernel (bf16x3 products, f32 sums) passes on every case, every wrong kernel listed there is
rejected on at least one case, and the case table covers what it says."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import repvgg_op_ref as R  # noqa: E402
from repvgg_op_cases import BLOCK_CASES, PLANES, REFUSED, STEM_CASES, WIDTHS  # noqa: E402
from wespeaker_hubert_amd import arch as A  # noqa: E402

_REFS = {}


def _ref(kind, i):
    """The float64 reference of a case, computed once."""
    if (kind, i) not in _REFS:
        _REFS[(kind, i)] = R.reference((BLOCK_CASES if kind == "block" else STEM_CASES)[i])
    return _REFS[(kind, i)]


def test_case_table():
    got = {(c["cin"], c["N"], c["stride"], c["real"], (c["B"], c["Fi"], c["Ti"])) for c in BLOCK_CASES}
    assert got == {w + (p,) for w in WIDTHS for p in PLANES}
    assert any(c["M"] % 128 for c in BLOCK_CASES) and any(c["M"] > 128 for c in BLOCK_CASES)
    assert any(c["ooff"] > 0 and c["ldo"] > c["N"] and c["ldx"] > c["cin"] for c in BLOCK_CASES)
    assert (2, 3, 5) in PLANES  # F = 3 < 5: every output position has live taps outside the plane
    assert {(c["C0"], c["taps"], c["F"]) for c in STEM_CASES} >= {(c0, k, f) for c0 in (32, 48, 64) for k in (9, 17)
                                                                  for f in (8, 80)}
    assert len(REFUSED) == 4
    for c in BLOCK_CASES:  # a folded kernel: zero at the dead taps, and the pad channels all zero
        for kf, kt in A.RSBB_DEAD_TAPS:
            assert not c["w"][:, :, kf, kt].any()
        if c["real"]:
            ci, co = c["real"]
            assert not c["x"][:, ci:c["cin"]].any() and not c["w"][co:].any() and not c["w"][:, ci:].any()
            assert not np.asarray(_ref("block", BLOCK_CASES.index(c))["out"])[:, co:].any()


@pytest.mark.parametrize("i", range(len(BLOCK_CASES)),
                         ids=[f"{c['cin']}to{c['N']}s{c['stride']}-{c['B']}x{c['Fi']}x{c['Ti']}" for c in BLOCK_CASES])
def test_faithful_block_emulation_passes(i):
    r = R.ratio(R.emulate_block(BLOCK_CASES[i]), _ref("block", i))
    assert 0.0 < r <= 1.0, r


@pytest.mark.parametrize("i", range(len(STEM_CASES)))
def test_faithful_stem_emulation_passes(i):
    r = R.ratio(R.emulate_stem(STEM_CASES[i]), _ref("stem", i))
    assert 0.0 < r <= 1.0, r


@pytest.mark.parametrize("wrong", R.BLOCK_WRONG)
def test_wrong_block_is_rejected(wrong):
    pick = {"stride_on_one_axis": lambda c: c["stride"] == 2 and c["Ti"] > 2,
            "cross_utterance": lambda c: c["B"] > 1 and (c["stride"] == 1 or c["Fi"] % 2 == 0)}.get(wrong, lambda c: True)
    idx = [i for i, c in enumerate(BLOCK_CASES) if c["cin"] <= 64 and pick(c)]
    assert idx
    worst = max(R.ratio(R.emulate_block(BLOCK_CASES[i], wrong), _ref("block", i)) for i in idx)
    assert worst > 1.0, (wrong, worst)
