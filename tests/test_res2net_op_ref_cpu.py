"""The Res2Net op-level reference and allowance (tests/res2net_op_ref.py) without a GPU: a faithful
CPU emulation of each kernel (bf16x3 products, f32 sums) passes on every case, every wrong kernel
listed there is rejected on at least one case, the hot cases reach the clamp's ceiling in the float64
reference, and the case table covers what it says."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import res2net_op_ref as R  # noqa: E402
from res2net_op_cases import PLANES, PW_CASES, REFUSED, TAIL_CASES, WIDTHS  # noqa: E402

_REFS = {}


def _ref(kind, i):
    """The float64 reference of a case, computed once."""
    if (kind, i) not in _REFS:
        _REFS[(kind, i)] = R.tail_reference(TAIL_CASES[i]) if kind == "tail" else R.pw_reference(PW_CASES[i])
    return _REFS[(kind, i)]


def test_case_table():
    got = {(c["w"], (c["B"], c["F"], c["T"]), c["has_res"]) for c in TAIL_CASES if not c["hot"]}
    assert got == {(w, p, r) for w in WIDTHS for p in PLANES for r in (False, True)}
    assert all(c["N"] == 4 * c["w"] for c in TAIL_CASES)
    assert sorted(c["w"] for c in TAIL_CASES if c["hot"]) == list(WIDTHS)
    assert {(c["cin"], c["ksplit"], c["stride"]) for c in PW_CASES} >= {
        (cin, ks, st) for cin, ks in ((32, 16), (64, 32), (512, 256)) for st in (1, 2)}
    assert len(REFUSED) == 4


@pytest.mark.parametrize("i", range(len(TAIL_CASES)), ids=[f"w{c['w']}-{c['B']}x{c['F']}x{c['T']}-res{int(c['has_res'])}"
                                                            f"{'-hot' if c['hot'] else ''}" for c in TAIL_CASES])
def test_faithful_tail_emulation_passes(i):
    r = R.ratio(R.emulate_tail(TAIL_CASES[i]), _ref("tail", i))
    assert 0.0 < r <= 1.0, r


@pytest.mark.parametrize("i", range(len(PW_CASES)))
def test_faithful_pw_emulation_passes(i):
    r = R.ratio(R.emulate_pw(PW_CASES[i]), _ref("pw", i))
    assert 0.0 < r <= 1.0, r


def test_hot_cases_reach_the_ceiling():
    """s and out have elements pinned at 20 and elements below it in the float64 reference."""
    for i, c in enumerate(TAIL_CASES):
        if c["hot"]:
            r = _ref("tail", i)
            for pre in (r["pre1"], r["pre"]):
                assert float((pre > 20.5).double().mean()) > 0.05 and float((pre < 19.5).double().mean()) > 0.05, c["hdr"]
            assert bool((r["s"] == 20.0).any()) and bool((r["out"] == 20.0).any())


# the smallest width keeps this quick; a defect that needs a shape names it
def _small(pred):
    return [i for i, c in enumerate(TAIL_CASES) if c["w"] <= 32 and pred(c)]


@pytest.mark.parametrize("wrong", R.TAIL_WRONG)
def test_wrong_tail_is_rejected(wrong):
    pick = {"no_ceiling_out": lambda c: c["hot"], "no_residual": lambda c: c["has_res"],
            "cross_utterance": lambda c: c["B"] > 1}.get(wrong, lambda c: not c["hot"])
    worst = max(R.ratio(R.emulate_tail(TAIL_CASES[i], wrong), _ref("tail", i)) for i in _small(pick))
    assert worst > 1.0, (wrong, worst)


@pytest.mark.parametrize("wrong", R.PW_WRONG)
def test_wrong_pw_is_rejected(wrong):
    worst = max(R.ratio(R.emulate_pw(c, wrong), _ref("pw", i)) for i, c in enumerate(PW_CASES) if c["cin"] <= 64)
    assert worst > 1.0, (wrong, worst)
