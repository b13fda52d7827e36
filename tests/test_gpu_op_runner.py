"""The framing of a real op-level runner (tools/op_runner.h), exercised through tools/xi_run.

The base file holds one valid offset-table case (B = 1, one shrink).  The same file with a wrong
magic, an unknown version, a truncated last array, an array count that disagrees with the header or four
trailing bytes must end the run with status 2, a message on stderr that names the fault, and a result
file no reader takes for a run's.  All of these are refusals of the file itself: no launch goes wrong.
"""
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import op_runner  # noqa: E402
from op_runner import FILL  # noqa: E402

pytestmark = pytest.mark.gpu

MAGIC, OFFS = 0x58505357, 2
OFF = np.array([0, 123], np.int32)
SHRINK = 14


def _case(off=OFF):
    return (OFFS, [1, 1, SHRINK, 0, 0, 0], [off])


def test_valid_file(tmp_path):
    (r,) = op_runner.run("xi_run", MAGIC, [_case()], tmp_path)
    assert r["status"] == 0 and r["message"] == "" and len(r["arrays"]) == 1
    words = r["arrays"][0].view(np.uint32)
    assert words.size == 4 and words[0] == FILL and words[-1] == FILL, "guard word touched"
    assert words[1:-1].view(np.int32).tolist() == [0, 123 - SHRINK]


def _valid_bytes(tmp_path, case=None):
    path = str(tmp_path / "valid.bin")
    op_runner.write_cases(path, MAGIC, [case or _case()], op_runner.LAYOUT["xi_run"][0])
    with open(path, "rb") as f:
        return f.read()


FAULTS = {
    "magic": (lambda b: struct.pack("<I", 0x44505357) + b[4:], "magic"),  # cam_dense_run's file
    "version": (lambda b: b[:4] + struct.pack("<I", 2) + b[8:], "version"),
    "truncated": (lambda b: b[:-4], "file too short"),
    "count": (None, "off: count does not match the header"),
    "trailing": (lambda b: b + b"\0\0\0\0", "trailing bytes"),
}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_malformed_file(tmp_path, fault):
    edit, names = FAULTS[fault]
    if edit is None:
        buf = _valid_bytes(tmp_path, _case(np.array([0, 100, 123], np.int32)))  # B + 1 = 2 offsets promised
    else:
        buf = edit(_valid_bytes(tmp_path))
    fin, fout = str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    with open(fin, "wb") as f:
        f.write(buf)
    p = op_runner.launch("xi_run", fin, fout, timeout=60)
    assert p.returncode == 2, f"runner status {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}"
    assert p.stderr.startswith("xi_run: bad case: ") and names in p.stderr, p.stderr
    with pytest.raises(AssertionError):
        op_runner.read_results(fout, 1, *op_runner.LAYOUT["xi_run"][1:])
