"""CPU checks of the Python side of the op-level runners' file format (tests/op_runner.py)."""
import os
import re
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import op_runner  # noqa: E402
from op_runner import FILL, MAGIC_OUT  # noqa: E402

MAGIC = 0x54505357  # 'WSPT': no runner's


def test_write_cases(tmp_path):
    rng = np.random.default_rng(1)
    f = rng.standard_normal((3, 5)).astype(np.float32)
    f[0, 0] = np.array([FILL], np.uint32).view(np.float32)[0]  # a NaN payload travels bit for bit
    i = np.array([0, -7, 2 ** 31 - 1, -2 ** 31], np.int32)
    cases = [(1, [4, -5, 6], [f, i, np.zeros(0, np.float32)]), (2, [], []), (7, list(range(8)), [i])]
    path = str(tmp_path / "cases.bin")
    op_runner.write_cases(path, MAGIC, cases, 8)
    cur = op_runner.Cursor(path)
    assert cur.take("III") == (MAGIC, 1, 3)
    assert cur.take("I8i") == (1, 4, -5, 6, 0, 0, 0, 0, 0)  # the header is padded with zeros to nh ints
    got_f, got_i, got_e = cur.arr(), cur.arr("<i4"), cur.arr()
    assert got_f.dtype == np.float32 and np.array_equal(got_f.view(np.uint32), f.reshape(-1).view(np.uint32))
    assert np.array_equal(got_i, i) and got_e.size == 0
    assert cur.take("I8i") == (2, 0, 0, 0, 0, 0, 0, 0, 0)
    assert cur.take("I8i") == (7, 0, 1, 2, 3, 4, 5, 6, 7) and np.array_equal(cur.arr("<i4"), i)
    cur.end()
    with pytest.raises(AssertionError, match="file too short"):
        cur.take("I")
    # the generic reader, told how many arrays each header promises (here: its op code)
    back = op_runner.read_cases(path, MAGIC, 8, lambda op, hdr: {1: 3, 2: 0, 7: 1}[op])
    assert [(op, hdr) for op, hdr, _ in back] == [(op, hdr + [0] * (8 - len(hdr))) for op, hdr, _ in cases]
    assert [len(a) for _, _, a in back] == [3, 0, 1]
    assert np.array_equal(back[0][2][0].view(np.uint32), f.reshape(-1).view(np.uint32))
    assert np.array_equal(back[0][2][1].view(np.int32), i) and np.array_equal(back[2][2][0].view(np.int32), i)
    with pytest.raises(AssertionError):
        op_runner.read_cases(path, MAGIC + 1, 8, lambda op, hdr: 0)
    with pytest.raises(AssertionError):  # one array too few promised: the next case does not parse
        op_runner.read_cases(path, MAGIC, 8, lambda op, hdr: {1: 2, 7: 1}.get(op, 0))
    with open(path, "ab") as fh:
        fh.write(b"\0")
    with pytest.raises(AssertionError, match="trailing bytes"):
        op_runner.read_cases(path, MAGIC, 8, lambda op, hdr: {1: 3, 2: 0, 7: 1}[op])
    with pytest.raises(AssertionError):  # an 8-byte dtype is not silently narrowed
        op_runner.write_cases(path, MAGIC, [(1, [], [np.zeros(2)])], 8)
    with pytest.raises(AssertionError):  # nor a header cut to nh ints
        op_runner.write_cases(path, MAGIC, [(1, list(range(9)), [])], 8)


def test_layout_table_matches_the_runners():
    """op_runner.LAYOUT restates each runner's Layout; a difference would mis-parse files, so it fails here."""
    for name, (nh, own, narrays) in op_runner.LAYOUT.items():
        with open(os.path.join(op_runner.ROOT, "tools", name + ".cpp")) as f:
            (found,) = re.findall(r'op_runner_main\(argc, argv, "(\w+)", 0x[0-9a-f]+u, Layout\{(\d+), (\d+), (\d+)\}', f.read())
        assert found == (name, str(nh), str(own), str(narrays or 0)), name
    tools = os.listdir(os.path.join(op_runner.ROOT, "tools"))
    assert sorted(n[:-4] for n in tools if n.endswith("_run.cpp")) == sorted(op_runner.LAYOUT)


def _text(s):
    return struct.pack("<I", len(s)) + s


def _results_file(counted=True):
    a = np.array([1.5, -2.0, 0.0], np.float32)
    b = np.array([FILL, 7], np.uint32)
    own = struct.pack("<24si", b"256x64", 256)  # a runner's own words, as conv_gemm_run's tile and block rows
    refused = struct.pack("<I", 1) + own + _text(b"attn: bad shape")
    ran = (struct.pack("<I", 0) + own + _text(b"") + (struct.pack("<I", 2) if counted else b"")
           + struct.pack("<I", a.size) + a.tobytes() + struct.pack("<I", b.size) + b.tobytes())
    return struct.pack("<II", MAGIC_OUT, 2) + refused + ran, a, b, own


@pytest.mark.parametrize("counted", [True, False])
def test_read_results(tmp_path, counted):
    buf, a, b, own = _results_file(counted)
    path = tmp_path / "results.bin"
    path.write_bytes(buf)
    refused, ran = op_runner.read_results(str(path), 2, own=7, narrays=None if counted else 2)
    assert refused == dict(status=1, message="attn: bad shape", own=own, arrays=[])
    assert (ran["status"], ran["message"], ran["own"]) == (0, "", own)
    assert len(ran["arrays"]) == 2 and all(x.dtype == np.float32 for x in ran["arrays"])
    assert np.array_equal(ran["arrays"][0], a)
    assert np.array_equal(ran["arrays"][1].view(np.uint32), b)
    assert op_runner.untouched(ran["arrays"][1][:1]) and not op_runner.untouched(ran["arrays"][1])


@pytest.mark.parametrize("fault", ["magic", "count", "trailing", "truncated", "empty"])
def test_read_results_rejects(tmp_path, fault):
    buf, _, _, _ = _results_file()
    n = 2
    if fault == "magic":
        buf = struct.pack("<I", MAGIC) + buf[4:]
    elif fault == "count":
        n = 3
    elif fault == "trailing":
        buf += b"\0\0\0\0"
    elif fault == "truncated":
        buf = buf[:-4]
    else:  # what a runner that exits with a status other than 0 leaves
        buf = b""
    path = tmp_path / "results.bin"
    path.write_bytes(buf)
    with pytest.raises(AssertionError):
        op_runner.read_results(str(path), n, own=7)
