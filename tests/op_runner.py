"""The Python side of the op-level runners' file format (the head comment of tools/op_runner.h).

A case is `(op, hdr, arrays)`: the op code, the header ints the op uses (padded with zeros to the
runner's `nh`) and its arrays in the order the runner's op table lists them.  A result is
`dict(status, message, own, arrays)`: status 0 = ran, 1 = refused by a WSP_CHECK of the library
(`message`), `own` the runner's own bytes of the record, `arrays` the result words as float32 (a test
that wants them as integers views them, which keeps every bit).
"""
import os
import struct
import subprocess
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAGIC_OUT, VERSION = 0x52505357, 1
FILL = 0x7FC5A5A5  # the NaN pattern result buffers are pre-filled with
# Each runner's Layout, as the last line of its tools/<name>.cpp gives it: header ints of a case, words of
# the runner's own in a result record, result arrays of a case that ran (None: their number is in the file).
LAYOUT = {"conv_gemm_run": (43, 7, 3), "cam_dense_run": (8, 0, 2), "eres2net_run": (16, 0, 1),
          "gemini_run": (16, 0, 1), "ssl_run": (16, 0, None), "xi_run": (8, 0, 1),
          "ecapa_run": (16, 2, None), "resnet_run": (16, 0, None)}


def untouched(x):
    return bool((np.ascontiguousarray(x).view(np.uint32) == FILL).all())


def write_cases(path, magic, cases, nh):
    buf = [struct.pack("<III", magic, VERSION, len(cases))]
    for op, hdr, arrays in cases:
        assert len(hdr) <= nh
        buf.append(struct.pack(f"<I{nh}i", op, *(int(v) for v in hdr), *([0] * (nh - len(hdr)))))
        for a in arrays:
            a = np.ascontiguousarray(a)
            assert a.dtype.itemsize == 4, a.dtype
            a = a.astype("<i4") if a.dtype.kind in "iu" else a.astype("<f4")
            buf.append(struct.pack("<I", a.size))
            buf.append(a.tobytes())
    with open(path, "wb") as f:
        f.write(b"".join(buf))


class Cursor:
    """Little-endian reads over a whole file; every read asserts that the bytes are there."""

    def __init__(self, path):
        with open(path, "rb") as f:
            self.d, self.o = f.read(), 0

    def take(self, fmt):
        assert self.o + struct.calcsize("<" + fmt) <= len(self.d), "file too short"
        v = struct.unpack_from("<" + fmt, self.d, self.o)
        self.o += struct.calcsize("<" + fmt)
        return v

    def arr(self, dtype="<f4"):
        (n,) = self.take("I")
        assert self.o + 4 * n <= len(self.d), "file too short"
        x = np.frombuffer(self.d, dtype=dtype, count=n, offset=self.o).copy()
        self.o += 4 * n
        return x

    def text(self):
        (n,) = self.take("I")
        return self.take(f"{n}s")[0].decode()

    def end(self):
        assert self.o == len(self.d), "trailing bytes"


def read_cases(path, magic, nh, narrays):
    """The Python twin of a runner's parser: (op, hdr, arrays) per case, every array as float32 words.
    `narrays(op, hdr)` is the number of arrays the header promises, as the runner's op table decides it."""
    cur = Cursor(path)
    got, version, n = cur.take("III")
    assert got == magic and version == VERSION
    out = []
    for _ in range(n):
        (op,) = cur.take("I")
        hdr = list(cur.take(f"{nh}i"))
        out.append((op, hdr, [cur.arr() for _ in range(narrays(op, hdr))]))
    cur.end()
    return out


def read_results(path, n, own=0, narrays=None):
    """`own` words of the runner's own per record; `narrays` result arrays, None: their number is in the file."""
    cur = Cursor(path)
    magic, cnt = cur.take("II")
    assert magic == MAGIC_OUT and cnt == n
    out = []
    for _ in range(n):
        (status,) = cur.take("I")
        assert status in (0, 1)
        r = dict(status=status, own=cur.take(f"{4 * own}s")[0], message=cur.text(), arrays=[])
        if status == 0:
            na = cur.take("I")[0] if narrays is None else narrays
            r["arrays"] = [cur.arr() for _ in range(na)]
        out.append(r)
    cur.end()
    return out


def launch(name, fin, fout, timeout=120):
    """One process of tools/<name> on the case file `fin`; one attempt, never retried."""
    runner = os.path.join(ROOT, "tools", name)
    if not os.path.exists(runner):
        pytest.fail(f"{runner} not built (run __graft_entry__.build())")
    return subprocess.run([runner, fin, fout], capture_output=True, text=True, timeout=timeout)


def run(name, magic, cases, tmp_dir, timeout=120):
    """Writes `cases`, runs tools/<name> on them once and returns its results."""
    nh, own, narrays = LAYOUT[name]
    fin, fout = os.path.join(str(tmp_dir), "cases.bin"), os.path.join(str(tmp_dir), "results.bin")
    write_cases(fin, magic, cases, nh)
    t0 = time.perf_counter()
    p = launch(name, fin, fout, timeout)
    print(f"\n{name}: {len(cases)} cases, {time.perf_counter() - t0:.2f} s")
    assert p.returncode == 0, f"runner status {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}"
    return read_results(fout, len(cases), own, narrays)
