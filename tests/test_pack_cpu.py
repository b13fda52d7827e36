"""Host weight packers (csrc/pack.cpp) under AddressSanitizer + UBSan: tools/pack_check.cpp is a
stand-alone program over pack.cpp, built here with the host compiler and run directly (no
GPU, nothing loaded into Python).  It checks every packer against the inverse of its layout."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "wespeaker_hubert_amd", "csrc")


def _compilers():
    """(compiler, extra flags), preferring a statically linked sanitizer runtime: the program then
    runs the same whatever else the environment loads into it."""
    rocm = "/opt/rocm/llvm/bin/clang++"
    out = [(rocm, [])] if os.path.exists(rocm) else []  # clang links its runtime statically
    for c in ("g++", "c++"):
        if shutil.which(c):
            out += [(c, ["-static-libasan", "-static-libubsan"]), (c, [])]
    if shutil.which("clang++"):
        out.append(("clang++", []))
    return out


def test_pack_check_under_sanitizers(tmp_path):
    cxxs = _compilers()
    assert cxxs, "no host C++ compiler found"
    exe = str(tmp_path / "pack_check")
    errors = []
    for cxx, extra in cxxs:  # the first whose sanitizer runtimes link
        cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
               "-fno-sanitize-recover=all", *extra, "-I", CSRC, os.path.join(REPO, "tools", "pack_check.cpp"),
               os.path.join(CSRC, "pack.cpp"), "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode == 0:
            break
        errors.append(f"{cxx} {extra}: {r.stderr[-2000:]}")
    else:
        pytest.fail("pack_check does not build:\n" + "\n".join(errors))
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "pack_check: ok" in r.stdout
