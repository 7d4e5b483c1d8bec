"""The workgroup -> item mapping of csrc/xcd_map.h (no HIP header, no HIP type) on the CPU: tests/host/xcd_map_check.cpp is built
with the host C++ compiler under AddressSanitizer + UndefinedBehaviorSanitizer and walks every grid size from 1 to 8200 -- a
bijection of [0, n), consecutive items for the blocks of one XCD, eight ranges in order whose sizes differ by at most one,
chunk_of_block the same function -- and, built with -DFRLW_NO_XCD_REMAP, finds the identity (the A/B arm)."""
import os
import shutil
import subprocess

import pytest

from frlw_evd_amd import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_cxx():
    for name in ("c++", "g++", "clang++"):
        exe = shutil.which(name)
        if exe:
            return exe
    return None


@pytest.mark.parametrize("define", [None, "-DFRLW_NO_XCD_REMAP"], ids=["remap", "identity"])
def test_xcd_owned_index_over_every_grid_under_asan_and_ubsan(tmp_path, define):
    exe = _host_cxx()
    assert exe, "no host C++ compiler (c++, g++, clang++)"
    prog = str(tmp_path / "xcd_map_check")
    cmd = [exe, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", _build.CSRC,
           os.path.join(ROOT, "tests", "host", "xcd_map_check.cpp"), "-o", prog] + ([define] if define else [])
    # the sanitizer runtimes linked INTO the program (gcc's default is the shared ones, which insist on being the first library of
    # the process); clang links them statically anyway and does not know the two flags
    c = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True, timeout=300)
    if c.returncode != 0:
        c = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr[-4000:]
    r = subprocess.run([prog], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "grids 1 .. 8200 and 5 large ones," in r.stdout and " 0 failed" in r.stdout, r.stdout
