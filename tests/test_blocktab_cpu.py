"""The block address table of kf_split_whole<true> (csrc/taf_blocktab.h: no HIP header, no HIP type) on the CPU:
tests/host/blocktab_check.cpp is built with the host C++ compiler under AddressSanitizer + UndefinedBehaviorSanitizer and run as a
program of its own.  It builds the table for random columns (zero-length, 1-record, short, block-sized, ~43-record, ~250-record and
65 535-record runs; address gaps up to beyond 2^28) and for the edges by hand, and compares the address of EVERY list position with the
plain L / D definition.  The GPU side is tests/test_split_gather_gpu.py."""
import os
import shutil
import subprocess

from frlw_evd_amd import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_cxx():
    for name in ("c++", "g++", "clang++"):
        exe = shutil.which(name)
        if exe:
            return exe
    return None


def test_every_position_of_random_columns_through_the_table_under_asan_and_ubsan(tmp_path):
    exe = _host_cxx()
    assert exe, "no host C++ compiler (c++, g++, clang++)"
    prog = str(tmp_path / "blocktab_check")
    cmd = [exe, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", _build.CSRC,
           os.path.join(ROOT, "tests", "host", "blocktab_check.cpp"), "-o", prog]
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
    assert " 0 failed" in r.stdout and "1554 columns" in r.stdout, r.stdout
    # the sweep is not vacuous: blocks with one boundary (the packed form) and blocks that fall back both occur in the thousands
    words = r.stdout.replace("(", " ").split()
    assert int(words[words.index("with") - 1]) > 10_000 and int(words[words.index("fallback),") - 1]) > 1_000, r.stdout
