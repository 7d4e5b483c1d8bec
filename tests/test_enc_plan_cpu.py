"""The general path's host planner (csrc/enc_plan.h: no HIP header, no HIP type) on the CPU: tests/host/enc_plan_check.cpp is built
with the host C++ compiler under AddressSanitizer + UndefinedBehaviorSanitizer and walks the grid of
tests/golden/encoder_workspace_bytes.json crossed with every knob of the general path -- the rules of the plan, of the scatter's
LDS and of the tile grid that the kernels rely on (see the program)."""
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


def test_planner_rules_hold_over_the_grid_under_asan_and_ubsan(tmp_path, golden_dir):
    exe = _host_cxx()
    assert exe, "no host C++ compiler (c++, g++, clang++)"
    prog = str(tmp_path / "enc_plan_check")
    cmd = [exe, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", _build.INCLUDE,
           "-I", _build.CSRC, os.path.join(ROOT, "tests", "host", "enc_plan_check.cpp"), "-o", prog]
    # the sanitizer runtimes linked INTO the program (gcc's default is the shared ones, which insist on being the first library of
    # the process); clang links them statically anyway and does not know the two flags
    c = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True, timeout=300)
    if c.returncode != 0:
        c = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr[-4000:]
    r = subprocess.run([prog, os.path.join(golden_dir, "encoder_workspace_bytes.json")], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    # 9 event counts (one negative) x 14 frames (two not positive) x 20 knob settings = 2520 calls
    assert " 0 failed" in r.stdout and "1280 planned, 1240 refused, 112 widened to 7, 120 widened to 8" in r.stdout, r.stdout
