"""The cell mean of kf_taf_walk without the division (csrc/taf_mean.h: no HIP header) on the CPU: tests/host/walk_mean_check.cpp is
built with the host C++ compiler at -O2 -ffp-contract=off and run as a program of its own.  For every count n of the reciprocal
table (0 ... 63) it compares mean_by_recip(sum, (float)n, 1.0f / (float)n) BITWISE against sum / ((float)n + 1e-8f):

  edges     sum = +0 and -0; -n and its two f32 neighbours (a count of 0 only ever meets sum = +-0: it has no neighbours to take)
  stride    every f32 multiple of 2^-24 in [-n, 0] -- what the walk's sequential sums can be -- with the odd stride 61 through the
            bit patterns
  binades   the 4096 values on either side of every power of two up to n
  random    10^6 seeded values per n that are NOT multiples of 2^-24: the formula does not rest on that property

The program's --full mode takes every f32 in [-n, -2^-24]: profiles/walk_mean_sweep.txt.  The GPU side is tests/test_walk_mean_gpu.py."""
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


def test_mean_by_recip_equals_the_division_bit_for_bit(tmp_path):
    exe = _host_cxx()
    assert exe, "no host C++ compiler (c++, g++, clang++)"
    prog = str(tmp_path / "walk_mean_check")
    c = subprocess.run([exe, "-std=c++17", "-O2", "-ffp-contract=off", "-pthread", "-I", _build.CSRC,
                        os.path.join(ROOT, "tests", "host", "walk_mean_check.cpp"), "-o", prog], capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr[-4000:]
    r = subprocess.run([prog], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    # a mismatch names its set, n, the sum and both quotients on stderr
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    sets = {ln.split()[0]: (int(ln.split()[1]), int(ln.split()[3])) for ln in r.stdout.splitlines() if "comparisons " in ln and not ln.startswith("walk_mean")}
    assert set(sets) == {"edges", "stride", "binades", "random"}, r.stdout
    assert all(bad == 0 for _, bad in sets.values()), r.stdout
    # the sets are not vacuous
    assert sets["edges"][0] == 2 * 64 + 3 * 63
    assert sets["stride"][0] > 10_000_000 and sets["binades"][0] > 10_000_000 and sets["random"][0] == 63 * 1_000_000
