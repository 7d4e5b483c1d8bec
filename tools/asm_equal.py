#!/usr/bin/env python3
"""Are two builds of one translation unit the same device code?  Compares gfx950 assembly listings function by function.

    hipcc <_build.HIPCC_FLAGS without -shared> -I include -I frlw-evd_amd/csrc --cuda-device-only -S csrc/taf_fast.hip -o new.s
    python tools/asm_equal.py parent.s new.s

Lines that carry only file names, line numbers or the identity of the compilation (.file, .loc, .ident, the __hip_cuid_<hash of
the source> symbol) are dropped first.  Prints the number of functions compared, the names of those that differ and the number of
differing lines in the whole listing; exit status 1 if anything differs."""
import difflib
import re
import sys


def load(path):
    with open(path) as f:
        return [l.rstrip() for l in f if not re.match(r"\s*\.(file|loc|ident)\b", l) and "__hip_cuid_" not in l]


def functions(lines):
    out, cur = {}, None
    for l in lines:
        m = re.match(r"^(_Z\w+):", l)
        if m:
            cur = m.group(1)
            out[cur] = []
        if cur:
            out[cur].append(l)
        if l.startswith(".Lfunc_end"):
            cur = None
    return out


def main():
    a, b = load(sys.argv[1]), load(sys.argv[2])
    fa, fb = functions(a), functions(b)
    differ = sorted(n for n in set(fa) | set(fb) if fa.get(n) != fb.get(n))
    lines = sum(1 for l in difflib.unified_diff(a, b, lineterm="", n=0) if l[0] in "+-" and not l.startswith(("+++", "---"))) if a != b else 0
    print(f"functions compared: {len(fa)} (only in the first: {len(set(fa) - set(fb))}, only in the second: {len(set(fb) - set(fa))})")
    print(f"functions that differ: {len(differ)}")
    for n in differ:
        print("   ", n)
    print(f"differing lines: {lines}")
    return 1 if lines else 0


if __name__ == "__main__":
    sys.exit(main())
