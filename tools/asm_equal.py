#!/usr/bin/env python3
"""Are two builds of one translation unit the same device code?  Compares gfx950 assembly listings function by function.

    hipcc <_build.HIPCC_FLAGS without -shared> -I include -I frlw-evd_amd/csrc --cuda-device-only -S csrc/taf_fast.hip -o new.s
    python tools/asm_equal.py parent.s new.s
    python tools/asm_equal.py parent.encoders.s,parent.partition.s new.encoders.s,new.partition.s,new.leaky.s

Either side may be several listings joined by commas (code that moved to another translation unit): they are read as one.

Lines that carry only file names, line numbers or the identity of the compilation (.file, .loc, .ident, the __hip_cuid_<hash of
the source> symbol) are dropped first.  Local labels carry the function's ordinal in the listing (.LBB12_3, .Lfunc_end12), which moves
when template kernels are instantiated in another order: functions are compared with the ordinal taken out.  Prints the number of
functions compared, the names of those that differ, whether the functions come in the same order, and the number of differing
lines in the whole listing, as it stands and as a bag of lines; exit status 1 if a function differs or is missing, if the bags
differ, or if lines differ while the order is the same."""
import collections
import difflib
import re
import sys


def load(paths):
    out = []
    for path in paths.split(","):
        with open(path) as f:
            out += [l.rstrip() for l in f if not re.match(r"\s*\.(file|loc|ident)\b", l) and "__hip_cuid_" not in l]
    return out


def functions(lines):
    out, cur = {}, None
    for l in lines:
        m = re.match(r"^(_Z\w+):", l)
        if m:
            cur = m.group(1)
            out[cur] = []
        if cur:
            out[cur].append(l)
        if l.startswith(".Lfunc_end") or (cur and l.startswith("\t.size\t" + cur + ",")):  # (.size: where a variable ends)
            cur = None
    return out


def unnumbered(body):
    # (the comment behind a label is padded to a column: with the ordinal out, so is the padding)
    return body and [re.sub(r":\s+;", ": ;", re.sub(r"(\.LBB|\bBB|\.Lfunc_end)\d+", r"\1", l)) for l in body]


def main():
    a, b = load(sys.argv[1]), load(sys.argv[2])
    fa, fb = functions(a), functions(b)
    differ = sorted(n for n in set(fa) | set(fb) if unnumbered(fa.get(n)) != unnumbered(fb.get(n)))
    lines = sum(1 for l in difflib.unified_diff(a, b, lineterm="", n=0) if l[0] in "+-" and not l.startswith(("+++", "---"))) if a != b else 0
    print(f"functions compared: {len(fa)} (only in the first: {len(set(fa) - set(fb))}, only in the second: {len(set(fb) - set(fa))})")
    print(f"functions that differ: {len(differ)}")
    for n in differ:
        print("   ", n)
    same_order = list(fa) == list(fb)
    print(f"functions in the same order: {'yes' if same_order else 'no'}")
    print(f"differing lines: {lines}")
    # what lies between the functions (kernel descriptors, metadata) moves with them: compared as a bag of lines
    bag = collections.Counter(unnumbered(a))
    bag.subtract(collections.Counter(unnumbered(b)))
    loose = sum(abs(v) for v in bag.values())
    print(f"differing lines, order ignored: {loose}")
    return 1 if differ or loose or (lines and same_order) else 0


if __name__ == "__main__":
    sys.exit(main())
