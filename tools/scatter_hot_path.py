#!/usr/bin/env python3
"""Instruction counts of kf_scatter_cm's rank loop (phase A) in the headline instance, read from the compiler's assembly.

    python tools/scatter_hot_path.py [--instance kf_scatter_cmILb0ELb0ELb1ELi20ELi0E] [--asm taf_fast.s] [--all]

Compiles csrc/taf_fast.hip to gfx950 assembly with the build's flags (no GPU needed), finds the instance and looks at the code
between consecutive returning LDS atomics (`ds_add_rtn_u32`: one per ranked batch of 64 events).  The loop is unrolled and
every batch is a chain of basic blocks, most of which only invalid events enter (the 64-bit division of the aliased pixel, the
error word), so the text between two atomics says little.  The tool follows the control flow instead: from behind every
atomic it takes the shortest path, in instructions, to the next atomic it can reach that still requests the events four
batches ahead and, towards a fast block, votes (hot_path below) -- the path of a full batch of valid events, which skips every
block that exists for the others (a heuristic, but one that does not need to know what a branch tests).  Along that path it
counts VALU, SALU, slow-rate VALU (quarter-rate integer multiplies, 64-bit shifts, f64), `v_writelane_b32` (SGPR spills) and branches, and says whether a full `s_waitcnt lgkmcnt(0)` stands on it.  Paths are grouped by
the kind of atomic they start from and end at: one under an exec-mask save (`slow`, the block with lane conditions) or not
(`fast`).  A developer aid, not a test: the counts move with the compiler."""
import argparse
import collections
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SLOW = re.compile(r"^(v_mul_hi_u32|v_mul_lo_u32|v_mul_hi_i32|v_mul_lo_i32|v_mad_u64_u32|v_mad_i64_i32|v_lshlrev_b64|v_lshrrev_b64|v_ashrrev_i64|v_\w+_f64)(_e32|_e64)?$")
BRANCH = re.compile(r"^s_(cbranch|branch)")
NOT_VALU = ("v_writelane", "v_readlane", "v_readfirstlane")
NOT_SALU = ("s_waitcnt", "s_nop", "s_barrier")


def assembly(path):
    from frlw_evd_amd import _build  # the one place that knows the flags
    flags = [f for f in _build.HIPCC_FLAGS if f not in ("-shared", "-fPIC")] + ["-I", _build.INCLUDE, "-I", _build.CSRC]
    subprocess.check_call([_build.hipcc()] + flags + ["-S", "--cuda-device-only", os.path.join(_build.CSRC, "taf_fast.hip"), "-o", path])


def body(lines, instance):
    """(instructions, label -> index of the instruction behind it) of the first function whose name contains `instance`"""
    start = next((i for i, l in enumerate(lines) if re.match(r"^_Z\w*" + re.escape(instance) + r"\w*:", l)), None)
    if start is None:
        raise SystemExit(f"no function matching {instance}")
    ops, labels = [], {}
    for l in lines[start + 1:]:
        t = l.split(";")[0].strip()
        if not t:
            continue
        if t.endswith(":"):
            labels[t[:-1]] = len(ops)
            continue
        if t.startswith("."):
            continue
        ops.append(t)
        if t.startswith("s_endpgm"):
            break
    return ops, labels


def successors(ops, labels, i):
    name = ops[i].split()[0]
    if name.startswith("s_endpgm"):
        return []
    if name == "s_branch":
        return [labels[ops[i].split()[1]]]
    if name.startswith("s_cbranch"):
        return [i + 1, labels[ops[i].split()[1]]]
    return [i + 1]


def hot_path(ops, labels, start, goals, fast_goal):
    """The shortest path a FULL batch of valid events can take from `start` to an atomic.  The shortest path of the graph alone
    is not it: it skips what the compiler guards with wave-uniform state it keeps in SGPRs.  So two things every such batch does
    must lie on the path: the request of the events four batches ahead (a global load, where any path has one) and, towards an
    atomic outside an exec-mask save, the vote (at least three vector compares).  Breadth first over (instruction, load seen,
    compares seen up to 3)."""
    first = (start, False, 0)
    prev, todo, ends = {first: None}, collections.deque([first]), []
    while todo:
        st = todo.popleft()
        i, load, cmps = st
        if i in goals:
            ends.append(st)  # (in order of path length)
            continue
        if i >= len(ops):
            continue
        load = load or ops[i].startswith("global_load")
        cmps = min(3, cmps + ops[i].startswith("v_cmp"))
        for n in successors(ops, labels, i):
            nst = (n, load, cmps)
            if nst not in prev:
                prev[nst] = st
                todo.append(nst)
    if not ends:
        return None, None
    if any(e[1] for e in ends):
        ends = [e for e in ends if e[1]]
    ok = [e for e in ends if not fast_goal(e[0]) or e[2] >= 3]
    end = (ok or ends)[0]
    path, st = [], prev[end]
    while st is not None:
        path.append(st[0])
        st = prev[st]
    return path[::-1], end[0]


def count(seg):
    names = [t.split()[0] for t in seg]
    return {"valu": sum(n.startswith("v_") and not n.startswith(NOT_VALU) for n in names),
            "salu": sum(n.startswith("s_") and not BRANCH.match(n) and not n.startswith(NOT_SALU) for n in names),
            "slow": sum(bool(SLOW.match(n)) for n in names),
            "writelane": sum(n.startswith("v_writelane") for n in names),
            "branch": sum(bool(BRANCH.match(n)) for n in names),
            "wait0": any(t.startswith("s_waitcnt") and "lgkmcnt(0)" in t for t in seg)}


def under_saveexec(ops, labels, at):
    """the atomic sits in a block entered through an exec-mask save (walk back to the block's label)"""
    starts = set(labels.values())
    i = at
    while i > 0 and i not in starts:
        i -= 1
        if "saveexec" in ops[i]:
            return True
    return any("saveexec" in ops[k] for k in range(max(0, i - 2), i))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instance", default="kf_scatter_cmILb0ELb0ELb1ELi20ELi0E")
    ap.add_argument("--asm", help="read this assembly file instead of compiling")
    ap.add_argument("--all", action="store_true", help="print every path, not only the medians")
    a = ap.parse_args()
    if a.asm:
        path = a.asm
    else:
        path = os.path.join(tempfile.mkdtemp(prefix="scatter_hot_"), "taf_fast.s")
        assembly(path)
    ops, labels = body(open(path).read().splitlines(), a.instance)
    at = [i for i, t in enumerate(ops) if t.startswith("ds_add_rtn_u32")]
    if len(at) < 2:
        raise SystemExit(f"{len(at)} returning LDS atomics in {a.instance}")
    kind = {i: "slow" if under_saveexec(ops, labels, i) else "fast" for i in at}
    print(f"{a.instance}: {len(ops)} instructions, {len(at)} returning LDS atomics ({sum(k == 'fast' for k in kind.values())} outside an exec-mask save)")
    keys = ("valu", "salu", "slow", "writelane", "branch")
    groups = collections.defaultdict(list)
    for i in at:
        p, goal = hot_path(ops, labels, i + 1, set(at), lambda g: kind[g] == "fast")
        if p is None:
            continue  # the last batch
        c = count([ops[k] for k in p])
        groups[f"{kind[i]} -> {kind[goal]}"].append(c)
        if a.all:
            print(f"  atomic at {i:5d} ({kind[i]}) -> {goal:5d} ({kind[goal]}): " + " ".join(f"{n} {c[n]:3d}" for n in keys) + f"  lgkmcnt(0) {'yes' if c['wait0'] else 'no'}")
    for name, group in sorted(groups.items()):
        med = " / ".join(str(int(statistics.median(c[n] for c in group))) for n in keys)
        print(f"  {len(group):2d} paths {name}: median VALU / SALU / slow-rate VALU / v_writelane / branches = {med}; "
              f"a full lgkmcnt(0) wait on {sum(c['wait0'] for c in group)} of them")


if __name__ == "__main__":
    main()
