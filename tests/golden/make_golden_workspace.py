#!/usr/bin/env python3
"""Records frlw_taf_batch_workspace_bytes over a grid that crosses every branch of the fast path's plan (direct / tile
bins, ordinary / big chunks, refused shapes) into workspace_bytes.json.  Host arithmetic only: no GPU needed.

    python tests/golden/make_golden_workspace.py <libfrlw_evd.so of the commit whose layout is the reference>

The fixture pins the size query across refactors of the layout code, so it is made from the build BEFORE such a change,
never from the code under test (tests/test_workspace_query_cpu.py)."""
import ctypes
import json
import os
import sys

EVENTS = [0, 1_000, 100_000, 1_000_000, 3_000_000, 6_000_000, 10_000_000, 64_000_000]
SEQUENCES = [1, 5, 8, 40, 64]
FRAMES = [[97, 131], [240, 304], [480, 640], [720, 1280]]
WINDOWS = [1, 977, 10_000, 250_000]


def grid():
    return [(n, s, h, w, win) for n in EVENTS for s in SEQUENCES for h, w in FRAMES for win in WINDOWS]


if __name__ == "__main__":
    lib = ctypes.CDLL(sys.argv[1])
    f = lib.frlw_taf_batch_workspace_bytes
    f.restype = ctypes.c_size_t
    f.argtypes = [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64]
    out = {"events": EVENTS, "sequences": SEQUENCES, "frames_h_w": FRAMES, "windows_us": WINDOWS,
           "order": "events (outermost), sequences, frames, windows", "bytes": [int(f(*g)) for g in grid()]}
    json.dump(out, open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "workspace_bytes.json"), "w"))
    print(len(out["bytes"]), "values,", sum(1 for b in out["bytes"] if b == 0), "refused")
