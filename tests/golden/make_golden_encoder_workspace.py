#!/usr/bin/env python3
"""Records frlw_encoder_workspace_bytes over the (events, frame) grid of tests/host/enc_plan_check.cpp into
encoder_workspace_bytes.json: tiny, ragged, GEN1 and 1 Mpx frames, the tile limit met exactly (16384 x 64), tall frames whose tiles
are widened to 7 and to 8 to stay under it, and frames refused at width 8.  Host arithmetic only: no GPU needed.

    python tests/golden/make_golden_encoder_workspace.py <libfrlw_evd.so of the commit whose layout is the reference>

The fixture pins what callers allocate (tests/test_workspace_query_cpu.py); regenerate it only when the layout is meant to change."""
import ctypes
import json
import os
import sys

EVENTS = [0, 1, 1023, 1024, 65_536, 1_000_000, 10_000_000, 2 ** 32 - 1]
FRAMES = [[1, 1], [8, 12], [20, 300], [240, 304], [720, 1280], [512, 512], [513, 8], [16384, 64], [4000, 4000], [64 * 240, 304],
          [8800, 100], [8800, 200]]


def grid():
    return [(n, h, w) for n in EVENTS for h, w in FRAMES]


if __name__ == "__main__":
    lib = ctypes.CDLL(sys.argv[1])
    f = lib.frlw_encoder_workspace_bytes
    f.restype = ctypes.c_size_t
    f.argtypes = [ctypes.c_int64, ctypes.c_int, ctypes.c_int]
    out = {"events": EVENTS, "frames_h_w": FRAMES, "order": "events (outermost), frames", "bytes": [int(f(*g)) for g in grid()]}
    json.dump(out, open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "encoder_workspace_bytes.json"), "w"))
    print(len(out["bytes"]), "values,", sum(1 for b in out["bytes"] if b == 0), "refused")
