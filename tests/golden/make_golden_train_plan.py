#!/usr/bin/env python3
"""Records the six integer queries of the training operators (csrc/train_ops.hip) over a grid that crosses every branch of
their host arithmetic into train_plan.json: operand rows rounded to 16 in the bf16x3 arithmetic, columns padded to 32, the
parity-grouped data-gradient operand on and off, the weight-gradient split count at 1, between 2 and 64 and above 64 (the
group allowance) for the 64 x 64, 128 x 32, 128 x 64 and 128 x 128 tiles, bn_rows_per_wg at its floor, in between and at its
cap, and the scratch layout of the block entries on top of all of them.  Host arithmetic only: no GPU needed.

    FRLW_LIB_PATH=<libfrlw_evd.so of the commit whose arithmetic is the reference> python tests/golden/make_golden_train_plan.py

The library is the one frlw_evd_amd._lib loads, so FRLW_LIB_PATH selects it.  The fixture pins the queries across refactors
of that host code, so it is made from the build BEFORE such a change, never from the code under test
(tests/test_train_plan_cpu.py)."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from frlw_evd_amd import _lib  # noqa: E402

KS = [1, 3]
STRIDES = [1, 2]
CHANNELS = [4, 32, 36, 64, 128, 256, 512]
# (B, H, W) of the input; odd and even sides; with stride 1 and 2 the outputs run from (1, 4, 4) to (64, 160, 160)
SHAPES = [(1, 8, 8), (2, 9, 9), (2, 16, 16), (4, 17, 15), (8, 40, 40), (16, 40, 40), (16, 80, 80), (64, 81, 79), (64, 80, 80), (64, 160, 160)]


def out_dim(h, k, stride):
    return (h + 2 * ((k - 1) // 2) - k) // stride + 1


def queries():
    """{symbol: list of argument tuples}"""
    pairs = [(ci, co) for ci in CHANNELS for co in CHANNELS]
    outs = sorted({(b, out_dim(h, k, s), out_dim(w, k, s)) for b, h, w in SHAPES for k in KS for s in STRIDES})
    return {
        "frlw_conv_operand_floats": [(k * k * ci, co, p) for k in KS for ci, co in pairs for p in (0, 1)],
        "frlw_baseconv_weight_cache_floats": [(ci, co, k, p) for k in KS for ci, co in pairs for p in (0, 1)],
        "frlw_conv2d_dgrad_parity": [(k, s, h, w) for k in KS + [5] for s in STRIDES + [3] for _, h, w in SHAPES + [(1, 8, 9), (1, 9, 8)]],
        "frlw_conv2d_wgrad_scratch_floats": [(b, ho, wo, ci, co, k) for b, ho, wo in outs for ci, co in pairs for k in KS],
        "frlw_bn_scratch_doubles": [(b * ho * wo, c) for b, ho, wo in outs for c in CHANNELS],
        "frlw_baseconv_train_scratch_bytes": [(b, h, w, ci, co, k, s) for b, h, w in SHAPES for ci, co in pairs for k in KS for s in STRIDES],
    }


if __name__ == "__main__":
    lib = _lib.load()
    out = {name: {"args": [list(a) for a in args], "values": [int(getattr(lib, name)(*a)) for a in args]} for name, args in queries().items()}
    json.dump(out, open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "train_plan.json"), "w"), separators=(",", ":"))
    # which branches the grid reached (slots = partial tiles of the weight gradient: splits, plus group sums above 64 splits)
    slots = [v // (a[5] * a[5] * a[3] * a[4]) for a, v in zip(queries()["frlw_conv2d_wgrad_scratch_floats"], out["frlw_conv2d_wgrad_scratch_floats"]["values"])]
    ms = sorted({m for m, _ in queries()["frlw_bn_scratch_doubles"]})  # bn_rows_per_wg: floor of 32 below M = 33 * 1024, cap of 512 from M = 513 * 1024
    print(_lib.library_path())
    print({k: len(v["values"]) for k, v in out.items()})
    print("weight-gradient slots: 1:", slots.count(1), " 2..64:", sum(1 < s <= 64 for s in slots), " > 64:", sum(s > 64 for s in slots), " max:", max(slots))
    print("pixel counts M with 32 rows per statistics workgroup:", sum(m < 33792 for m in ms), " in between:", sum(33792 <= m < 525312 for m in ms),
          " 512:", sum(m >= 525312 for m in ms))
