#!/usr/bin/env python3
"""Timings of the native Dual TV-L1 solver (``motion.tvl1_flow``, csrc/tvl1.hip) with default parameters, one JSON line each:

  64 synthetic time-surface-like pairs at 240 x 304 and 8 at 720 x 1280 (tests/tvl1_data.py: sparse moving edges, 2 % impulse cells,
  large zero areas), already in HBM: the time per call, the inner iterations actually run (summed over levels and warps: the
  slowest pair, which sets the number of launches, and the mean) and the kernel launches the call enqueued;
  the float32 numpy restatement (tests/tvl1_restated.py) on ONE CPU thread for one pair of each size: in full at 240 x 304; at
  720 x 1280 a fixed schedule of 5 levels x 3 iterations is timed and the full run is EXTRAPOLATED from the iterations the device
  ran per level (said so in the line).

Host clock around work that ends in a device synchronisation; one warm-up, then the median of ``--runs`` (7) with min .. max.
There is no earlier number to compare with: the numbers are reported, not gated.

``python tools/time_tvl1.py [--runs 7] [--out profiles/tvl1_time.txt]``
"""
import argparse
import json
import os
import sys
import time

for var in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):   # the restatement's numpy on one thread
    os.environ[var] = "1"

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = {"304x240": ((240, 304), 64), "1280x720": ((720, 1280), 8)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tvl1_time.txt"))
    args = ap.parse_args()
    import torch
    import tvl1_data
    import tvl1_restated
    from frlw_evd_amd import _lib, motion
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    lines = [f"# tools/time_tvl1.py --runs {args.runs} (MI355X; host clock around synchronised work, 1 warm-up, median of {args.runs}); reported, not gated",
             json.dumps({"device": torch.cuda.get_device_name(0), "library": _lib.load().frlw_version().decode()})]

    def say(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    for key, (shape, n) in SIZES.items():
        H, W = shape
        host = tvl1_data.timing_pairs(n, H, W)
        pairs = torch.from_numpy(host).cuda()
        before = motion.tvl1_counts()
        flows, iters = motion.tvl1_flow(pairs, return_iters=True)   # the warm-up
        torch.cuda.synchronize()
        after = motion.tvl1_counts()
        per_pair = iters.sum(dim=(1, 2)).cpu().numpy()
        ms = []
        for _ in range(args.runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            motion.tvl1_flow(pairs)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        med = float(np.median(ms))
        say({"what": f"tvl1_flow {key}: {n} pairs in HBM, default parameters", "ms_median": round(med, 3), "ms_min": round(min(ms), 3),
             "ms_max": round(max(ms), 3), "runs": len(ms), "ms_per_pair": round(med / n, 3), "calls": after[0] - before[0],
             "kernel_launches": after[1] - before[1], "inner_iterations_slowest_pair": int(per_pair.max()),
             "inner_iterations_mean": round(float(per_pair.mean()), 1), "inner_iterations_cap": 5 * 5 * 300,
             "mean_flow_magnitude_px": round(float(flows.norm(dim=-1).mean()), 4)})
        one = host[0]
        if H * W <= 240 * 304:
            t0 = time.perf_counter()
            r = tvl1_restated.tvl1(one[0], one[1], np.float32)
            sec = time.perf_counter() - t0
            say({"what": f"numpy float32 restatement {key}: one pair, one CPU thread, in full", "s": round(sec, 2),
                 "inner_iterations": int(r["iters"].sum()), "device_iterations_same_pair": int(per_pair[0]),
                 "restatement_x_pairs / device": round(sec * 1e3 * n / med, 1)})
        else:
            short = dict(epsilon=0.0, nscales=5, warps=1, outer=1, inner=3)
            t0 = time.perf_counter()
            r = tvl1_restated.tvl1(one[0], one[1], np.float32, **short)
            sec = time.perf_counter() - t0
            cells = np.asarray([h * w for h, w in r["levels"]], np.float64)
            per_cell_iter = sec / float((cells * 3).sum())   # warp, median and gradient of the short run are charged to its iterations
            full = float((iters[0].sum(dim=1).cpu().numpy() * cells).sum()) * per_cell_iter
            say({"what": f"numpy float32 restatement {key}: one pair, one CPU thread, 5 levels x 3 iterations timed", "s": round(sec, 2),
                 "EXTRAPOLATED_s_for_the_iterations_the_device_ran": round(full, 1), "device_iterations_same_pair": int(per_pair[0]),
                 "extrapolated_restatement_x_pairs / device": round(full * 1e3 * n / med, 1)})
        del pairs, flows
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
