#!/usr/bin/env python3
"""Writes tests/golden/tvl1.npz from tests/tvl1_restated.py (the float64 and the float32 restatement of the Dual TV-L1 solver) on the
seeded inputs of tests/tvl1_data.py -- no GPU, no third-party solver.  ``python tests/golden/make_golden_tvl1.py``.

Per case the file keeps what a GPU test would otherwise recompute and the bound it is held to:

  short_<case>_bound      fixed short schedules (epsilon = 0): max |float32 - float64| over the flow
  smooth_<case>_flow      default parameters, the float64 flow (at most 64 x 80 x 2)
  smooth_<case>_iters     its (levels, warps) inner-iteration counts -- the float32 restatement runs the same, asserted here
  smooth_<case>_bound     max |float32 - float64| over the flow
  noisy_density64 / 32    default parameters on the noisy pair: the density of tvl1_data.NOISY_BOXES in both restatements

and asserts its own conditions: every default-parameter smooth case keeps the last error of every (level, warp) at least
MARGIN away from the threshold in both dtypes (else a summation order could change an iteration count: such a case is replaced,
not excused), and no density of the noisy case lies within four times the float32 - float64 difference of a bucket edge."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import tvl1_data as D  # noqa: E402
import tvl1_restated as R  # noqa: E402

MARGIN = 0.05


def margin(r):
    return float(np.abs(r["errors"] / r["eps"][:, None] - 1.0).min())


def density(flow, box):
    """motion_level_statistics_gt.py:130 on an integer box: the float32 magnitudes, summed in float64."""
    _, x0, x1, y0, y1 = (int(v) for v in box)
    f = flow[y0:y1, x0:x1].astype(np.float32)
    return float(np.sqrt(f[..., 0] ** 2 + f[..., 1] ** 2).astype(np.float64).sum() / ((y1 - y0) * (x1 - x0) + 1e-8))


def main():
    from frlw_evd_amd.settings import MOTION_LEVEL_EDGES
    out, failed = {}, []
    for name, (pair, prm) in D.short_cases().items():
        r64, r32 = R.tvl1(pair[0], pair[1], np.float64, **prm), R.tvl1(pair[0], pair[1], np.float32, **prm)
        out[f"short_{name}_bound"] = np.abs(r32["flow"].astype(np.float64) - r64["flow"]).max()
        print("short", name, r64["levels"], "max |f32 - f64|", out[f"short_{name}_bound"], "largest flow", np.abs(r64["flow"]).max())
    for name, case in D.SMOOTH.items():
        a, b = D.blob_pair(*case)
        shift = case[2]
        r64, r32 = R.tvl1(a, b, np.float64), R.tvl1(a, b, np.float32)
        print("smooth", name, "margins", margin(r64), margin(r32), "epe", R.interior_epe(r64["flow"], shift), R.interior_epe(r32["flow"], shift),
              "iters", r64["iters"].tolist())
        assert np.array_equal(r64["iters"], r32["iters"]), f"{name}: the float32 restatement runs other iteration counts"
        if margin(r64) < MARGIN or margin(r32) < MARGIN:
            failed.append(f"{name}: an error within 5 % of the threshold ({margin(r64):.4f}, {margin(r32):.4f}): replace the case")
        assert R.interior_epe(r64["flow"], shift) <= 0.1
        out[f"smooth_{name}_flow"] = r64["flow"]
        out[f"smooth_{name}_iters"] = r64["iters"]
        out[f"smooth_{name}_bound"] = np.abs(r32["flow"].astype(np.float64) - r64["flow"]).max()
        print("   max |f32 - f64|", out[f"smooth_{name}_bound"])
    a, b = D.surface_pair(*D.NOISY)
    r64, r32 = R.tvl1(a, b, np.float64), R.tvl1(a, b, np.float32)
    d64 = np.asarray([density(r64["flow"], bx) for bx in D.NOISY_BOXES])
    d32 = np.asarray([density(r32["flow"], bx) for bx in D.NOISY_BOXES])
    print("noisy densities", d64.tolist(), d32.tolist(), "pointwise max |f32 - f64|", np.abs(r32["flow"] - r64["flow"]).max())
    edges = np.asarray(MOTION_LEVEL_EDGES["gen1"])
    for v64, v32 in zip(d64, d32):
        assert np.all(np.abs(edges - v64) > 4 * abs(v32 - v64)), "a density within the bound of a bucket edge: choose another box"
    out["noisy_density64"], out["noisy_density32"] = d64, d32
    np.savez_compressed(os.path.join(HERE, "tvl1.npz"), **out)
    print("wrote tvl1.npz", os.path.getsize(os.path.join(HERE, "tvl1.npz")), "bytes")
    if failed:   # the file is written so that the other tests can run; tests/test_tvl1_cpu.py fails on the same condition
        raise SystemExit("\n".join(failed))


if __name__ == "__main__":
    main()
