#!/usr/bin/env python3
"""Timings of the device half of the motion-level evaluation against the numpy statements it replaces, same box, same run, one
JSON line each, at 304x240 and at 1280x720:

  pairs    64 overlapping label windows of one file (50 000 events each at 304x240, 200 000 at 1280x720):
           ``motion.time_surface_pairs`` (the file already in HBM; the call ends in a synchronisation, it reads the stamp ranges)
           against 64 calls of ``motion.time_surface_numpy`` on the host records, and -- once, for one window -- against the
           per-event loop the reference runs under numba, here without it
  density  64 flows x 16 boxes: ``motion.box_flow_density`` on flows already in HBM, and including their upload, against the
           per-box numpy statement of motion_level_statistics_gt.py:130

Host clock around work that ends in a device synchronisation; one warm-up, then the median of ``--runs`` (7) with min .. max.
The numbers are reported, not gated.

``python tools/time_motion_level.py [--runs 7] [--out profiles/motion_level_time.txt]``
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B = 64
SIZES = {"304x240": ((240, 304), 50_000), "1280x720": ((720, 1280), 200_000)}   # frame, events per window


def timed(fn, runs, sync=None):
    fn()
    out = []
    for _ in range(runs):
        if sync:
            sync()
        t0 = time.perf_counter()
        fn()
        if sync:
            sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def report(lines, what, ms, **extra):
    row = {"what": what, "ms_median": round(float(np.median(ms)), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3), "runs": len(ms)}
    row.update(extra)
    lines.append(json.dumps(row))
    print(lines[-1], flush=True)
    return float(np.median(ms))


def per_event_loop(rec, shape):
    """generate_timesurface as the reference writes it, event by event (no numba here)."""
    w = rec["_"].astype(np.uint32)
    events = np.stack([w & 16383, (w >> 14) & 16383, rec["t"]], axis=1).astype(float)
    events = events[(events[:, 0] < shape[1]) & (events[:, 1] < shape[0])]
    volume1, volume2 = np.zeros(shape), np.zeros(shape)
    end_stamp, start_stamp = events[:, 2].max(), events[:, 2].min()
    for event in events:
        if event[2] < end_stamp - 50000:
            volume1[int(event[1])][int(event[0])] = event[2]
        volume2[int(event[1])][int(event[0])] = event[2]
    volume1 = (volume1 - start_stamp) / (end_stamp - 50000 - start_stamp) * 255
    volume2 = (volume2 - start_stamp - 50000) / (end_stamp - 50000 - start_stamp) * 255
    return np.stack([np.where(volume1 < 0, 0, volume1).astype(np.uint8), np.where(volume2 < 0, 0, volume2).astype(np.uint8)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_level_time.txt"))
    args = ap.parse_args()
    import torch
    from frlw_evd_amd import _lib, motion, synth
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    sync = torch.cuda.synchronize
    lines = [f"# tools/time_motion_level.py --runs {args.runs} (MI355X; host clock around synchronised work, 1 warm-up, median of {args.runs})",
             json.dumps({"device": torch.cuda.get_device_name(0), "library": _lib.load().frlw_version().decode()})]
    for key, (shape, per) in SIZES.items():
        H, W = shape
        # ---- pairs: windows of `per` records that start every (n - per) / 63 records of one 500 ms-per-window stream
        n = 8 * per
        rec = synth.to_dat8(synth.synth_events(9100 + H, n, W, H, 8 * 500_000, hotspot=True, t_offset=1000))
        ranges = [(i * (n - per) // (B - 1), i * (n - per) // (B - 1) + per) for i in range(B)]
        dat = torch.from_numpy(rec.view(np.uint8).reshape(-1, 8).copy()).cuda()
        got = motion.time_surface_pairs(dat, ranges, shape)[0].cpu().numpy()
        assert all(np.array_equal(got[i], motion.time_surface_numpy(rec[lo:hi], shape)) for i, (lo, hi) in enumerate(ranges[:3]))
        dev = report(lines, f"pairs {key}: time_surface_pairs, {B} windows x {per} events, file in HBM", timed(lambda: motion.time_surface_pairs(dat, ranges, shape), args.runs, sync))
        host = report(lines, f"pairs {key}: time_surface_numpy, {B} windows x {per} events",
                      timed(lambda: [motion.time_surface_numpy(rec[lo:hi], shape) for lo, hi in ranges], args.runs))
        lo, hi = ranges[0]
        t0 = time.perf_counter()
        loop = per_event_loop(rec[lo:hi], shape)
        loop_ms = (time.perf_counter() - t0) * 1e3
        assert np.array_equal(loop, got[0])
        lines.append(json.dumps({"what": f"pairs {key}: numpy / device", "ratio": round(host / dev, 1),
                                 "per_event_loop_ms_one_window_one_run": round(loop_ms, 1), "loop_x64 / device": round(64 * loop_ms / dev, 1)}))
        print(lines[-1], flush=True)
        del dat
        # ---- density: 16 boxes on each of 64 flows
        rng = np.random.default_rng(9200 + H)
        flows = rng.standard_normal((B, H, W, 2)).astype(np.float32)
        xy = np.stack([rng.uniform(0, W - 60, B * 16), rng.uniform(0, H - 60, B * 16)], axis=1)
        rows = np.zeros((B * 16, 8))
        rows[:, 1:3], rows[:, 3:5] = xy, rng.uniform(10, min(H, W) / 2, (B * 16, 2))
        rows, corners = motion.clamp_boxes(rows, shape)
        index = np.repeat(np.arange(B), 16)

        def numpy_side():
            out = []
            for r, c, f in zip(rows, corners, index):
                x1, y1, x2, y2 = c
                flow = flows[f]
                out.append(np.sum(np.sqrt(flow[int(y1):int(y2), int(x1):int(x2), 0] ** 2 + flow[int(y1):int(y2), int(x1):int(x2), 1] ** 2))
                           / (int(r[4]) * int(r[3]) + 1e-8))
            return np.asarray(out, np.float64)
        fd = torch.from_numpy(flows).cuda()
        assert np.allclose(motion.box_flow_density(fd, rows, index, corners), numpy_side(), rtol=1e-5, atol=0)
        dev = report(lines, f"density {key}: box_flow_density, {B} flows x 16 boxes, flows in HBM", timed(lambda: motion.box_flow_density(fd, rows, index, corners), args.runs, sync))
        up = report(lines, f"density {key}: upload of the {B} flows + box_flow_density",
                    timed(lambda: motion.box_flow_density(torch.from_numpy(flows).cuda(), rows, index, corners), args.runs, sync),
                    flow_bytes=int(flows.nbytes))
        host = report(lines, f"density {key}: per-box numpy statement, {B} flows x 16 boxes", timed(numpy_side, args.runs))
        lines.append(json.dumps({"what": f"density {key}: numpy / device", "ratio_in_hbm": round(host / dev, 1), "ratio_with_upload": round(host / up, 1)}))
        print(lines[-1], flush=True)
        del fd
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
