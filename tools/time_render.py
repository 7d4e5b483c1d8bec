#!/usr/bin/env python3
"""Time the renderer (csrc/render.hip through frlw_evd_amd/visualize.py) -> profiles/render_time.txt.

Two cases, TAF with 16 channels and 16 boxes a frame (8 ground truth, 8 detections):
  gen1: 64 frames, 304x240 sampled from the stored 256x320;
  gen4:  8 frames, 1280x720 sampled from the stored 512x640.
Per case: the fused launch alone (boxes already packed and on the device), ``visualize.render`` end to end (host packing and the
upload of the box records included), and the two-step route -- backgrounds, then the boxes in BGR mode -- that
``detect_recording.py --frames --seq_nms`` takes.  Median of 7 after one warm-up, host clock around synchronised work.  Beside
them the numpy restatement of the tests on one thread (one run).  Figures are reported, not gated.

    python tools/time_render.py [--out profiles/render_time.txt] [--no_numpy]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

CASES = (("gen1", 64, (240, 304), (256, 320)), ("gen4", 8, (720, 1280), (512, 640)))
CHANNELS, BOXES, REPEATS = 16, 16, 7


def make_case(n, sensor, stored, seed):
    rng = np.random.default_rng(seed)
    vol = (rng.random((n, CHANNELS) + stored) ** 4 * 255).astype(np.uint8)       # mostly dark, as TAF volumes are

    def rows(k):
        r = np.zeros((k, 8), np.float64)
        r[:, 1], r[:, 2] = rng.uniform(0, sensor[1] - 40, k), rng.uniform(16, sensor[0] - 40, k)
        r[:, 3], r[:, 4] = rng.uniform(10, sensor[1] / 3, k), rng.uniform(10, sensor[0] / 3, k)
        r[:, 5], r[:, 6] = rng.integers(0, 2, k), rng.uniform(0, 1, k)
        return r
    return vol, [rows(BOXES // 2) for _ in range(n)], [rows(BOXES - BOXES // 2) for _ in range(n)]


def median_ms(fn):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no_numpy", action="store_true")
    args = ap.parse_args()
    from frlw_evd_amd import _lib, visualize
    lib = _lib.load()
    lines = [f"renderer timings on {torch.cuda.get_device_name(0)}: TAF, {CHANNELS} channels, {BOXES} boxes a frame; "
             f"median (min .. max) of {REPEATS}, ms, host clock around synchronised work"]
    for name, n, sensor, stored in CASES:
        vol, gt, dt = make_case(n, sensor, stored, 5)
        src = torch.from_numpy(vol).cuda()
        packed = [visualize.pack_boxes(g, d) for g, d in zip(gt, dt)]
        offsets = np.zeros(n + 1, np.int32)
        offsets[1:] = np.cumsum([len(p) for p in packed])
        boxes_d = torch.from_numpy(np.concatenate(packed).view(np.uint8).reshape(-1, 32)).cuda()
        out = torch.empty((n,) + sensor + (3,), dtype=torch.uint8, device="cuda")
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def launch():
            _lib.check(lib.frlw_render_frames(C.c_void_p(src.data_ptr()), n, CHANNELS, stored[0], stored[1], 0, sensor[0], sensor[1],
                                              C.c_void_p(boxes_d.data_ptr()), offsets.ctypes.data_as(C.POINTER(C.c_int32)),
                                              C.c_void_p(out.data_ptr()), stream))

        def fused():
            return visualize.render(src, "TAF", sensor, gt, dt)

        def two_step():
            return visualize.render(visualize.render(src, "TAF", sensor), "BGR", sensor, gt, dt)
        launch()
        assert torch.equal(out, fused()) and torch.equal(out, two_step())
        read, written = vol.nbytes, out.numel()
        lines.append(f"{name}: {n} frames {sensor[1]}x{sensor[0]} from stored {stored[1]}x{stored[0]} "
                     f"({read / 1e6:.1f} MB read, {written / 1e6:.1f} MB written)")
        for label, fn in (("fused launch alone", launch), ("visualize.render, fused", fused),
                          ("visualize.render, backgrounds then BGR overlay", two_step)):
            med, lo, hi = median_ms(fn)
            extra = f"  {(read + written) / med / 1e6:.0f} GB/s" if fn is launch else ""
            lines.append(f"  {label:<48s} {med:9.3f} ({lo:.3f} .. {hi:.3f}){extra}")
        if not args.no_numpy:
            import render_restated as rr
            torch.set_num_threads(1)
            t0 = time.perf_counter()
            want = rr.render(vol, "TAF", sensor, gt, dt)
            ms = (time.perf_counter() - t0) * 1e3
            assert np.array_equal(want, out.cpu().numpy()), "the GPU image differs from the restatement"
            lines.append(f"  {'numpy restatement, one thread (one run)':<48s} {ms:9.1f}   (byte-equal to the GPU image)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
