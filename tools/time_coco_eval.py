#!/usr/bin/env python3
"""Times the COCO scorer on a synthetic split of 50 000 windows x 2 classes (1-10 ground truths, <= 100 detections per
window): the kernels alone (device events around frlw_coco_eval on packed device arrays), evaluate_detection's wall
time (packing, copies and the kernels included), and the literal CPU restatement (tests/coco_literal.py) on 2 000
windows of the same input, scaled by 25.

    python tools/time_coco_eval.py [--images 50000] [--literal-images 2000] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=50_000)
    ap.add_argument("--literal-images", type=int, default=2_000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_coco_eval needs a GPU"
    import coco_literal as lit
    from test_coco_eval_gpu import split

    from frlw_evd_amd import coco_eval
    gts, dts = split(args.images, 5, max_dt=100, max_gt=10, files=500)
    n_gt, n_dt = sum(map(len, gts)), sum(map(len, dts))
    p = coco_eval.pack(gts, dts, 2)
    coco_eval.coco_eval_packed(p, 2)  # warm-up: code objects, allocator
    # kernels only: the device arrays stay put, device events around the call
    import ctypes as C

    from frlw_evd_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    d = {k: torch.from_numpy(np.ascontiguousarray(p[k])).to(dev) for k in
         ("gt_box", "gt_area", "gt_cls", "gt_off", "dt_box", "dt_area", "dt_score", "dt_cls", "dt_off")}
    thr, rec = torch.from_numpy(coco_eval.IOU_THRS).to(dev), torch.from_numpy(coco_eval.REC_THRS).to(dev)
    nb = int(lib.frlw_coco_workspace_bytes(p["n_img"], len(p["gt_area"]), len(p["dt_area"]), 2))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    prec = torch.empty((10, 101, 2, 4, 3), dtype=torch.float64, device=dev)
    recl = torch.empty((10, 2, 4, 3), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def call():
        _lib.check(lib.frlw_coco_eval(d["gt_box"].data_ptr(), d["gt_area"].data_ptr(), d["gt_cls"].data_ptr(),
                                      d["gt_off"].data_ptr(), len(p["gt_area"]), d["dt_box"].data_ptr(), d["dt_area"].data_ptr(),
                                      d["dt_score"].data_ptr(), d["dt_cls"].data_ptr(), d["dt_off"].data_ptr(), len(p["dt_area"]),
                                      p["n_img"], 2, thr.data_ptr(), rec.data_ptr(), ws.data_ptr(), C.c_int64(nb),
                                      prec.data_ptr(), recl.data_ptr(), stream), "frlw_coco_eval")
    call()
    torch.cuda.synchronize()
    kern = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        kern.append(a.elapsed_time(b))
    wall = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stats = coco_eval.evaluate_detection(gts, dts)
        wall.append(1e3 * (time.perf_counter() - t0))
    pack_ms = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        coco_eval.pack(gts, dts, 2)
        pack_ms.append(1e3 * (time.perf_counter() - t0))
    # the literal restatement on the first windows of the same split, scaled to the full split
    sub_g, sub_d, n = [], [], 0
    for g, dd in zip(gts, dts):
        if n >= args.literal_images:
            break
        sub_g.append(g)
        sub_d.append(dd)
        n += len(np.unique(g[:, 0]))
    t0 = time.perf_counter()
    lit.literal_eval(sub_g, sub_d, 2)
    lit_s = time.perf_counter() - t0
    print(json.dumps({"images": p["n_img"], "ground_truths": n_gt, "detections": n_dt,
                      "kernel_ms_median": round(float(np.median(kern)), 3), "kernel_ms": [round(x, 3) for x in kern],
                      "evaluate_detection_ms_median": round(float(np.median(wall)), 1), "pack_ms_median": round(float(np.median(pack_ms)), 1),
                      "literal_images": n, "literal_s": round(lit_s, 2),
                      "literal_s_scaled": round(lit_s * p["n_img"] / n, 1), "AP": stats[0],
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
