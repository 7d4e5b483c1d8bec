#!/usr/bin/env python3
"""Timings of the AED detector (Darknet-21; the ``basic`` / ``taf`` / ``taf_bfm`` recipes) on one GPU, one JSON line each:

  forward        eval forward of the plan at batch 32, 256 x 320 x 10, and its share of the fp32 MFMA peak
  detect         forward + decode + NMS (with the host's list of detections)
  train          the train step at batch 64, replayed as a HIP graph like bench.py's
  stem           Focus + stem alone at batch 32 for (C, 64) and (4 | 8, 32): the fused kernel against Focus + convolution, same process

Device events around `n` back-to-back calls, `--runs` (>= 5) such regions after a warm-up; the value is the median, the spread
min .. max.  ``python tools/time_aed.py [--runs 7] [--skip-train]``
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from frlw_evd_amd import _lib  # noqa: E402
from frlw_evd_amd.detector import ACT_SILU, DetectorEngine, gemm_weight  # noqa: E402
from frlw_evd_amd.yolox.model import build_aed, recipe_state_dict  # noqa: E402

PEAK_FP32_MFMA = 157.3e12  # the figure README.md uses for the yolox forward


def regions(fn, runs, n, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / n)
    return out


def report(name, ms, **extra):
    row = {"what": name, "ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
           "runs": len(ms)}
    row.update(extra)
    print(json.dumps(row), flush=True)
    return row["ms_median"]


def stem_plan(lib, prec, Cin, H, W, w, bias, fused):
    """One plan of the stem alone: buffers 0 = input, 1 = output, 2 = the Focus image of the unfused pair."""
    det = lib.frlw_det_create()
    _lib.check(lib.frlw_det_set_precision(det, prec))
    Cout = w.shape[0]
    wm, npad = gemm_weight(w.cpu())
    op = wm.cuda().contiguous()
    keep = [op, bias]
    if prec == 1:
        img = torch.empty(lib.frlw_conv_split_operand_bytes(wm.shape[0], npad), dtype=torch.uint8, device="cuda")
        _lib.check(lib.frlw_conv_split_operand(op.data_ptr(), wm.shape[0], npad, img.data_ptr(), torch.cuda.current_stream().cuda_stream))
        keep.append(img)
        op = img
    if fused:
        rc = lib.frlw_det_add_focus_stem(det, 0, Cin, H, W, op.data_ptr(), bias.data_ptr(), Cout, 1, Cout, 0)
        if rc == _lib.FRLW_ERR_UNSUPPORTED:  # a shape the host function keeps on the unfused pair
            lib.frlw_det_destroy(det)
            return None, keep
        _lib.check(rc, "focus_stem")
    else:
        _lib.check(lib.frlw_det_add_focus(det, 0, Cin, H, W, 2), "focus")
        # the plan's own stem convolution (DetectorEngine._conv_raw): Focus image -> output, no image stride of its own
        # (dst_bs = 0), no residual (-1), SiLU, no sigmoid columns, no groups
        _lib.check(lib.frlw_det_add_conv(det, 2, 4 * Cin, 0, 4 * Cin, H // 2, W // 2, op.data_ptr(), bias.data_ptr(), Cout, npad, 3, 1,
                                         1, Cout, 0, 0, -1, 0, 0, ACT_SILU, 0, 0), "conv")
    return det, keep


def time_stem(lib, runs, Cin, Cout, B, precision):
    H, W = 256, 320
    prec = {"f32": 0, "bf16x3": 1}[precision]
    g = torch.Generator(device="cuda").manual_seed(Cin)
    x = torch.rand((B, Cin, H, W), generator=g, device="cuda")
    w = torch.randn((Cout, 4 * Cin, 3, 3), generator=g, device="cuda") * (2.0 / (36 * Cin)) ** 0.5
    bias = torch.randn((Cout,), generator=g, device="cuda") * 0.1
    y = [torch.empty((B, H // 2, W // 2, Cout), device="cuda") for _ in range(2)]
    f = torch.empty((B, H // 2, W // 2, 4 * Cin), device="cuda")
    scratch = torch.zeros(3 * (8 * 256 * 64 * 64 + 1024), device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {}
    for i, fused in enumerate((True, False)):
        det, keep = stem_plan(lib, prec, Cin, H, W, w, bias, fused)
        if det is None:
            print(json.dumps({"what": f"stem fused C={Cin} Cout={Cout} B={B} {precision}", "refused": "stays on Focus + convolution"}), flush=True)
            continue
        _lib.check(lib.frlw_det_set_scratch(det, 3, 8 * 256 * 64 * 64 + 1024))
        ptrs = (C.c_void_p * 4)(x.data_ptr(), y[i].data_ptr(), f.data_ptr(), scratch.data_ptr())
        ms = regions(lambda: _lib.check(lib.frlw_det_run(det, B, ptrs, 4, 0, -1, stream)), runs, 20)
        res[fused] = report(f"stem {'fused' if fused else 'focus+conv'} C={Cin} Cout={Cout} B={B} {precision}", ms)
        lib.frlw_det_destroy(det)
    if True not in res:
        return
    err = float((y[0] - y[1]).abs().max() / y[1].abs().max())
    print(json.dumps({"what": f"stem C={Cin} Cout={Cout} {precision}: fused / unfused", "ratio": round(res[True] / res[False], 4),
                      "max_rel_diff": err}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--skip-train", action="store_true")
    a = ap.parse_args()
    assert a.runs >= 5
    lib = _lib.load()
    print(json.dumps({"device": torch.cuda.get_device_name(0), "library": lib.frlw_version().decode()}), flush=True)
    for Cin, Cout in ((10, 64), (16, 64), (4, 64), (8, 64), (4, 32), (8, 32)):  # every kernel form of k_focus_stem_wide
        for precision in ("f32", "bf16x3"):
            time_stem(lib, a.runs, Cin, Cout, 32, precision)
    B = 32
    x = torch.rand(B, 10, 256, 320, device="cuda")
    for precision in ("f32", "bf16x3"):
        m = build_aed(10, 2)
        m.load_state_dict(recipe_state_dict(m, seed=1004))
        m.eval().cuda()
        eng = DetectorEngine(m, precision=precision)
        ms = regions(lambda: eng.raw_outputs(x), a.runs, 10)
        med = float(np.median(ms))
        fl = eng.flops_per_image * B
        report(f"forward B={B} 256x320x10 {precision}", ms, frames_per_s=round(B / med * 1e3, 1), gflop_per_image=round(eng.flops_per_image / 1e9, 3),
               tflops=round(fl / med / 1e9, 2), share_of_fp32_mfma_peak=round(fl / (med * 1e-3) / PEAK_FP32_MFMA, 4))
        ms = regions(lambda: eng.detect(x), a.runs, 10)
        report(f"detect (forward + decode + NMS) B={B} {precision}", ms, frames_per_s=round(B / float(np.median(ms)) * 1e3, 1))
    if not a.skip_train:
        from frlw_evd_amd.trainer import Trainer
        Bt = 64
        m = build_aed(10, 2)
        m.load_state_dict(recipe_state_dict(m, seed=1004))
        tr = Trainer(m.cuda(), global_batch=Bt, nodes=1, iters_per_epoch=100, graph=True)
        xt = torch.rand(Bt, 10, 256, 320, 1, 1, device="cuda")
        lab = torch.zeros(Bt, 80, 5, dtype=torch.float64, device="cuda")
        lab[:, 0] = torch.tensor([1, 100.0, 120.0, 40.0, 60.0])
        lab[:, 1] = torch.tensor([0, 200.0, 80.0, 30.0, 30.0])
        step = [0]

        def one():
            tr.train_step(xt, lab, step[0], sync=False)
            step[0] += 1
        ms = regions(one, a.runs, 5)
        report(f"train step B={Bt} 256x320x10 (graph replay)", ms, frames_per_s=round(Bt / float(np.median(ms)) * 1e3, 1))


if __name__ == "__main__":
    main()
