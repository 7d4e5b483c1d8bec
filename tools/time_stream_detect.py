#!/usr/bin/env python3
"""Frames per second of detection on a raw recording: ``stream.StreamDetector`` (one encode_taf_chain per detector batch) against
the per-frame route (one encode_taf_dat call per frame with the state carried, then the same hand-off and the same detector
batches), on one synthetic GEN1-sized recording: 304x240, ``--frames`` frames every 50 ms, about 20 000 events per 10 ms window,
the ``yolox`` detector at 256x320 with recipe weights.  Also the encode half alone (no detector) of both routes.

Wall time around whole runs, synchronised; 1 warm-up + ``--runs`` runs, median and spread.  Both routes must return the same
boxes.  The work runs in a child process under a time limit; the parent never opens the GPU.

``python tools/time_stream_detect.py [--runs 7] [--frames 64] [--out profiles/stream_detect_time.txt]``
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SENSOR, IMG, K, WINDOW, PERIOD, T_BEGIN, PER_WINDOW, BATCH = (240, 304), (256, 320), 8, 10_000, 50_000, 1_000_000, 20_000, 32
LIMIT_S = 420


def timed(fn, runs):
    import numpy as np
    import torch
    secs = []
    for _ in range(runs + 1):   # the first run is the warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
    secs = secs[1:]
    return out, float(np.median(secs)), min(secs), max(secs)


def child(runs, frames):
    import numpy as np
    import torch
    from frlw_evd_amd import _lib, event_representation as er, synth
    from frlw_evd_amd.stream import StreamDetector, to_bbox_records
    from frlw_evd_amd.yolox import build_yolox
    from frlw_evd_amd.yolox.model import recipe_state_dict
    print(json.dumps({"device": torch.cuda.get_device_name(0), "library": _lib.load().frlw_version().decode(), "frames": frames,
                      "events": frames * (PERIOD // WINDOW) * PER_WINDOW}), flush=True)
    bins = PERIOD // WINDOW
    rec = synth.to_dat8(synth.synth_events(600, frames * bins * PER_WINDOW, SENSOR[1], SENSOR[0], frames * PERIOD, hotspot=True,
                                           t_offset=T_BEGIN))
    dat = torch.from_numpy(rec.view(np.uint8).reshape(-1, 8).copy()).cuda()
    net = build_yolox(2 * K, 2)
    net.load_state_dict(recipe_state_dict(net, seed=1004))
    net = net.cuda().eval()
    det = StreamDetector(net, SENSOR, IMG, dataset="gen1", volume_bins=K, input_bins=K, period_us=PERIOD, window_us=WINDOW,
                         frames_per_call=BATCH)
    t_end = T_BEGIN + frames * PERIOD
    times = det.frame_times(T_BEGIN, t_end)
    cuts = np.searchsorted(rec["t"], [T_BEGIN] + times, side="left")

    def per_frame_volumes():
        state = torch.full(SENSOR + (2, K), -6000.0, device="cuda")
        return [er.encode_taf_dat(dat[cuts[j]:cuts[j + 1]], SENSOR, state, ts - PERIOD, WINDOW, bins, K)[0] for j, ts in enumerate(times)]

    def per_frame():
        vols, out = per_frame_volumes(), []
        for g in range(0, len(times), BATCH):
            with torch.no_grad():
                outputs = net.detect(det.hand_off(torch.stack(vols[g:g + BATCH]), SENSOR))
            out += det.boxes(outputs, times[g:g + BATCH])
        return to_bbox_records(out, times)

    def chain_volumes():
        state = torch.full(SENSOR + (2, K), -6000.0, device="cuda")
        return [er.encode_taf_chain(dat[cuts[g]:cuts[min(g + BATCH, len(times))]], SENSOR, state, times[g] - PERIOD, WINDOW,
                                    [bins] * len(times[g:g + BATCH]), K) for g in range(0, len(times), BATCH)]

    rows = {}
    for name, fn in (("stream: StreamDetector.run", lambda: det.run(dat, T_BEGIN, t_end)), ("per frame: encode_taf_dat per frame, same batches", per_frame),
                     ("encode only, one encode_taf_chain per batch", chain_volumes), ("encode only, encode_taf_dat per frame", per_frame_volumes)):
        out, med, lo, hi = timed(fn, runs)
        rows[name] = (out, med)
        print(json.dumps({"what": name, "s_median": round(med, 5), "s_min": round(lo, 5), "s_max": round(hi, 5), "runs": runs,
                          "frames_per_s": round(frames / med, 1)}), flush=True)
    (a, ta), (b, tb) = rows["stream: StreamDetector.run"], rows["per frame: encode_taf_dat per frame, same batches"]
    assert a.tobytes() == b.tobytes(), "the two routes disagree"
    print(json.dumps({"what": "stream / per frame", "boxes": int(len(a)), "identical": True, "time_ratio": round(ta / tb, 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.child:
        child(a.runs, a.frames)
        return 0
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--runs", str(a.runs), "--frames", str(a.frames)],
                           capture_output=True, text=True, timeout=LIMIT_S)
    except subprocess.TimeoutExpired:
        print(f"no result inside {LIMIT_S} s", file=sys.stderr)
        return 1
    sys.stdout.write(p.stdout)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-3000:])
        return 1
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"# tools/time_stream_detect.py --runs {a.runs} --frames {a.frames} (MI355X; wall time of whole runs, synchronised)\n" + p.stdout)
    return 0


if __name__ == "__main__":
    sys.exit(main())
