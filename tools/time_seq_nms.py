#!/usr/bin/env python3
"""What Seq-NMS costs: ``seq_nms.seq_nms`` (pack, upload, the two launches of ``frlw_seq_nms``, download) on

  * one recording of 1 200 frames with about 6 boxes a frame (a GEN1-like minute at 20 Hz),
  * 64 such recordings in one call,

in both ``isolated`` modes; the plain restatement (tests/seqnms_restated.py) of the one recording on one CPU thread, for scale; and
``StreamDetector.run`` frames per second with ``seq_nms`` off and on, on the recording of tools/time_stream_detect.py.

Host clock around synchronised work (the call ends in a download), 1 warm-up + ``--runs`` runs, median and spread.  All reported,
nothing gated.  The work runs in a child process under a time limit; the parent never opens the GPU.

``python tools/time_seq_nms.py [--runs 7] [--frames 64] [--out profiles/seq_nms_time.txt]``
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

LIMIT_S = 540
MINUTE_FRAMES = 1200


def _minute(seed):
    """1 200 frames: tracks of 2 to 15 s that come and go (about five alive at a time, 5 % of their boxes dropped, a near-duplicate
    on every fifth) and one false positive every other frame."""
    import numpy as np
    rng = np.random.default_rng([9100, seed])
    frames = [[] for _ in range(MINUTE_FRAMES)]
    for _ in range(5):
        t = int(rng.integers(0, 100))
        while t < MINUTE_FRAMES:
            n = int(rng.integers(40, 300))
            w, h = rng.uniform(20, 70, 2)
            x, y = rng.uniform(0, 304 - w), rng.uniform(0, 240 - h)
            vx, vy = rng.uniform(-1.5, 1.5, 2)
            cls, base = int(rng.integers(0, 2)), rng.uniform(0.3, 0.95)
            for f in range(t, min(MINUTE_FRAMES, t + n)):
                x, y = x + vx, y + vy
                if rng.uniform() < 0.05:
                    continue
                j = rng.uniform(-1.5, 1.5, 4)
                box = [x + j[0], y + j[1], x + w + j[2], y + h + j[3]]
                frames[f].append(box + [float(np.clip(base + rng.uniform(-0.15, 0.15), 0.02, 1.0)), cls])
                if rng.uniform() < 0.2:
                    d = rng.uniform(-4, 4, 4)
                    frames[f].append([box[0] + d[0], box[1] + d[1], box[2] + d[2], box[3] + d[3], float(rng.uniform(0.02, 0.3)), cls])
            t += n + int(rng.integers(5, 60))
    for f in range(MINUTE_FRAMES):
        if rng.uniform() < 0.5:
            w, h = rng.uniform(10, 60, 2)
            x, y = rng.uniform(0, 304 - w), rng.uniform(0, 240 - h)
            frames[f].append([x, y, x + w, y + h, float(rng.uniform(0.02, 0.9)), int(rng.integers(0, 2))])
    out = []
    for fr in frames:
        a = np.asarray(fr, dtype=np.float64).reshape(-1, 6)
        a[:, :4] = a[:, :4].astype(np.float32)
        out.append(a)
    return out


def child(runs, frames):
    import numpy as np
    import torch
    import seqnms_restated
    import time_stream_detect as tsd
    from frlw_evd_amd import _lib, seq_nms as sn, synth
    from frlw_evd_amd.stream import StreamDetector
    from frlw_evd_amd.yolox import build_yolox
    from frlw_evd_amd.yolox.model import recipe_state_dict
    print(json.dumps({"device": torch.cuda.get_device_name(0), "library": _lib.load().frlw_version().decode()}), flush=True)
    videos = [_minute(k) for k in range(64)]
    print(json.dumps({"what": "one recording", "frames": MINUTE_FRAMES, "boxes": int(sum(len(f) for f in videos[0])),
                      "boxes_per_frame": round(sum(len(f) for f in videos[0]) / MINUTE_FRAMES, 2)}), flush=True)
    for isolated in ("stop", "skip"):
        for name, arg in (("1 recording", [videos[0]]), ("64 recordings", videos)):   # without the per-frame Python of pack / unpack
            packed = sn.pack(arg)
            opts = sn._options(0.5, 0.3, "avg", isolated, 65536)
            _, med, lo, hi = tsd.timed(lambda: sn.run_packed(*packed, *opts), runs)
            print(json.dumps({"what": f"run_packed {isolated}: {name} (upload, two launches, download)", "s_median": round(med, 5),
                              "s_min": round(lo, 5), "s_max": round(hi, 5), "runs": runs}), flush=True)
        for name, arg in (("1 recording", videos[0]), ("64 recordings, one call", videos)):
            out, med, lo, hi = tsd.timed(lambda: sn.seq_nms(arg, isolated=isolated), runs)
            first = out[0] if name.startswith("64") else out
            print(json.dumps({"what": f"seq_nms {isolated}: {name}", "s_median": round(med, 5), "s_min": round(lo, 5), "s_max": round(hi, 5),
                              "runs": runs, "sequences_first_recording": int(max(int(q.max()) for _, q, _ in first if len(q)))}), flush=True)
        torch.set_num_threads(1)
        t0 = time.perf_counter()
        res, selections, _ = seqnms_restated.seq_nms(videos[0], isolated=isolated)
        cpu = time.perf_counter() - t0
        got = sn.seq_nms(videos[0], isolated=isolated)
        same = all((a[0] == b[0]).all() and (a[1] == b[1]).all() and (a[2] == b[2]).all() for a, b in zip(got, res))
        print(json.dumps({"what": f"restatement {isolated}: 1 recording, one CPU thread, 1 run", "s": round(cpu, 3), "sequences": len(selections),
                          "gpu_identical": bool(same)}), flush=True)
    # the detector route, with and without
    bins = tsd.PERIOD // tsd.WINDOW
    rec = synth.to_dat8(synth.synth_events(600, frames * bins * tsd.PER_WINDOW, tsd.SENSOR[1], tsd.SENSOR[0], frames * tsd.PERIOD, hotspot=True,
                                           t_offset=tsd.T_BEGIN))
    dat = torch.from_numpy(rec.view(np.uint8).reshape(-1, 8).copy()).cuda()
    net = build_yolox(2 * tsd.K, 2)
    net.load_state_dict(recipe_state_dict(net, seed=1004))
    net = net.cuda().eval()
    t_end = tsd.T_BEGIN + frames * tsd.PERIOD
    for name, opt in (("off", None), ("stop", {"isolated": "stop"}), ("skip", {"isolated": "skip"})):
        det = StreamDetector(net, tsd.SENSOR, tsd.IMG, dataset="gen1", volume_bins=tsd.K, input_bins=tsd.K, period_us=tsd.PERIOD,
                             window_us=tsd.WINDOW, frames_per_call=tsd.BATCH, seq_nms=opt)
        out, med, lo, hi = tsd.timed(lambda: det.run(dat, tsd.T_BEGIN, t_end), runs)
        print(json.dumps({"what": f"StreamDetector.run, seq_nms {name}", "frames": frames, "boxes": int(len(out)), "sequences": int(det.sequences),
                          "s_median": round(med, 5), "s_min": round(lo, 5), "s_max": round(hi, 5), "frames_per_s": round(frames / med, 1)}),
              flush=True)


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
            f.write(f"# tools/time_seq_nms.py --runs {a.runs} --frames {a.frames} (MI355X; host clock around synchronised work)\n" + p.stdout)
    return 0


if __name__ == "__main__":
    sys.exit(main())
