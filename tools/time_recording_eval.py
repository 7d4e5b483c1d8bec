#!/usr/bin/env python3
"""Wall time of scoring a checkpoint on a test split, from the recordings to the evaluator's lists, on a synthetic GEN1-sized
split (``--sequences`` recordings of ``--events`` events over ``--seconds`` s, 304x240, a label every 50 ms behind 0.6 s; the
``yolox_taf_bfm`` detector at 256x320, K = 4, recipe weights, batches of ``--batch``):

* the file route: ``generate.generate_taf`` (encode, copy to the host, one bins4 and one bins8 file per label) into a scratch
  directory, then ``Loader(propheseeTafDataset)`` over the files -> detector -> evaluator, as ``test.py --data_path`` runs it;
* the recording route: ``RecordingLoader`` -> detector -> evaluator, as ``test.py --raw_dir --representation taf`` runs it;
* the hand-off alone on one batch (B = 32, C = 16, 240x304 -> 256x320): ``transforms.hand_off`` (one launch) against the route it
  replaces (channel slice + ``.contiguous()``, ``resize_nearest``, reshape, ``transform_images``).

Wall time (host clock) around whole, synchronised runs; 1 warm-up + ``--runs`` runs, median and spread.  Both routes must return
the same lists.  The work runs in a child process under a time limit; the parent never opens the GPU.

``python tools/time_recording_eval.py [--runs 7] [--out profiles/recording_eval_time.txt]``
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SENSOR, IMG, BINS = (240, 304), [256, 320], 4
LIMIT_S = 1100
BBOX_DTYPE = [("t", "<u8"), ("x", "<f4"), ("y", "<f4"), ("w", "<f4"), ("h", "<f4"), ("class_id", "u1"), ("class_confidence", "<f4"),
              ("track_id", "<u4")]


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


def write_split(root, sequences, events, seconds):
    import numpy as np
    from frlw_evd_amd import dat_io, synth
    raw, lab = os.path.join(root, "raw", "test"), os.path.join(root, "label", "test")
    os.makedirs(raw)
    os.makedirs(lab)
    labels = 0
    for s in range(sequences):
        rec = synth.to_dat8(synth.synth_events(700 + s, events, SENSOR[1], SENSOR[0], seconds * 1_000_000, hotspot=True, t_offset=1_000))
        dat_io.write_dat(os.path.join(raw, f"seq{s}_td.dat"), rec, *SENSOR)
        times = np.arange(600_000, seconds * 1_000_000, 50_000)
        boxes = np.zeros(2 * len(times), dtype=BBOX_DTYPE)
        boxes["t"] = np.repeat(times, 2)
        boxes["x"], boxes["y"], boxes["w"], boxes["h"], boxes["class_confidence"] = 50, 60, 40, 30, 1.0
        boxes["class_id"] = np.tile([0, 1], len(times))
        np.save(os.path.join(lab, f"seq{s}_bbox.npy"), boxes)
        labels += len(times)
    return os.path.dirname(raw), os.path.dirname(lab), labels


def child(a):
    import numpy as np
    import torch
    from frlw_evd_amd import _lib, event_representation as er, generate, transforms
    from frlw_evd_amd.dataset import Loader, propheseeTafDataset
    from frlw_evd_amd.evaluator import evaluator
    from frlw_evd_amd.recording_dataset import RecordingLoader
    from frlw_evd_amd.yolox import build_yolox
    from frlw_evd_amd.yolox.model import recipe_state_dict
    work = tempfile.mkdtemp(prefix="recording_eval_")
    try:
        raw, lab, labels = write_split(work, a.sequences, a.events, a.seconds)
        print(json.dumps({"device": torch.cuda.get_device_name(0), "library": _lib.load().frlw_version().decode(), "sequences": a.sequences,
                          "events_per_sequence": a.events, "labels": labels, "batch": a.batch}), flush=True)
        net = build_yolox(2 * BINS, 2, stem="bfm")
        net.load_state_dict(recipe_state_dict(net, seed=41))
        net = net.cuda().eval()

        def evaluate(loader):
            ev = evaluator(loader.object_classes if hasattr(loader, "object_classes") else loader.dataset.object_classes, a.batch, 10000,
                           304, 240, IMG[1], IMG[0], "gen1")
            for imgs, targets, names, stamps in loader:
                with torch.no_grad():
                    ev = net(imgs, targets, names, stamps, evaluator=ev)
            return ev.evaluate()

        def files_generate():
            target = os.path.join(work, "processed")
            shutil.rmtree(target, ignore_errors=True)
            generate.generate_taf(raw, lab, target, "gen1")
            return os.path.join(target, "taf")

        def files_evaluate(data_dir):
            ds = propheseeTafDataset(lab, data_dir, "gen1", IMG, IMG, 10000, BINS, "test", False, False)
            return evaluate(Loader(ds, a.batch, 8, False, "cuda", shuffle=False))

        def recording_route():
            return evaluate(RecordingLoader(lab, raw, "taf", "gen1", IMG, IMG, BINS, "test", a.batch, "cuda"))

        results = {}
        data_dir = files_generate()
        for name, fn in (("file route: generate_taf + Loader over the files + detector", lambda: files_evaluate(files_generate())),
                         ("file route, the command alone: generate_taf", files_generate),
                         ("file route, evaluation alone: Loader over the files + detector", lambda: files_evaluate(data_dir)),
                         ("recording route: RecordingLoader + detector", recording_route)):
            out, med, lo, hi = timed(fn, a.runs)
            results[name] = (out, med)
            print(json.dumps({"what": name, "s_median": round(med, 4), "s_min": round(lo, 4), "s_max": round(hi, 4), "runs": a.runs,
                              "labels_per_s": round(labels / med, 1)}), flush=True)
        (fa, ta), (ra, tr) = results["file route: generate_taf + Loader over the files + detector"], results["recording route: RecordingLoader + detector"]
        for key in ("gt_boxes_list", "dt_boxes_list"):
            assert len(fa[key]) == len(ra[key]) and all(x.tobytes() == y.tobytes() for x, y in zip(fa[key], ra[key])), f"the routes disagree on {key}"
        print(json.dumps({"what": "recording route / file route", "frames": len(fa["dt_boxes_list"]),
                          "detections": int(sum(len(d) for d in fa["dt_boxes_list"])), "identical": True, "time_ratio": round(tr / ta, 4)}), flush=True)

        # the hand-off alone: one batch out of one chain's snapshots
        B, K, C = 32, 8, 16
        snaps = torch.randint(0, 256, (B, K, 2) + SENSOR, dtype=torch.uint8, device="cuda")

        def one_launch():
            return transforms.hand_off([snaps[b] for b in range(B)], C, SENSOR, IMG)

        def four_launches():
            vol = snaps.reshape(B, 2 * K, *SENSOR)[:, :C].contiguous()
            vol = er.resize_nearest(vol.reshape(B * C, *SENSOR), IMG).reshape(B, C, *IMG)
            return transforms.transform_images(vol, [transforms.SampleParams()] * B)

        assert torch.equal(one_launch(), four_launches())
        bytes_moved = B * C * (SENSOR[0] * SENSOR[1] + 4 * IMG[0] * IMG[1])
        for name, fn in (("hand-off: transforms.hand_off, one launch", one_launch), ("hand-off: slice + resize_nearest + transform_images", four_launches)):
            def many(fn=fn):
                for _ in range(50):
                    out = fn()
                return out
            _, med, lo, hi = timed(many, a.runs)
            print(json.dumps({"what": name, "us_median": round(med / 50 * 1e6, 2), "us_min": round(lo / 50 * 1e6, 2), "us_max": round(hi / 50 * 1e6, 2),
                              "runs": a.runs, "calls_per_run": 50, "GB_per_s_of_the_one_launch_bytes": round(bytes_moved / (med / 50) / 1e9, 1)}), flush=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--sequences", type=int, default=3)
    ap.add_argument("--events", type=int, default=3_000_000)
    ap.add_argument("--seconds", type=int, default=6)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.child:
        child(a)
        return 0
    opts = ["--runs", str(a.runs), "--sequences", str(a.sequences), "--events", str(a.events), "--seconds", str(a.seconds), "--batch", str(a.batch)]
    import threading
    lines = []
    with tempfile.TemporaryFile("w+") as err:   # the rows are passed on as they come: a run takes minutes
        p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child"] + opts, stdout=subprocess.PIPE, stderr=err, text=True)
        watchdog = threading.Timer(LIMIT_S, p.kill)
        watchdog.start()
        try:
            for line in p.stdout:
                lines.append(line)
                sys.stdout.write(line)
                sys.stdout.flush()
            rc = p.wait()
        finally:
            watchdog.cancel()
        if rc != 0:
            err.seek(0)
            sys.stderr.write(err.read()[-3000:] + f"\nthe child ended with {rc} (killed after {LIMIT_S} s if negative)\n")
            return 1
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"# tools/time_recording_eval.py {' '.join(opts)} (MI355X; wall time of whole runs, synchronised)\n" + "".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
