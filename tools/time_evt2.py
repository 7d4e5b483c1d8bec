#!/usr/bin/env python3
"""Times the EVT 2.0 and EVT 2.1 decodes (frlw_evd_amd.raw_io: frlw_evt2_count + frlw_evt2_emit) beside the EVT 3.0 decode and writes
profiles/evt2_time.txt.

One 1280 x 720 stream of events, the one tools/time_evt3.py uses for its mix (a segment made by ``synth.synth_burst_events``,
repeated), written in each of the three encodings: the EVT 3.0 words are that tool's; the EVT 2.0 / 2.1 words of a repetition are
the segment's words with every EVT_TIME_HIGH raised by the repetition's offset, so t keeps rising without a clock wrap (a wrap adds
2^34 us there and would not fit a DAT record).  Each stream is decoded with the words already in device memory, and again with the
upload from host memory inside the timed region.  Median of 7, HIP events around synchronised work.  Beside each time: events per
second, the bytes the decode moves (the words are read three times, the records written once) per second, and the rate of a
device-to-device copy that moves the same number of bytes, measured on the same device in the same process.  The CPU figures are
the plain Python restatements of the tests on one thread.  Reported, not gated.

Every encoding is measured in a child process of its own under a time limit; the first one that fails ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

REPEATS = 7
SIZE = (720, 1280)
NAMES = {"EVT2": "EVT 2.0 (32-bit words)", "EVT21": "EVT 2.1 (64-bit words, up to 32 events a word)", "EVT3": "EVT 3.0 (16-bit words)"}


def timed(fn, torch):
    ms = []
    for _ in range(REPEATS + 1):              # the first run warms up
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms[1:])


def stream_of(encoding, n_words_evt3):
    """-> (words of the whole stream, words of one segment, repetitions)."""
    from frlw_evd_amd import raw_io, synth
    seg_events = max(10_000, min(7_000_000, n_words_evt3 // 14))
    rec = synth.to_dat8(synth.synth_burst_events(5, seg_events, SIZE[1], SIZE[0], seg_events // 50))
    seg3 = raw_io.encode_evt3(rec)
    reps = max(1, -(-n_words_evt3 // len(seg3)))
    if encoding == "EVT3":
        return np.tile(seg3, reps), seg3, reps
    seg = {"EVT2": raw_io.encode_evt2, "EVT21": raw_io.encode_evt21}[encoding](rec)
    at = 28 if encoding == "EVT2" else 60
    is_high = (seg >> seg.dtype.type(at)) == 0x8
    step = (int(rec["t"].max()) >> 6) + 1                     # EVT_TIME_HIGH units per repetition
    assert reps * step < 1 << 26
    words = np.tile(seg, reps)
    offsets = (np.arange(reps, dtype=seg.dtype) * seg.dtype.type(step)) << seg.dtype.type(at - 28)
    words.reshape(reps, len(seg))[:, is_high] += offsets[:, None]
    return words, seg, reps


def measure(encoding, n_words_evt3):
    """One encoding, in this process: -> a dict of figures."""
    import torch
    from frlw_evd_amd import raw_io
    words, seg, reps = stream_of(encoding, n_words_evt3)
    count = raw_io.evt3_count if encoding == "EVT3" else (lambda w, s: raw_io.evt2_count(w, s, encoding=encoding))
    emit = raw_io.evt3_emit if encoding == "EVT3" else (lambda w, s, p, o, n: raw_io.evt2_emit(w, s, p, o, n, encoding=encoding))
    signed = {2: np.int16, 4: np.int32, 8: np.int64}[words.dtype.itemsize]
    host = torch.from_numpy(words.view(signed))
    dev = host.cuda()
    counters, _, _ = count(dev, SIZE)
    n = int(counters.events)
    out = torch.empty((n, 8), dtype=torch.uint8, device="cuda")

    def decode(w=dev):
        c, _, plan = count(w, SIZE)
        status = emit(w, SIZE, plan, out, n)
        assert status == 0 and int(c.events) == n

    moved = 3 * words.nbytes + 8 * n
    src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    t_dev = timed(decode, torch)
    t_up = timed(lambda: decode(host.cuda()), torch)
    t_copy = timed(lambda: dst.copy_(src), torch)

    import evt2_restated
    import evt3_restated
    sample = seg[:200_000]
    t0 = time.perf_counter()
    if encoding == "EVT3":
        evt3_restated.decode(sample, SIZE[1], SIZE[0])
    else:
        evt2_restated.decode(sample, SIZE[1], SIZE[0], encoding)
    cpu = len(sample) / (time.perf_counter() - t0)
    return {"encoding": encoding, "device": torch.cuda.get_device_name(0), "geometry": raw_io.geometry(encoding), "words": len(words),
            "word_bytes": words.dtype.itemsize, "events": n, "repetitions": reps, "unsorted": int(counters.unsorted),
            "time_loops": int(counters.time_loops), "out_of_frame": int(counters.out_of_frame), "ms_device": t_dev, "ms_upload": t_up,
            "ms_copy": t_copy, "moved": moved, "cpu_words_per_s": cpu, "cpu_sample": len(sample)}


def lines_of(r):
    return [NAMES[r["encoding"]] + "   chunk / lane piece: {0} / {1} words".format(*r["geometry"]),
            "  words {0:,} ({1:,} bytes)  events {2:,}  ({3:.2f} events / word; unsorted {4}, time_loops {5}, out_of_frame {6})".format(
                r["words"], r["words"] * r["word_bytes"], r["events"], r["events"] / r["words"], r["unsorted"], r["time_loops"], r["out_of_frame"]),
            "  count + emit, words in device memory: {0:8.3f} ms  {1:7.2f} Gevents/s  {2:7.2f} Gwords/s  {3:7.1f} GB/s moved (3 x words read, records written)".format(
                r["ms_device"], r["events"] / r["ms_device"] / 1e6, r["words"] / r["ms_device"] / 1e6, r["moved"] / r["ms_device"] / 1e6),
            "  count + emit with the upload:         {0:8.3f} ms  {1:7.2f} Gevents/s".format(r["ms_upload"], r["events"] / r["ms_upload"] / 1e6),
            "  device-to-device copy moving as many bytes ({0:,} read + {0:,} written): {1:8.3f} ms  {2:7.1f} GB/s".format(
                r["moved"] // 2, r["ms_copy"], r["moved"] / r["ms_copy"] / 1e6),
            "  CPU, the plain Python restatement on one thread: {0:.2f} Mwords/s ({1:,} words)".format(r["cpu_words_per_s"] / 1e6, r["cpu_sample"]), ""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--words", type=int, default=100_000_000)      # EVT 3.0 words of the stream, as tools/time_evt3.py counts them
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evt2_time.txt"))
    ap.add_argument("--step_timeout", type=int, default=280)       # seconds per encoding
    ap.add_argument("--one")                                       # (the child's mode) one encoding, a JSON line on stdout
    args = ap.parse_args()
    if args.one:     # (a comma-separated list measures several in one process: one kernel trace with every kernel in it)
        for encoding in args.one.split(","):
            print("RESULT " + json.dumps(measure(encoding, args.words)), flush=True)
        return
    results = []
    for encoding in ("EVT2", "EVT21", "EVT3"):
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", encoding, "--words", str(args.words)],
                               capture_output=True, text=True, timeout=args.step_timeout)
        found = [line for line in child.stdout.splitlines() if line.startswith("RESULT ")]
        if child.returncode != 0 or not found:
            sys.exit("{0}: the measurement ended with status {1}\n{2}".format(encoding, child.returncode, (child.stdout + child.stderr)[-3000:]))
        results.append(json.loads(found[-1][7:]))
        print("\n".join(lines_of(results[-1])), flush=True)
    lines = ["EVT 2.0 / EVT 2.1 / EVT 3.0 decode of the same events, " + results[0]["device"] + ", median of {0}, HIP events".format(REPEATS),
             "1280 x 720, {0} repetitions of one burst segment".format(results[0]["repetitions"]), ""]
    for r in results:
        lines += lines_of(r)
    lines.append("Agreement with the vendor's decoder: unmeasured (no Metavision SDK here).")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print("wrote " + args.out)


if __name__ == "__main__":
    main()
