#!/usr/bin/env python3
"""Times the EVT 3.0 decode (frlw_evd_amd.raw_io: frlw_evt3_count + frlw_evt3_emit) and writes profiles/evt3_time.txt.

Two streams: a 1280 x 720 stream of about 100 M words with about half of its events in vector runs (a segment made by
``synth.synth_burst_events`` + ``raw_io.encode_evt3``, repeated -- every repetition opens with EVT_TIME_HIGH 0 behind a later value,
which the decoder takes as a clock wrap, so t keeps rising), and 64 M words of EVT_ADDR_X alone.  Each is decoded with the words
already in device memory, and again with the upload from host memory inside the timed region.  Median of 7, HIP events around
synchronised work.  Beside each time: the bytes the decode moves (the words are read three times, the records written once) per
second, and the rate of a device-to-device copy that moves the same number of bytes, measured here on the same device.  The CPU
figure is the plain Python restatement of the tests (tests/evt3_restated.py) on one thread.  Reported, not gated."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

REPEATS = 7


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


def main():
    import torch
    from frlw_evd_amd import raw_io, synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--words", type=int, default=100_000_000)
    ap.add_argument("--addr_x_words", type=int, default=64_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evt3_time.txt"))
    args = ap.parse_args()
    size = (720, 1280)
    lines = ["EVT 3.0 decode, " + torch.cuda.get_device_name(0) + ", median of {0}, HIP events".format(REPEATS),
             "chunk / lane piece: {0} / {1} words".format(*raw_io.geometry()), ""]

    seg_events = max(10_000, min(7_000_000, args.words // 14))
    seg = raw_io.encode_evt3(synth.to_dat8(synth.synth_burst_events(5, seg_events, size[1], size[0], seg_events // 50)))
    mix = np.tile(seg, max(1, -(-args.words // len(seg))))
    rng = np.random.default_rng(6)
    n_ax = args.addr_x_words
    plain = (0x2000 | rng.integers(0, 1280, size=n_ax, dtype=np.uint16) | (rng.integers(0, 2, size=n_ax, dtype=np.uint16) << 11)).astype(np.uint16)
    plain[:3] = [0x8000, 0x6000, 0x0005]

    for name, words in (("mix 1280x720 (half of the events in vector runs)", mix), ("EVT_ADDR_X only", plain)):
        host = torch.from_numpy(words.view(np.int16))
        dev = host.cuda()
        counters, state, ws = raw_io.evt3_count(dev, size)
        n = int(counters.events)
        out = torch.empty((n, 8), dtype=torch.uint8, device="cuda")

        def decode(w=dev):
            c, _, plan = raw_io.evt3_count(w, size)
            status = raw_io.evt3_emit(w, size, plan, out, n)
            assert status == 0 and int(c.events) == n

        moved = 3 * words.nbytes + 8 * n
        src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        t_dev = timed(decode, torch)
        t_up = timed(lambda: decode(host.cuda()), torch)
        t_copy = timed(lambda: dst.copy_(src), torch)
        kinds = np.bincount(words >> 12, minlength=16)
        lines += [name,
                  "  words {0:,}  events {1:,}  ({2:.2f} events / word; vector words {3:.1%}, unsorted {4}, time_loops {5})".format(
                      len(words), n, n / len(words), (kinds[4] + kinds[5]) / len(words), int(counters.unsorted), int(counters.time_loops)),
                  "  count + emit, words in device memory: {0:8.3f} ms  {1:7.2f} Gwords/s  {2:7.1f} GB/s moved (3 x words read, records written)".format(
                      t_dev, len(words) / t_dev / 1e6, moved / t_dev / 1e6),
                  "  count + emit with the upload:         {0:8.3f} ms  {1:7.2f} Gwords/s".format(t_up, len(words) / t_up / 1e6),
                  "  device-to-device copy moving as many bytes ({0:,} read + {0:,} written): {1:8.3f} ms  {2:7.1f} GB/s".format(
                      moved // 2, t_copy, moved / t_copy / 1e6), ""]
        del dev, out, src, dst, ws

    import evt3_restated
    sample = mix[:200_000]
    t0 = time.perf_counter()
    evt3_restated.decode(sample, size[1], size[0])
    dt = time.perf_counter() - t0
    lines += ["CPU, the plain Python restatement on one thread: {0:.2f} Mwords/s ({1:,} words of the mix)".format(len(sample) / dt / 1e6, len(sample)),
              "Agreement with the vendor's decoder: unmeasured (no Metavision SDK here)."]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
