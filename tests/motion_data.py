"""Fabricated inputs of the motion-level evaluation, regenerated from seeds on both sides: tests/golden/make_golden_motion.py runs
the REFERENCE on them (``PSEELoader``, ``generate_timesurface``, ``nms``, the two statistics scripts), the tests run the product,
and only the answers are committed (tests/golden/motion.npz).  TV-L1 flows are not computed anywhere: a "flow" is a seeded normal
field whose scale puts the label's boxes into a chosen density bucket.

Time surfaces: one stream on a 24 x 40 frame whose sensor is 30 x 48, so about a third of the events lie outside the frame, with
the windows of ``surface_windows()``; a second stream with timestamps close to the end of the record's 32-bit time field.

Dataset (GEN1 sensor, ``<root>/raw/test/<seq>_td.dat`` + ``<seq>_bbox.npy`` side by side, as the statistics scripts read them):
  seqM  seven label times: one closer than 500 ms to the file start (the loader is reset: records [0, 500 ms)), two 2 ms apart (a
        detection lies within 4999 us of both), the five-box isolation case, boxes that leave the frame or start at negative
        corners, a label without any recorded detection, and one behind the last event (no records).
  seqN  three label times.
Densities fall into buckets 0, 1, 2 and 4 of the GEN1 edges; bucket 3 holds no ground truth at all, bucket 4 ground truth without a
detection (the placeholder row).
"""
import os

import numpy as np

from frlw_evd_amd import dat_io, synth

SENSOR = (240, 304)
BBOX_DTYPE = np.dtype([("t", "<u8"), ("x", "<f4"), ("y", "<f4"), ("w", "<f4"), ("h", "<f4"), ("class_id", "u1"),
                       ("class_confidence", "<f4"), ("track_id", "<u4")])
EXP_NAME = "exp_motion"

# ---- time surfaces ----------------------------------------------------------------------------------------------------------
FRAME = (24, 40)
SLICE = 2 * 8 * 256   # records one workgroup of the scatter takes


def surface_stream():
    """12 000 records over 700 ms, crafted stretches (see ``surface_windows``)."""
    ev = synth.synth_events(7301, 12_000, 48, 30, 700_000, t_offset=10_000)
    x, y, t = ev["x"], ev["y"], ev["t"]
    x[9200:9300] = 45                                  # a stretch wholly outside the frame
    # [5800, 7000): records 6100..6199 in reversed order, and one cell written twice inside them -- its last writer in stream order
    # carries the EARLIER time
    for k in ("x", "y", "p", "t"):
        ev[k][6100:6200] = ev[k][6100:6200][::-1].copy()
    hit = (x[5800:7000] == 3) & (y[5800:7000] == 5)
    x[5800:7000][hit] = 0
    x[6120], y[6120], x[6180], y[6180] = 3, 5, 3, 5
    assert t[6120] > t[6180]
    # [7000, 9000): cell (7, 9) hit in front of and behind end - 50 ms, cell (8, 10) only behind it
    for cx, cy in ((7, 9), (8, 10)):
        hit = (x[7000:9000] == cx) & (y[7000:9000] == cy)
        x[7000:9000][hit] = 1
    x[7010], y[7010], x[8990], y[8990], x[8995], y[8995] = 7, 9, 7, 9, 8, 10
    x[10000], y[10000] = 1, 1                          # a window of this one record: den = -50 000
    return synth.to_dat8(ev)


def surface_windows():
    """name -> record range of ``surface_stream()``, in the order of the golden's ``surface_pairs``."""
    return {
        "overlap_a": (0, 3000), "overlap_b": (1500, 4500), "overlap_c": (2500, 5600),
        "slice_plus_one": (5000, 5000 + SLICE + 1),
        "all_outside": (9200, 9300), "empty": (777, 777),
        "swapped": (5800, 7000),
        "cutoff": (7000, 9000),
        "short_span": (10000, 10300), "one_event": (10000, 10001),
        "whole": (0, 12000),
    }


HOST_WINDOWS = ("short_span", "one_event")   # event span <= 50 ms: computed in numpy, counted in the tally


def late_stream():
    """3 000 records over 600 ms that end 4 s before the 32-bit time field of a DAT record wraps (t > 2^31 throughout)."""
    return synth.to_dat8(synth.synth_events(7302, 3_000, 48, 30, 600_000, t_offset=4_290_000_000))


def many_windows(n_records=12000, n=65):
    step = n_records // 80
    return [(i * step, i * step + 12 * step + i) for i in range(n)]


def big_stream():
    """100 000 records on the GEN1 frame over 400 ms (one window)."""
    return synth.to_dat8(synth.synth_events(7303, 100_000, 304, 240, 400_000, hotspot=True, t_offset=5_000))


# ---- isolation filter ---------------------------------------------------------------------------------------------------------
def isolation_cases():
    """name -> rows whose columns 1..4 are corners (what the scripts hand to ``nms``)."""
    def rows(corners, dtype=np.float64):
        out = np.zeros((len(corners), 8), dtype)
        out[:, 1:5] = corners
        return out
    rng = np.random.default_rng(7310)
    xy = rng.uniform(0, 200, (40, 2))
    rand = np.concatenate([xy, xy + rng.uniform(5, 60, (40, 2))], axis=1)
    return {
        "five": rows([[0, 0, 10, 10], [5, 5, 15, 15], [50, 50, 60, 60], [52, 52, 70, 70], [100, 100, 110, 110]]),
        "none": rows(np.zeros((0, 4))),
        "one": rows([[3, 4, 30, 40]]),
        "chain": rows([[0, 0, 20, 20], [10, 0, 30, 20], [20, 0, 40, 20], [100, 0, 120, 20]]),
        "degenerate": rows([[10, 10, 10, 40], [10, 10, 30, 40], [200, 200, 230, 230]]),
        "random": rows(rand),
        "random_f32": rows(rand, np.float32),
    }


# ---- dataset ------------------------------------------------------------------------------------------------------------------
# file -> (seed, events, span us, t offset, [(label time, flow scale, [(x, y, w, h, class)])])
FILES = {
    "seqM": (7321, 120_000, 2_400_000, 1_000, [
        (300_000, 0.04, [(50, 60, 40, 30, 0), (150.5, 100.25, 33.3, 44.7, 1)]),
        (700_000, 0.04, [(20, 30, 40, 50, 0), (200.5, 120.5, 60.25, 40.75, 1)]),
        (702_000, 0.13, [(22, 31, 40, 50, 0), (120, 40, 30, 35, 1)]),
        (1_200_000, 0.35, [(0, 0, 10, 10, 0), (5, 5, 10, 10, 0), (50, 50, 10, 10, 0), (52, 52, 18, 18, 0), (100, 100, 30, 30, 0),
                           (250, 180, 80, 90, 1)]),
        (1_900_000, 2.5, [(60, 70, 45, 38, 0), (180, 40, 50.5, 60.5, 1)]),
        (2_390_000, 0.35, [(400, 100, 30, 30, 0), (-20, -10, 60, 50, 1), (130, 100, 40.6, 40.7, 0)]),
        (3_500_000, 0.13, [(10, 10, 30, 30, 0)]),
    ]),
    "seqN": (7322, 60_000, 1_500_000, 0, [
        (600_000, 0.13, [(30.2, 40.9, 50.7, 30.1, 0), (170, 150, 44, 52, 1)]),
        (900_000, 0.04, [(90, 20, 35, 45, 1), (10.5, 180.5, 60, 40, 0)]),
        (1_400_000, 0.35, [(220, 60, 70.5, 80.5, 0), (40, 100, 33, 29, 1)]),
    ]),
}
NO_DETECTIONS = {("seqM", 1_900_000)}


def label_times(name):
    return np.asarray([lab[0] for lab in FILES[name][4]], dtype=np.int64)


def records(name):
    seed, n, span, t0, _ = FILES[name]
    return synth.to_dat8(synth.synth_events(seed, n, SENSOR[1], SENSOR[0], span, t_offset=t0))


def boxes(name):
    labels = FILES[name][4]
    out = np.zeros(sum(len(lab[2]) for lab in labels), dtype=BBOX_DTYPE)
    i = 0
    for t, _, rows in labels:
        for k, (x, y, w, h, c) in enumerate(rows):
            out[i] = (t, x, y, w, h, c, 1.0, k)
            i += 1
    return out


def flow(name, label_time):
    """The (240, 304, 2) float32 "flow" of one label."""
    scale = {lab[0]: lab[1] for lab in FILES[name][4]}[int(label_time)]
    seed = [FILES[name][0], int(label_time)]
    return (np.random.default_rng(seed).standard_normal((SENSOR[0], SENSOR[1], 2)) * scale).astype(np.float32)


def detections():
    """``summarise.npz`` as ``evaluator.recorder`` writes it: (file names, (n, 8) float32 rows [t, x, y, w, h, class, score, 0])."""
    rng = np.random.default_rng(7330)
    names, rows = [], []
    for name, (_, _, _, _, labels) in FILES.items():
        for t, _, gts in labels:
            if (name, t) in NO_DETECTIONS:
                continue
            for (x, y, w, h, c) in gts:
                jit = rng.uniform(-2, 2, 4)
                cls = c if rng.uniform() < 0.85 else 1 - c
                rows.append([t + (3000 if rng.uniform() < 0.3 else 0), x + jit[0], y + jit[1], w + jit[2], h + jit[3], cls,
                             rng.uniform(0.3, 1.0), 0])
                names.append(name)
            rows.append([t, rng.uniform(0, 250), rng.uniform(0, 190), rng.uniform(12, 50), rng.uniform(12, 50), rng.integers(0, 2),
                         rng.uniform(0.05, 0.6), 0])   # a false positive
            names.append(name)
    return np.array(names), np.asarray(rows, dtype=np.float32)


def build(root, with_flows=True):
    """Write the dataset, the flows and ``log/<EXP_NAME>/summarise.npz`` under ``root`` (the working directory the scripts expect);
    returns the raw directory."""
    raw = os.path.join(root, "raw")
    os.makedirs(os.path.join(raw, "test"), exist_ok=True)
    os.makedirs(os.path.join(root, "log", EXP_NAME), exist_ok=True)
    for name in FILES:
        dat_io.write_dat(os.path.join(raw, "test", name + "_td.dat"), records(name), SENSOR[0], SENSOR[1])
        np.save(os.path.join(raw, "test", name + "_bbox.npy"), boxes(name))
        if with_flows:
            os.makedirs(os.path.join(root, "optical_flow_buffer"), exist_ok=True)
            for t in label_times(name):
                np.save(os.path.join(root, "optical_flow_buffer", f"{name}_{t}.npy"), flow(name, t))
    names, rows = detections()
    np.savez(os.path.join(root, "log", EXP_NAME, "summarise.npz"), file_names=names, dts=rows)
    return raw
