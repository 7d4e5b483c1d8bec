"""Fabricated detections for Seq-NMS, regenerated from seeds on both sides: tests/golden/make_golden_seqnms.py runs the REFERENCE
on them, the tests run the restatement and the kernels, and only the answers are committed (tests/golden/seqnms.npz).

A case is a list of ``(n, 6)`` float64 frames ``[x1, y1, x2, y2, score, class]`` whose box columns hold float32 values.  Random
cases: constant-velocity tracks with jitter, dropped frames, false positives, lower-scored near-duplicates (to be suppressed) and
two classes.  Named cases: the edges listed in ``cases()``.
"""
import numpy as np

FRAME = (240.0, 304.0)


def _frame(rows):
    a = np.asarray(rows, dtype=np.float64).reshape(-1, 6)
    a[:, :4] = a[:, :4].astype(np.float32)
    return a


def random_case(seed, F=24, tracks=3, drop=0.1, false_pos=0.5, dup=0.3, max_boxes=12):
    rng = np.random.default_rng([7700, seed])
    frames = [[] for _ in range(F)]
    for k in range(tracks):
        t0 = int(rng.integers(0, max(1, F // 3)))
        t1 = int(rng.integers(min(F, t0 + 2), F + 1))
        w, h = rng.uniform(20, 70, 2)
        x, y = rng.uniform(0, FRAME[1] - w), rng.uniform(0, FRAME[0] - h)
        vx, vy = rng.uniform(-4, 4, 2)
        cls = k % 2
        base = rng.uniform(0.2, 0.95)
        for f in range(t0, t1):
            x, y = x + vx, y + vy
            if rng.uniform() < drop:
                continue
            j = rng.uniform(-2, 2, 4)
            box = [x + j[0], y + j[1], x + w + j[2], y + h + j[3]]
            frames[f].append(box + [float(np.clip(base + rng.uniform(-0.15, 0.15), 0.02, 1.0)), cls])
            if rng.uniform() < dup:   # a lower-scored near-duplicate, now and then of the other class
                d = rng.uniform(-5, 5, 4)
                frames[f].append([box[0] + d[0], box[1] + d[1], box[2] + d[2], box[3] + d[3], float(rng.uniform(0.02, 0.3)),
                                  cls if rng.uniform() < 0.7 else 1 - cls])
    for f in range(F):
        for _ in range(int(rng.poisson(false_pos))):
            w, h = rng.uniform(10, 60, 2)
            x, y = rng.uniform(0, FRAME[1] - w), rng.uniform(0, FRAME[0] - h)
            frames[f].append([x, y, x + w, y + h, float(rng.uniform(0.02, 0.999)), int(rng.integers(0, 2))])
        order = rng.permutation(len(frames[f]))[:max_boxes]
        frames[f] = [frames[f][i] for i in order]
    return [_frame(fr) for fr in frames]


def _still(box, score, cls, F, t0=0):
    """The same box in frames t0 .. t0 + F - 1 as (frame, row) pairs."""
    return [(t0 + k, list(box) + [score, cls]) for k in range(F)]


def _build(F, items):
    frames = [[] for _ in range(F)]
    for f, row in items:
        frames[f].append(row)
    return [_frame(fr) for fr in frames]


def wide64():
    """F = 3, the middle frame holds 64 disjoint boxes: box 63 is linked from frame 0 (mask bit 63) and links on to frame 2 (lane
    63 carries an out-edge); box 0 has a shorter path."""
    grid = [[20.0 * (k % 8), 20.0 * (k // 8), 20.0 * (k % 8) + 10, 20.0 * (k // 8) + 10, 0.1 + 0.01 * k, k % 2] for k in range(64)]
    b63, b0 = grid[63][:4], grid[0][:4]
    first = [b63 + [0.6, 1], b0 + [0.5, 0], [200, 200, 230, 230, 0.4, 0]]
    last = [[300, 0, 320, 20, 0.3, 1], [b63[0] + 1, b63[1], b63[2] + 1, b63[3], 0.7, 1]]
    return [_frame(first), _frame(grid), _frame(last)]


def exact_half():
    """Integer boxes: [0,0,2,1] against [0,0,1,1] has IoU exactly 0.5 and links; [0,0,3,1] against [0,0,1,1] (1/3) does not."""
    return [_frame([[0, 0, 2, 1, 0.5, 0], [10, 0, 13, 1, 0.9, 0]]),
            _frame([[10, 0, 11, 1, 0.9, 0], [0, 0, 1, 1, 0.25, 0]]),
            _frame([[0, 0, 2, 1, 0.5, 0]])]


def exact_three_tenths():
    """A = [0,0,3,2] stays for three frames; B = [0,1,7,2] (IoU with A exactly 3/10: 3 / (6 + 7 - 3)) stays for frames 1 and 2 and
    would be a sequence of its own -- unless the 0.3 threshold crosses as a double and suppresses it."""
    a, b = [0, 0, 3, 2], [0, 1, 7, 2]
    return _build(3, _still(a, 0.9, 0, 3) + _still(b, 0.6, 0, 2, t0=1))


def ties():
    """Every score 0.5.  P (frames 0-1) forks into two equal successors (the lower index wins); Q (frames 0-1) ties with P inside
    frame 0 (the lower box wins) and R (frames 1-2) ties with both across frames (the lower frame wins)."""
    p, q, r = [0, 0, 40, 40], [100, 0, 140, 40], [200, 100, 240, 140]
    items = [(0, p + [0.5, 0]), (0, q + [0.5, 0]),
             (1, [2, 0, 42, 40, 0.5, 0]), (1, [0, 2, 40, 42, 0.5, 0]), (1, q + [0.5, 0]), (1, r + [0.5, 1]),
             (2, r + [0.5, 1])]
    return _build(3, items)


def cross_class():
    """A (class 0) over three frames; C (class 1) in frames 1 and 2 overlaps frame 0's A exactly as much as A's own successor does
    (mirror image) and is not linked to it -- but it is suppressed by the A sequence, so C never forms one."""
    items = [(0, [10, 10, 50, 50, 0.9, 0]),
             (1, [12, 10, 52, 50, 0.8, 0]), (1, [8, 10, 48, 50, 0.95, 1]),
             (2, [14, 10, 54, 50, 0.85, 0]), (2, [6, 10, 46, 50, 0.9, 1])]
    return _build(3, items)


def stop_vs_skip():
    """12 frames: a strong track, an isolated 0.995 box and a weak track (0.2 a box over 4 frames: 0.8 < 0.995).  ``stop`` ends on the
    isolated box after the strong track; ``skip`` goes on to the weak one."""
    items = _still([20, 20, 70, 80], 0.8, 0, 10, t0=1) + _still([150, 100, 200, 160], 0.2, 1, 4, t0=5) + \
        [(3, [240, 10, 280, 60, 0.995, 1])]
    return _build(12, items)


def with_empty_frames():
    frames = random_case(31, F=12, tracks=3, drop=0.0)
    for f in (0, 6, 11):
        frames[f] = _frame([])
    return frames


def cases():
    """name -> frames.  Every case is small (F <= 40, N <= 12) except ``wide64`` (a 64-box frame) and ``long130`` (130 frames: a
    path and the reduction over the frames' roots cross a 64-frame boundary)."""
    return {
        "one_frame": random_case(1, F=1, tracks=2, false_pos=2.0),
        "two_frames": _build(2, _still([30, 30, 80, 90], 0.7, 0, 2) + [(1, [200, 50, 240, 90, 0.9, 1])]),
        "empty_frames": with_empty_frames(),
        "single_box_frames": _build(4, _still([50, 60, 120, 140], 0.6, 1, 4)),
        "wide64": wide64(),
        "exact_half": exact_half(),
        "exact_three_tenths": exact_three_tenths(),
        "ties": ties(),
        "cross_class": cross_class(),
        "long130": random_case(130, F=130, tracks=4, drop=0.02, false_pos=0.3, max_boxes=8),
        "stop_vs_skip": stop_vs_skip(),
        "random_a": random_case(11, F=40, tracks=5),
        "random_b": random_case(12, F=25, tracks=4, drop=0.2, false_pos=1.0, dup=0.5),
    }


def more_seeds(n=20):
    return {f"seed{k}": random_case(100 + k, F=int(8 + 2 * (k % 12)), tracks=2 + k % 4, drop=0.05 * (k % 4), false_pos=0.3 + 0.1 * (k % 5))
            for k in range(n)}
