"""The renderer on the GPU (csrc/render.hip through frlw_evd_amd/visualize.py): everything here is BYTE-EQUAL to the numpy
restatement in tests/render_restated.py -- the colour conversion over its whole domain, the four backgrounds through a
non-integer nearest ratio and a ragged right edge, the box painter at every clipping and size case, batches against single
frames, the BGR overlay against the fused call, and the PNG frames detect_recording.py writes."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import render_restated as rr  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN4 = ["ped", "cyc", "car", "trk", "bus", "sign", "light"]
STORED = (16, 24)
CANVAS = (40, 56)


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from frlw_evd_amd import visualize
    return visualize


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def test_hsv_to_bgr_whole_domain():
    vz = need_gpu()
    S = (0, 1, 128, 254, 255)
    hsv = np.zeros((len(S), 256, 256, 3), np.uint8)
    hsv[..., 0] = np.arange(256, dtype=np.uint8)[None, :, None]
    hsv[..., 2] = np.arange(256, dtype=np.uint8)[None, None, :]
    for i, s in enumerate(S):
        hsv[i, :, :, 1] = s
    got = host(vz.hsv_to_bgr(dev(hsv)))
    want = rr.hsv_to_bgr(hsv)
    bad = np.argwhere((got != want).any(axis=-1))
    assert len(bad) == 0, (len(bad), hsv[tuple(bad[0])], got[tuple(bad[0])], want[tuple(bad[0])])
    assert (got[0] == hsv[0, :, :, 2:3]).all()      # S = 0: grey V


def volumes(C, seed, n=2):
    """(n, C, 16, 24) uint8: frame 0 uniform over all 256 levels (every level present in channel 0), frame 1 from a handful of
    levels, so that channels tie for the maximum and around the median, ECI's p == q and EV's equal bins occur; a few pixels
    hold one value in every channel."""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 256, (n, C) + STORED, dtype=np.uint8)
    v[0, 0].reshape(-1)[:256] = rng.permutation(256).astype(np.uint8)
    v[1:] = rng.choice(np.array([0, 1, 90, 127, 128, 180, 254, 255], np.uint8), size=(n - 1, C) + STORED)
    v[:, :, 3, 5:9] = v[:, :1, 3, 5:9]
    v[:, :, 0, 0] = 0
    v[:, :, 15, 23] = 255
    return v


BACKGROUND_CASES = [("TAF", 16), ("TAF", 2), ("TAF", 6), ("TAF", 20), ("SAE", 6), ("ECI", 2), ("EV", 10), ("EV", 2)]   # TAF above 16 channels: the median that re-reads


@pytest.mark.parametrize("shape", [(13, 19), (16, 24)], ids=["13x19", "16x24"])
@pytest.mark.parametrize("mode,C", BACKGROUND_CASES, ids=[f"{m}{c}" for m, c in BACKGROUND_CASES])
def test_backgrounds(mode, C, shape):
    vz = need_gpu()
    v = volumes(C, 100 + C)
    assert len(np.unique(v)) == 256
    top = np.sort(v[1].astype(np.int16), axis=0)
    assert C < 2 or (top[-1] == top[-2]).any()                          # two channels tie for the maximum
    if mode == "ECI":
        assert (v[:, 0] == v[:, 1]).any() and (v[:, 0] > v[:, 1]).any() and (v[:, 0] < v[:, 1]).any()
    if mode == "EV" and C > 2:
        c = np.maximum(v[1, C // 2:], v[1, :C // 2]).astype(np.int16)
        assert ((c == c.max(0)).sum(0) > 1).any()                       # equal bins: the first one keeps the hue
    got = host(vz.render(dev(v), mode, shape))
    want = rr.render(v, mode, shape)
    assert got.shape == want.shape == (2,) + shape + (3,)
    assert np.array_equal(got, want), np.argwhere((got != want).any(axis=-1))[:5]
    long_name = {"TAF": "TAF", "SAE": "SurfaceOfActiveEvent", "ECI": "EventCountImage", "EV": "EventVolume"}[mode]
    assert torch.equal(vz.render(dev(v), long_name, shape), dev(got))   # the reference's datatype names


def row(x, y, w, h, cls=0, conf=0.5):
    return [0, x, y, w, h, cls, conf, 0]


def box_frames():
    """Per frame (gt rows, dt rows) on the 40 x 56 canvas (label map: gen4's, for a five-letter class)."""
    rng = np.random.default_rng(77)
    sizes = (0, 1, 3, 4, 5)
    frames = [
        # clipped at the left, right, top and bottom edge; wholly outside; negative origin
        ([row(-5, 20, 12, 9), row(50, 18, 20, 10, 2)], [row(20, -6, 14, 12, 1, 0.25), row(30, 35, 12, 20, 3, 0.07)]),
        ([row(100, 100, 10, 10), row(-200, 5, 20, 20), row(10, -90, 5, 5)], [row(300, 2, 4, 4), row(-10, -10, 15, 30, 4, 0.99)]),
        # widths and heights 0, 1, 3, 4, 5 (a box narrower than 4 is filled), as ground truth and as detections
        ([row(2 + 10 * i, 17, w, sizes[(i + 2) % 5]) for i, w in enumerate(sizes)], []),
        ([], [row(1 + 9 * i, 18 + 4 * (i % 2), sizes[(i + 3) % 5], h, 5, 0.5) for i, h in enumerate(sizes)]),
        ([row(3, 30, w, w, 6) for w in sizes], [row(44, 20 + w, w, 5 - w, 0, 0.1 * w) for w in sizes]),
        # the tag cut by row 0 and by the right edge (and by both)
        ([row(4, 5, 20, 20, 5)], [row(30, 25, 10, 10, 2, 0.33), row(40, 3, 12, 30, 0, 0.5)]),
        ([row(30, 0, 10, 10, 1), row(54, 15, 1, 1, 2)], [row(0, 0, 5, 5, 6, 1.0), row(55, 39, 0, 0, 1, 0.0)]),
        # order: a detection over a ground truth that lies over ... an earlier detection's tag is over the ground truth
        ([row(10, 20, 20, 15, 2)], [row(8, 30, 30, 8, 1, 0.61), row(12, 22, 25, 12, 3, 0.42), row(14, 34, 6, 4, 0, 0.9)]),
        # a five-letter class with score 1.00, characters outside the table (none here), a class beyond the map (its number)
        ([row(1, 16, 30, 20, 6)], [row(2, 38, 50, 1, 6, 1.0), row(3, 17, 40, 10, 9, 0.999)]),
        ([], []),
    ]
    gt = [row(int(x), int(y), int(w), int(h), int(c)) for x, y, w, h, c in
          zip(rng.integers(-20, 60, 200), rng.integers(-20, 50, 200), rng.integers(0, 30, 200), rng.integers(0, 30, 200), rng.integers(0, 7, 200))]
    dt = [row(float(x), float(y), float(w), float(h), int(c), float(s)) for x, y, w, h, c, s in
          zip(rng.uniform(-20, 60, 312), rng.uniform(-20, 50, 312), rng.uniform(0, 30, 312), rng.uniform(0, 30, 312), rng.integers(0, 7, 312),
              rng.uniform(0, 1, 312))]
    frames.append((gt, dt))                                            # exactly 512 boxes
    return [(np.array(g, np.float64).reshape(-1, 8), np.array(d, np.float64).reshape(-1, 8)) for g, d in frames]


@pytest.fixture(scope="module")
def canvas():
    """11 frames: TAF volumes (C = 2) at 16 x 24, the boxes of box_frames, and the restatement's image of them on 40 x 56."""
    frames = box_frames()
    v = volumes(2, 9, n=len(frames))
    gt, dt = [g for g, _ in frames], [d for _, d in frames]
    want = rr.render(v, "TAF", CANVAS, gt, dt, GEN4)
    want.setflags(write=False)
    return v, gt, dt, want


def test_boxes_every_case(canvas):
    vz = need_gpu()
    v, gt, dt, want = canvas
    assert [len(g) + len(d) for g, d in zip(gt, dt)][-2:] == [0, 512]
    got = host(vz.render(dev(v), "TAF", CANVAS, gt, dt, GEN4))
    for i in range(len(v)):
        bad = np.argwhere((got[i] != want[i]).any(axis=-1))
        assert len(bad) == 0, (i, len(bad), bad[:5].tolist())
    plain = rr.render(v, "TAF", CANVAS)
    assert np.array_equal(got[-2], plain[-2])                          # the frame without boxes is its background
    changed = [(got[i] != plain[i]).any(axis=-1).sum() for i in range(len(v))]
    assert changed[1] > 0 and all(c > 0 for c in changed[:-2]), changed  # every other frame shows something
    assert ((got[8] == 0).all(axis=-1) & (plain[8] != 0).any(axis=-1)).sum() > 40     # glyph pixels: "lig", "light", "1.00", "9"
    with pytest.raises(ValueError):
        vz.render(dev(v[:1]), "TAF", CANVAS, [gt[-1]], [np.concatenate([dt[-1], dt[-1][:1]])], GEN4)    # 513 boxes


@pytest.mark.parametrize("n", [1, 3, 64])
def test_batched_equals_single_frames(canvas, n):
    vz = need_gpu()
    v, gt, dt, want = canvas
    pick = [(7 * i + 3) % len(v) for i in range(n)]                    # different box counts from frame to frame
    vol = dev(v[pick])
    g, d = [gt[j] for j in pick], [dt[j] for j in pick]
    got = vz.render(vol, "TAF", CANVAS, g, d, GEN4)
    assert np.array_equal(host(got), want[pick])
    for i in sorted(set([0, n // 2, n - 1])):
        assert torch.equal(vz.render(vol[i:i + 1], "TAF", CANVAS, [g[i]], [d[i]], GEN4)[0], got[i]), i


def test_more_than_64_frames_are_split(canvas):
    vz = need_gpu()
    v, gt, dt, want = canvas
    pick = [(5 * i + 1) % len(v) for i in range(67)]
    got = vz.render(dev(v[pick]), "TAF", CANVAS, [gt[j] for j in pick], [dt[j] for j in pick], GEN4)
    assert np.array_equal(host(got), want[pick])


def test_bgr_overlay_equals_the_fused_call(canvas):
    vz = need_gpu()
    v, gt, dt, want = canvas
    plain = vz.render(dev(v), "TAF", CANVAS)
    assert np.array_equal(host(vz.render(plain, "BGR", CANVAS, gt, dt, GEN4)), want)
    assert torch.equal(vz.render(plain, "BGR", CANVAS), plain)
    # a width that leaves rows unaligned and the last thread ragged
    odd = vz.render(dev(v), "TAF", (13, 19))
    g = [np.array([row(2, 12, 9, 5, 0)])] * len(v)
    assert np.array_equal(host(vz.render(odd, "BGR", (13, 19), g, None, GEN4)), rr.render(v, "TAF", (13, 19), g, None, GEN4))


# ---- detect_recording.py --frames on the GEN1-sized synthetic recording of tests/test_stream_detect_gpu.py

SPAN, PERIOD = 800_000, 50_000


def start_command(tmp_path, path, ck, tag, extra):
    """The two runs of the test go side by side: most of a run is the start of the process and the model build."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    out = str(tmp_path / f"boxes_{tag}")
    proc = subprocess.Popen([sys.executable, os.path.join(ROOT, "detect_recording.py"), "--dat", path, "--dataset", "gen1", "--exp_type",
                             "yolox", "--checkpoint", ck, "--event_volume_bins", "8", "--period", str(PERIOD), "--out", out, "--log_path",
                             str(tmp_path / tag) + "/", "--frames", str(tmp_path / f"frames_{tag}")] + extra,
                            env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    return proc, out + ".npy", str(tmp_path / f"frames_{tag}")


def finish_command(proc):
    try:
        stdout, stderr = proc.communicate(timeout=300)
    except subprocess.TimeoutExpired:
        proc.kill()
        raise
    assert proc.returncode == 0, stdout[-2000:] + stderr[-2000:]
    return stdout


def test_detect_recording_frames(tmp_path):
    vz = need_gpu()
    from frlw_evd_amd import dat_io, synth
    from frlw_evd_amd.yolox import build_yolox
    from frlw_evd_amd.yolox.model import recipe_state_dict
    rec = synth.to_dat8(synth.synth_events(21, 400_000, 304, 240, SPAN, hotspot=True))
    path = str(tmp_path / "rec_td.dat")
    dat_io.write_dat(path, rec, 240, 304)
    net = build_yolox(16, 2)
    ck = str(tmp_path / "weights.pth")
    torch.save({"state_dict": {"module." + k: v for k, v in recipe_state_dict(net, seed=1004).items()}, "epoch": 0}, ck)

    plain_run = start_command(tmp_path, path, ck, "plain", [])
    seq_run = start_command(tmp_path, path, ck, "seq", ["--seq_nms", "stop", "--frames_every", "2"])
    try:
        check_frames(vz, path, plain_run, seq_run)
    finally:
        for proc, _, _ in (plain_run, seq_run):
            if proc.poll() is None:
                proc.kill()
                proc.communicate()


def check_frames(vz, path, plain_run, seq_run):
    from frlw_evd_amd import dat_io, dataset
    from frlw_evd_amd import event_representation as er
    from frlw_evd_amd import seq_nms as sn
    # the volumes the command's detector read: one chain over the recording, a frame every 5 windows
    f_event = dat_io.DatFile(path)
    stamps = [PERIOD * j for j in range(1, f_event.total_time() // PERIOD + 1)]
    assert len(stamps) == 15
    rows = f_event.to_device()
    t = rows.view(torch.int32).reshape(-1, 2)[:, 0].to(torch.int64) & 0xFFFFFFFF
    cut = int(torch.searchsorted(t, torch.tensor([stamps[-1]], device=t.device), right=False))
    state = torch.full((240, 304, 2, 8), -6000.0, device="cuda")
    u8 = er.encode_taf_chain(rows[:cut], (240, 304), state, 0, 10_000, [5] * len(stamps), 8, flip_k=True)
    vol = u8.reshape(len(stamps), 16, 240, 304)

    def per_frame(boxes):
        return [boxes[boxes["t"] == ts] for ts in stamps]

    def decoded(folder, which):
        names = sorted(os.listdir(folder))
        assert names == sorted(f"rec_{stamps[j]}.png" for j in which), names
        return np.stack([vz.read_png(os.path.join(folder, f"rec_{stamps[j]}.png")) for j in which])

    proc, npy, folder = plain_run
    text = finish_command(proc)
    assert "'frames': 15" in text and "'frames_written': 15" in text, text[-300:]
    plain = dataset.read_boxes(npy)
    assert len(plain) > 0
    want = vz.render(vol, "TAF", (240, 304), dt=per_frame(plain))
    got = decoded(folder, range(15))
    assert got.shape == (15, 240, 304, 3) and np.array_equal(got, host(want))
    assert not np.array_equal(got, host(vz.render(vol, "TAF", (240, 304))))       # boxes were drawn

    # --seq_nms stop: backgrounds per batch, boxes overlaid at the end == one fused render with the rescored boxes that
    # no sequence suppressed; every second frame
    proc, npy, folder = seq_run
    text = finish_command(proc)
    assert "'frames_written': 8" in text, text[-300:]
    frames = []
    for m in per_frame(plain):
        r = np.zeros((len(m), 8), np.float32)
        for j, name in enumerate(("x", "y", "w", "h", "class_id", "class_confidence")):
            r[:, j + 1] = m[name]
        frames.append(r)
    kept, _ = sn.rescore_frames(frames, isolated="stop", metric="avg", drop_suppressed=True)
    which = list(range(0, 15, 2))
    want = vz.render(vol[which], "TAF", (240, 304), dt=[kept[j] for j in which])
    assert np.array_equal(decoded(folder, which), host(want))
    written = dataset.read_boxes(npy)
    assert len(written) == len(plain)                                             # the box file keeps the suppressed ones
