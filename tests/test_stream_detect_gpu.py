"""StreamDetector / detect_recording.py: boxes at a fixed cadence from the raw records of one recording.

Two geometries on one synthetic recording each: a sensor smaller than the detector input (the volume is encoded natively and
resized up: GEN1) and a larger one (coordinate maps move the events, the encode runs at the detector's shape: 1 Mpx).  The
stream route -- one encode_taf_chain per group of frames -- must give, row for row and bit for bit, what the route without the
chain gives: one encode_taf_dat per frame with the state carried, the same hand-off, the same detector batches.  That the
comparison is about real boxes is established without the GPU: the CPU oracle's volumes through the torch CPU forward of the same
weights give between 1 and 200 boxes on at least half of the frames.
"""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from frlw_evd_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, WINDOW, PERIOD, FRAMES, T_BEGIN = 8, 10_000, 30_000, 12, 1_000_000   # (frames behind 0.5 s: the Prophesee filter drops earlier ones)
BINS = PERIOD // WINDOW
PER_WINDOW = 3_000
IMG = (64, 96)
FRAMES_PER_CALL = 5   # groups of 5, 5 and 2 frames
# geometry -> (sensor shape, input_bins, stream seed, weight seed).  With these seeds the CPU forward below finds a few boxes on
# most frames (the head's objectness biases need no shift); test_cpu_forward_finds_boxes asserts it.
CASES = {"resize_up": ((56, 72), 8, 11, 1004), "coordinate_maps": ((90, 160), 4, 12, 1004)}


def recording(sensor, seed):
    n = FRAMES * BINS * PER_WINDOW
    return synth.to_dat8(synth.synth_events(seed, n, sensor[1], sensor[0], FRAMES * PERIOD, hotspot=True, t_offset=T_BEGIN))


def build_net(input_bins, weight_seed):
    from frlw_evd_amd.yolox import build_yolox
    from frlw_evd_amd.yolox.model import recipe_state_dict
    net = build_yolox(2 * input_bins, 2)
    net.load_state_dict(recipe_state_dict(net, seed=weight_seed))
    return net.eval()


def encode_shape(sensor):
    return IMG if IMG[0] < sensor[0] else sensor


def stamps():
    return [T_BEGIN + j * PERIOD for j in range(1, FRAMES + 1)]


def kept_rows(ev, rows, keep):
    return rows[keep & (rows[:, 1:7] != 0).any(axis=1)]


@pytest.mark.parametrize("case", list(CASES))
def test_cpu_forward_finds_boxes(case):
    """No GPU code here: the oracle's TAF volumes, the hand-off in numpy, the torch CPU forward with decode and NMS, the
    evaluator's host arithmetic -> between 1 and 200 boxes on at least half of the frames."""
    from frlw_evd_amd.evaluator import evaluator
    from oracle import oracle as orc
    sensor, input_bins, seed, wseed = CASES[case]
    enc = encode_shape(sensor)
    rec = recording(sensor, seed)
    t = rec["t"].astype(np.int64)
    net = build_net(input_bins, wseed)
    ev = evaluator(None, FRAMES, 10000, sensor[1], sensor[0], IMG[1], IMG[0], "gen1")
    vols = []
    for j, ts in enumerate(stamps(), 1):
        view, _ = orc.taf_stream_dat8(rec[t < ts], sensor, enc, K, T_BEGIN, WINDOW, BINS * j, np.full(enc + (2, K), -6000, np.float32))
        u8 = np.ascontiguousarray(orc.quantize_u8(orc.leaky_transform(view.reshape(K, 2, enc[0], enc[1])))[::-1])
        vol = u8.reshape(2 * K, enc[0], enc[1])[:2 * input_bins]
        if enc != IMG:
            vol = orc.resize_nearest(np.ascontiguousarray(vol), IMG)
        vols.append(vol.astype(np.float32) / np.float32(255))
    with torch.no_grad():
        dets = net.detect(torch.from_numpy(np.stack(vols))[..., None])
    counts = []
    for d, ts in zip(dets, stamps()):
        rows = ev.transform_dt(d, ts)
        rows = ev.filter_boxes(rows)
        counts.append(int((rows[:, 1:7] != 0).any(axis=1).sum()))
    print(case, counts)
    assert sum(1 <= c <= 200 for c in counts) >= FRAMES // 2, counts


@pytest.mark.parametrize("case", list(CASES))
def test_stream_equals_the_per_frame_route(case):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from frlw_evd_amd import event_representation as er
    from frlw_evd_amd import transforms
    from frlw_evd_amd.stream import BBOX_DTYPE, StreamDetector
    sensor, input_bins, seed, wseed = CASES[case]
    enc = encode_shape(sensor)
    rec = recording(sensor, seed)
    dat = torch.from_numpy(rec.view(np.uint8).reshape(-1, 8).copy()).cuda()
    net = build_net(input_bins, wseed).cuda()
    det = StreamDetector(net, sensor, IMG, dataset="gen1", volume_bins=K, input_bins=input_bins, period_us=PERIOD, window_us=WINDOW,
                         frames_per_call=FRAMES_PER_CALL)
    got = det.run(dat, T_BEGIN, T_BEGIN + FRAMES * PERIOD + PERIOD // 2)   # (half a period at the end makes no frame)
    assert got.dtype == BBOX_DTYPE

    # the route without the chain
    xmap, ymap = er.coordinate_maps(sensor, IMG, dat.device) if enc != sensor else (None, None)
    times = stamps()
    cuts = np.searchsorted(rec["t"], [T_BEGIN] + times, side="left")
    state = torch.full(enc + (2, K), -6000.0, device="cuda")
    frames = []
    for j, ts in enumerate(times):
        u8, _ = er.encode_taf_dat(dat[cuts[j]:cuts[j + 1]], enc, state, ts - PERIOD, WINDOW, BINS, K, xmap=xmap, ymap=ymap)
        frames.append(u8)
    want = []
    for g in range(0, FRAMES, FRAMES_PER_CALL):
        u8 = torch.stack(frames[g:g + FRAMES_PER_CALL])
        S = u8.shape[0]
        vol = u8.reshape(S, 2 * K, enc[0], enc[1])[:, :2 * input_bins].contiguous()
        if enc != IMG:
            vol = er.resize_nearest(vol.reshape(-1, enc[0], enc[1]), IMG)
        x = transforms.transform_images(vol.reshape(S, 2 * input_bins, IMG[0], IMG[1]), [transforms.SampleParams()] * S)[..., 0]
        with torch.no_grad():
            outputs = net.detect(x)
        rows, keep = det.evaluator.transform_dt_batch(outputs, times[g:g + FRAMES_PER_CALL])
        for ts, r, k in zip(times[g:g + FRAMES_PER_CALL], rows, keep):
            for row in kept_rows(det.evaluator, r, k):
                want.append((ts,) + tuple(row[1:7]) + (0,))
    want = np.array(want, dtype=BBOX_DTYPE)
    print(case, "rows", len(got), "per frame", [int((got["t"] == ts).sum()) for ts in times])
    assert len(got) == len(want) and got.tobytes() == want.tobytes()
    assert sum(1 <= int((got["t"] == ts).sum()) <= 200 for ts in times) >= FRAMES // 2


def test_arguments():
    from frlw_evd_amd.stream import StreamDetector
    with pytest.raises(ValueError):
        StreamDetector(None, (56, 72), IMG, period_us=25_000, window_us=10_000)
    with pytest.raises(ValueError):
        StreamDetector(None, (56, 72), IMG, input_bins=5)
    with pytest.raises(ValueError):
        StreamDetector(None, (56, 72), IMG, frames_per_call=65)
    d = StreamDetector(None, (56, 72), IMG, period_us=PERIOD)
    assert d.frame_times(100, 100 + 2 * PERIOD + 1) == [100 + PERIOD, 100 + 2 * PERIOD] and d.frame_times(0, PERIOD - 1) == []


def test_detect_recording_round_trip(tmp_path):
    """The command on a GEN1-sized recording with a checkpoint of recipe weights: <out>.npy holds what dataset.read_boxes reads
    back -- the fields of a *_bbox.npy file, timestamps on the frame grid."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from frlw_evd_amd import dat_io, dataset
    from frlw_evd_amd.stream import BBOX_DTYPE
    from frlw_evd_amd.yolox import build_yolox
    from frlw_evd_amd.yolox.model import recipe_state_dict
    span = 800_000
    rec = synth.to_dat8(synth.synth_events(21, 400_000, 304, 240, span, hotspot=True))
    path = str(tmp_path / "rec_td.dat")
    dat_io.write_dat(path, rec, 240, 304)
    net = build_yolox(16, 2)
    ck = str(tmp_path / "weights.pth")
    torch.save({"state_dict": {"module." + k: v for k, v in recipe_state_dict(net, seed=1004).items()}, "epoch": 0}, ck)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    out = str(tmp_path / "boxes")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "detect_recording.py"), "--dat", path, "--dataset", "gen1", "--exp_type", "yolox",
                        "--checkpoint", ck, "--event_volume_bins", "8", "--period", "50000", "--out", out, "--log_path", str(tmp_path) + "/"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "'frames': 15" in r.stdout, r.stdout[-500:]
    boxes = dataset.read_boxes(out + ".npy")
    assert boxes.dtype == BBOX_DTYPE
    assert ((boxes["t"] % 50_000 == 0) & (boxes["t"] > 500_000) & (boxes["t"] <= span)).all() and (boxes["track_id"] == 0).all()
