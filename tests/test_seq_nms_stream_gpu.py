"""StreamDetector with Seq-NMS over the whole recording: the small random-weight model and the synthetic recording of
tests/test_stream_detect_gpu.py.  ``seq_nms=None`` leaves the output byte-equal to the plain run; in ``stop`` mode without a drop
the boxes stay, and ``class_confidence`` / ``track_id`` equal the restatement (tests/seqnms_restated.py) applied to the plain
run's boxes."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import seqnms_restated  # noqa: E402
from test_stream_detect_gpu import CASES, FRAMES, FRAMES_PER_CALL, IMG, K, PERIOD, T_BEGIN, WINDOW, build_net, recording, stamps  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

THRESHOLDS = (0.3, 0.1, 0.03, 0.01)   # the head's confidence threshold, lowered until boxes of neighbouring frames link


def frames_of(rec):
    """A ``run()`` result -> the per-frame (n, 8) float32 rows it was made of."""
    rows = []
    for ts in stamps():
        m = rec[rec["t"] == ts]
        r = np.zeros((len(m), 8), np.float32)
        for j, name in enumerate(("x", "y", "w", "h", "class_id", "class_confidence", "track_id")):
            r[:, j + 1] = m[name]
        r[:, 0] = ts
        rows.append(r)
    return rows


def test_run_with_seq_nms_equals_the_restatement_on_the_plain_run():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from frlw_evd_amd import seq_nms as sn
    from frlw_evd_amd.stream import StreamDetector, to_bbox_records
    sensor, input_bins, seed, wseed = CASES["resize_up"]
    dat = torch.from_numpy(recording(sensor, seed).view(np.uint8).reshape(-1, 8).copy()).cuda()
    t_end = T_BEGIN + FRAMES * PERIOD

    def detector(net, **kw):
        return StreamDetector(net, sensor, IMG, dataset="gen1", volume_bins=K, input_bins=input_bins, period_us=PERIOD, window_us=WINDOW,
                              frames_per_call=FRAMES_PER_CALL, **kw)
    found = None
    for thr in THRESHOLDS:
        net = build_net(input_bins, wseed)
        net.head.obj_threshold = thr
        net = net.cuda()
        plain = detector(net).run(dat, T_BEGIN, t_end)
        rows = frames_of(plain)
        frames, picks = sn.rows_to_frames(rows)
        res, selections, _ = seqnms_restated.seq_nms(frames, isolated="stop")
        print("threshold", thr, "boxes per frame", [len(r) for r in rows], "sequences", [len(p) for _, p, _ in selections])
        if selections:
            found = (net, plain, rows, picks, res, selections)
            break
    assert found is not None, "no two boxes of neighbouring frames link at any threshold: the test has nothing to compare"
    net, plain, rows, picks, res, selections = found
    assert (plain["track_id"] == 0).all()
    # seq_nms=None: byte-equal to today's output
    assert detector(net, seq_nms=None).run(dat, T_BEGIN, t_end).tobytes() == plain.tobytes()
    det = detector(net, seq_nms={"isolated": "stop"})
    got = det.run(dat, T_BEGIN, t_end)
    want = to_bbox_records(sn.apply_to_rows(rows, picks, res), stamps())
    assert det.sequences == len(selections) >= 1
    for name in ("t", "x", "y", "w", "h", "class_id"):
        assert got[name].tobytes() == plain[name].tobytes(), name          # the same boxes
    assert got.tobytes() == want.tobytes()
    assert sorted(set(got["track_id"].tolist()) - {0}) == list(range(1, len(selections) + 1))
    # skip mode finds at least as many sequences, and dropping removes exactly the flagged boxes
    res_skip, sel_skip, _ = seqnms_restated.seq_nms(sn.rows_to_frames(rows)[0], isolated="skip")
    det = detector(net, seq_nms={"isolated": "skip", "drop_suppressed": True})
    dropped = det.run(dat, T_BEGIN, t_end)
    assert det.sequences == len(sel_skip) >= len(selections)
    assert len(dropped) == len(plain) - int(sum(s.sum() for _, _, s in res_skip))


def test_detect_recording_writes_track_ids(tmp_path):
    """The command with ``--seq_nms skip`` on the GEN1-sized synthetic recording of tests/test_stream_detect_gpu.py: the box file
    holds non-zero ``track_id``s, one id per printed sequence, and what ``rescore_records`` makes of the plain command's file."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from frlw_evd_amd import dat_io, dataset, synth
    from frlw_evd_amd import seq_nms as sn
    from frlw_evd_amd.yolox import build_yolox
    from frlw_evd_amd.yolox.model import recipe_state_dict
    span = 800_000
    rec = synth.to_dat8(synth.synth_events(21, 400_000, 304, 240, span, hotspot=True))
    path = str(tmp_path / "rec_td.dat")
    dat_io.write_dat(path, rec, 240, 304)
    net = build_yolox(16, 2)
    ck = str(tmp_path / "weights.pth")
    torch.save({"state_dict": {"module." + k: v for k, v in recipe_state_dict(net, seed=1004).items()}, "epoch": 0}, ck)
    outs = {}
    for mode in ("off", "skip"):
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
        out = str(tmp_path / f"boxes_{mode}")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "detect_recording.py"), "--dat", path, "--dataset", "gen1", "--exp_type", "yolox",
                            "--checkpoint", ck, "--event_volume_bins", "8", "--period", "50000", "--out", out, "--log_path",
                            str(tmp_path) + "/", "--seq_nms", mode], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs[mode] = (dataset.read_boxes(out + ".npy"), r.stdout)
    plain, text = outs["off"]
    assert "'sequences': 0" in text and (plain["track_id"] == 0).all()
    got, text = outs["skip"]
    ids = sorted(set(got["track_id"].tolist()) - {0})
    assert ids and ids == list(range(1, len(ids) + 1)) and f"'sequences': {len(ids)}," in text, text[-300:]
    stamps = [50_000 * j for j in range(1, span // 50_000 + 1)]
    want, n = sn.rescore_records(plain, stamps=stamps, isolated="skip")
    assert n == len(ids) and got.tobytes() == want.tobytes()
