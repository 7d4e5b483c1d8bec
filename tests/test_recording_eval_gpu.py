"""Evaluation straight from recordings against the file route, on the fabricated dataset of tests/recording_eval_data.py (GEN1
geometry, 240x304 -> 256x320, two test sequences so that batches cross a file boundary):

* ``RecordingLoader`` over the recordings yields, batch for batch, what ``Loader`` yields over the files ``generate.generate_*``
  wrote (run in-process here): images byte-equal, labels, names and stamps equal -- for every kind, a second lambda (a channel
  offset into the chain's volume), TAF with K = 8 and K = 4, and a 1 Mpx sequence (coordinate maps, no resize in the hand-off);
* ``exp.yolox`` / ``exp.yoloxtafBFM`` ``.test()`` through ``--data_path`` and through ``--raw_dir`` return the same lists byte for byte
  (one child process runs both routes of both recipes, tests/recording_eval_child.py), on frames that carry boxes;
* ``test.py --raw_dir ... --record True --metric coco`` prints the file route's ``test_loader_len`` and writes its summarise.npz.
"""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import recording_eval_data as red

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = 4


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    root = tmp_path_factory.mktemp("recording_eval")
    raw, lab = red.build_dataset(str(root / "dataset"))
    return {"root": str(root), "raw": raw, "lab": lab, "processed": str(root / "processed"), "done": set()}


def generated(work, command, dataset="gen1", raw=None, lab=None, processed=None):
    """Run an offline command once per module; returns the directory it wrote under."""
    from frlw_evd_amd import generate
    processed = processed or work["processed"]
    if (command, processed) not in work["done"]:
        getattr(generate, command)(raw or work["raw"], lab or work["lab"], processed, dataset)
        work["done"].add((command, processed))
    return processed


def file_loader(lab, data_dir, dataset, size, bins, taf):
    from frlw_evd_amd.dataset import Loader, propheseeDataset, propheseeTafDataset
    if taf:
        ds = propheseeTafDataset(lab, data_dir, dataset, size, size, 10000, bins, "test", False, False)
    else:
        ds = propheseeDataset(lab, data_dir, dataset, size, size, bins, 10000, 1, "test", False, False)
    return Loader(ds, BATCH, 2, False, "cuda", shuffle=False)


def assert_same_batches(files, recordings, sizes):
    assert len(files) == len(recordings) == len(sizes)
    a, b = list(files), list(recordings)
    assert [x[0].shape[0] for x in a] == [y[0].shape[0] for y in b] == sizes
    for k, (x, y) in enumerate(zip(a, b)):
        assert y[0].is_cuda and y[0].dtype == torch.float32 and x[0].shape == y[0].shape, k
        assert x[0].cpu().numpy().tobytes() == y[0].cpu().numpy().tobytes(), f"batch {k}: images differ"
        assert y[1].is_cuda and x[1].dtype == y[1].dtype == torch.float64 and x[1].shape == y[1].shape == (sizes[k], 80, 8)
        assert torch.equal(x[1], y[1]), f"batch {k}: labels differ"
        assert list(x[2]) == list(y[2]), f"batch {k}: names differ"
        assert np.asarray(x[3]).dtype == np.asarray(y[3]).dtype and np.array_equal(x[3], y[3]), f"batch {k}: stamps differ"
    return a


@pytest.mark.parametrize("name,bins", [("EventVolume250000", 5), ("EventCountImage50000", 1), ("SurfaceOfActiveEvents1e-05", 1),
                                       ("SurfaceOfActiveEvents2.5e-06", 1), ("taf", 8), ("taf", 4)])
def test_loader_equals_the_file_route(work, name, bins):
    from frlw_evd_amd.recording_dataset import RecordingLoader
    processed = generated(work, red.REPRESENTATIONS[name][1])
    size = list(red.TARGET)
    files = file_loader(work["lab"], os.path.join(processed, name), "gen1", size, bins, name == "taf")
    recordings = RecordingLoader(work["lab"], work["raw"], name, "gen1", size, size, bins, "test", BATCH, "cuda")
    kind = {"E": "ev", "S": "sae", "t": "taf"}[name[0]] if not name.startswith("EventCount") else "eci"
    planned = red.planned_samples(work["raw"], work["lab"], kind)
    assert recordings.samples == planned and len(files.dataset) == len(planned)
    sizes = [min(BATCH, len(planned) - i) for i in range(0, len(planned), BATCH)]
    assert sizes == [4, 4, 1]
    batches = assert_same_batches(files, recordings, sizes)
    assert [(n, int(t)) for b in batches for n, t in zip(b[2], b[3])] == planned
    assert batches[0][0].shape[1:] == (2 * bins, 256, 320, 1, 1)
    assert float(batches[1][0].max()) > 0    # the volumes are not empty
    # a second pass yields the same batches again (the generators start anew with every file)
    again = list(recordings)
    assert all(torch.equal(x[0], y[0]) for x, y in zip(batches, again)) and len(again) == len(batches)


def test_loader_with_coordinate_maps(work):
    """A 1 Mpx sequence: the sensor is larger than the detector input, the events are moved and the encode runs at 512 x 640 -- the
    hand-off does no resize.  The label behind the last event ends the file."""
    from frlw_evd_amd.recording_dataset import RecordingLoader
    raw, lab = red.build_gen4_dataset(os.path.join(work["root"], "gen4"))
    processed = generated(work, "generate_eventvolume", "gen4", raw, lab, os.path.join(work["root"], "gen4_processed"))
    size = list(red.GEN4_TARGET)
    files = file_loader(lab, os.path.join(processed, "EventVolume250000"), "gen4", size, 5, False)
    recordings = RecordingLoader(lab, raw, "EventVolume250000", "gen4", size, size, 5, "test", BATCH, "cuda")
    assert [t for _, t in recordings.samples] == red.GEN4_LABELS[:-1]
    assert (recordings.width, recordings.height) == (1280, 720) and len(recordings.object_classes) == 7
    batches = assert_same_batches(files, recordings, [4, 1])
    assert batches[0][0].shape[1:] == (10, 512, 640, 1, 1) and float(batches[0][0].max()) > 0


@pytest.fixture(scope="module")
def both_routes(work):
    """The child process: both routes of both entry-point cases -> the npz of their evaluator lists; (npz, log root)."""
    for case in red.ENTRY_CASES.values():
        generated(work, red.REPRESENTATIONS[case["representation"]][1])
    log_root = os.path.join(work["root"], "log")
    for key, case in red.ENTRY_CASES.items():
        red.write_checkpoint(os.path.join(log_root, key), case)
    out = os.path.join(work["root"], "routes.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "recording_eval_child.py"), work["raw"], work["lab"], work["processed"],
                        log_root, out], env=_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return np.load(out), log_root, r.stdout


def _env():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")


@pytest.mark.parametrize("key", list(red.ENTRY_CASES))
def test_entry_point_routes_agree(both_routes, key):
    got, _, _ = both_routes
    frames = []
    for name in ("gt_boxes_list", "dt_boxes_list"):
        n = int(got[f"{key}/files/{name}/n"])
        assert n == int(got[f"{key}/recordings/{name}/n"]) == 7   # the labels behind 0.5 s: the evaluator drops the others
        for i in range(n):
            a, b = got[f"{key}/files/{name}/{i}"], got[f"{key}/recordings/{name}/{i}"]
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (key, name, i)
            if name == "dt_boxes_list":
                frames.append(red.real_rows(b))
    print(key, "boxes per frame", frames)
    assert sum(1 <= c <= 200 for c in frames) >= (len(frames) + 1) // 2, frames


def test_command_round_trip(work, both_routes):
    """``test.py --raw_dir ... --record True --metric coco`` against the file route's run of the same checkpoint."""
    _, log_root, child_out = both_routes
    case = red.ENTRY_CASES["yolox"]
    log = os.path.join(log_root, "yolox") + "/"
    assert child_out.count("test_loader_len: 3") == 4    # both routes of both cases
    r = subprocess.run([sys.executable, os.path.join(ROOT, "test.py"), "--raw_dir", work["raw"], "--bbox_path", work["lab"],
                        "--representation", case["representation"], "--record", "True", "--metric", "coco", "--resume_exp", "R",
                        "--exp_type", case["exp_type"], "--event_volume_bins", str(case["bins"]), "--batch_size", str(BATCH),
                        "--dataset", "gen1", "--nodes", "1", "--log_path", log], env=_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "test_loader_len: 3" in r.stdout and "Current score" in r.stdout, r.stdout[-1000:]
    want = np.load(os.path.join(log, "R", "summarise_files.npz"))
    got = np.load(os.path.join(log, "R", "summarise.npz"))
    assert sorted(got.files) == sorted(want.files) == ["dts", "file_names"]
    assert len(want["dts"]) > 0 and got["dts"].dtype == want["dts"].dtype and got["dts"].tobytes() == want["dts"].tobytes()
    assert list(got["file_names"]) == list(want["file_names"])
