"""Motion-level evaluation on the GPU (frlw_time_surface_batch, frlw_box_flow_sums, the statistics files and the bucketed mAP).

Time-surface pairs are compared byte for byte: with the reference's own output (tests/golden/motion.npz) on the small frame, with
``motion.time_surface_numpy`` -- which tests/test_motion_cpu.py pins to the same golden -- where the golden would be large.  A DAT
record keeps its time in 32 bits, so "late" timestamps are such close to 2^32 (and above 2^31), not beyond it.

Box sums are compared with ``np.sum(mag.astype(float64))``, ``mag`` in float32: the operands are identical, only the float64
summation order differs, at most n * 2^-53 ~ 1e-10 for a full 1280 x 720 frame; 1e-9 is allowed.  Densities are compared with the
reference's float32 numpy sums within four times the difference the golden maker measured between those and a float64 sum
(``density_bound``); tests/test_motion_cpu.py asserts that no density of the fixture lies that close to a bucket edge."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import motion_data  # noqa: E402
from test_motion_cpu import restated_map  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def motion():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from frlw_evd_amd import motion
    return motion


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "motion.npz")))


def to_dev(rec):
    return torch.from_numpy(rec.view(np.uint8).reshape(-1, 8).copy()).cuda()


# ---- time-surface pairs -----------------------------------------------------------------------------------------------------------
def test_pairs_equal_the_reference(motion, golden):
    """Overlapping windows, one record more than a workgroup's slice, a window wholly outside the frame, an empty one, a stretch in
    swapped order, cells on both sides of the cutoff, and two windows that span 50 ms or less (numpy on the host, tallied)."""
    rec, win = motion_data.surface_stream(), motion_data.surface_windows()
    before = motion.motion_counts()[0]
    pairs, tally = motion.time_surface_pairs(to_dev(rec), list(win.values()), motion_data.FRAME)
    assert pairs.dtype == torch.uint8 and tuple(pairs.shape) == (len(win), 2) + motion_data.FRAME
    got = pairs.cpu().numpy()
    for i, name in enumerate(win):
        assert np.array_equal(got[i], golden["surface_pairs"][i]), name
    assert tally == {"calls": 1, "host_windows": len(motion_data.HOST_WINDOWS)}
    assert motion.motion_counts()[0] - before == 1


def test_pairs_with_late_timestamps(motion, golden):
    rec = motion_data.late_stream()
    pairs, tally = motion.time_surface_pairs(to_dev(rec), [(0, len(rec))], motion_data.FRAME)
    assert np.array_equal(pairs[0].cpu().numpy(), golden["late_pair"]) and tally["host_windows"] == 0


def test_65_windows_take_two_calls(motion):
    rec = motion_data.surface_stream()
    ranges = motion_data.many_windows(len(rec))
    before = motion.motion_counts()[0]
    pairs, tally = motion.time_surface_pairs(to_dev(rec), ranges, motion_data.FRAME)
    assert tally["calls"] == 2 and motion.motion_counts()[0] - before == 2
    got = pairs.cpu().numpy()
    for i, (lo, hi) in enumerate(ranges):
        assert np.array_equal(got[i], motion.time_surface_numpy(rec[lo:hi], motion_data.FRAME)), i


def test_one_gen1_window_of_100k_events(motion):
    rec = motion_data.big_stream()
    pairs, tally = motion.time_surface_pairs(to_dev(rec), [(0, len(rec))], motion_data.SENSOR)
    want = motion.time_surface_numpy(rec, motion_data.SENSOR)
    assert want[1].max() == 255 and np.array_equal(pairs[0].cpu().numpy(), want) and tally["host_windows"] == 0


def test_pairs_refuse_a_range_outside_the_tensor(motion):
    d = to_dev(motion_data.late_stream())
    for bad in ((-1, 5), (10, 5), (0, 3001)):
        with pytest.raises(ValueError):
            motion.time_surface_pairs(d, [bad], motion_data.FRAME)


# ---- box sums ---------------------------------------------------------------------------------------------------------------------
def sum_cases(T, H, W):
    """[flow, x0, x1, y0, y1]: 1 x 1, 1 x W, H x 1, the full frame, widths around the wavefront and the workgroup, an empty box, the
    last flow of the batch, two boxes on one flow."""
    cases = [[0, 3, 4, 5, 6], [0, 0, W, 7, 8], [0, 9, 10, 0, H], [0, 0, W, 0, H], [1, 5, 5, 2, 9], [1, 5, 9, 9, 9], [1, 9, 5, 2, 9],
             [T - 1, 1, W - 1, 1, H - 1], [1, 2, 30, 3, 11], [1, 20, 61, 0, 17]]
    for width in (63, 64, 65, 257):
        if width <= W:
            cases += [[T - 1, W - width, W, 1, H - 2], [0, 0, width, 0, 3]]
    return np.asarray(cases, dtype=np.int32)


@pytest.mark.parametrize("shape", [(3, 17, 70), (2, 240, 304)], ids=["17x70", "240x304"])
def test_box_flow_sums(motion, shape):
    T, H, W = shape
    flows = (np.random.default_rng(7340 + H).standard_normal((T, H, W, 2)) * 1.7).astype(np.float32)
    boxes = sum_cases(T, H, W)
    d = torch.from_numpy(flows).cuda()
    got = motion.box_flow_sums(d, boxes).cpu().numpy()
    again = motion.box_flow_sums(d, boxes).cpu().numpy()
    assert got.dtype == np.float64 and got.tobytes() == again.tobytes()   # a fixed reduction order
    for (f, x0, x1, y0, y1), g in zip(boxes, got):
        mag = np.sqrt(flows[f, y0:y1, x0:x1, 0] ** 2 + flows[f, y0:y1, x0:x1, 1] ** 2)
        assert mag.dtype == np.float32
        want = np.sum(mag.astype(np.float64))
        if mag.size == 0:
            assert g == 0.0
        else:
            assert abs(g - want) <= 1e-9 * want, (f, x0, x1, y0, y1, g, want)
    one = boxes[0]
    assert got[0] == float(np.sqrt(flows[0, one[3], one[1], 0] ** 2 + flows[0, one[3], one[1], 1] ** 2))   # one pixel: numpy's value


def test_box_flow_sums_refuse_a_box_outside_the_batch(motion):
    d = torch.zeros((2, 17, 70, 2), dtype=torch.float32, device="cuda")
    for bad in ([2, 0, 5, 0, 5], [0, 0, 71, 0, 5], [0, 0, 5, 0, 18], [0, -1, 5, 0, 5], [-1, 0, 5, 0, 5]):
        with pytest.raises(ValueError):
            motion.box_flow_sums(d, np.asarray([bad], dtype=np.int32))
    assert motion.box_flow_sums(d, np.zeros((0, 5), np.int32)).numel() == 0


# ---- statistics files and bucketed mAP, end to end --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run(motion, tmp_path_factory):
    """statistics_gt, statistics_dt and motion_level_map on the fabricated dataset."""
    root = str(tmp_path_factory.mktemp("motion_gpu"))
    raw = motion_data.build(root)
    flows = os.path.join(root, "optical_flow_buffer")
    gt = motion.statistics_gt(raw, "gen1", flow_dir=flows, out_dir=os.path.join(root, "statistics_result"))
    dt = motion.statistics_dt(raw, "gen1", motion_data.EXP_NAME, flow_dir=flows, log_dir=os.path.join(root, "log"))
    assert gt == os.path.join(root, "statistics_result", "gt_gen1.npz")
    assert dt == os.path.join(root, "log", motion_data.EXP_NAME, "summarise_stats.npz")
    stats_gt, stats_dt = dict(np.load(gt)), dict(np.load(dt))
    return {"root": root, "raw": raw, "gt": stats_gt, "dt": stats_dt, "map": motion.motion_level_map(stats_dt, stats_gt, "gen1")}


@pytest.mark.parametrize("kind", ["gt", "dt"])
def test_statistics_files_equal_the_references(run, golden, kind):
    got = run[kind]
    rows_key = "gts" if kind == "gt" else "dts"
    assert sorted(got) == sorted(["file_names", rows_key, "densitys"])
    bound = 4 * float(golden["density_bound"])
    assert len(got["file_names"]) == len(golden[f"{kind}_file_names"])
    for name in motion_data.FILES:   # the scripts walk os.listdir: the order of the files is the directory's, the rows' is fixed
        sel, ref = got["file_names"] == name, golden[f"{kind}_file_names"] == name
        assert got[rows_key].dtype == golden[f"{kind}_rows"].dtype and np.array_equal(got[rows_key][sel], golden[f"{kind}_rows"][ref])
        a, b = got["densitys"][sel].astype(np.float64), golden[f"{kind}_densitys"][ref].astype(np.float64)
        print(kind, name, "largest relative difference", np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)), "allowed", bound)
        assert np.all(np.abs(a - b) <= bound * np.abs(b))


def test_bucketed_map_equals_the_restatement(run, golden):
    seen = {"placeholder": [], "empty": []}
    want = restated_map(run["dt"]["dts"], run["dt"]["file_names"], run["dt"]["densitys"], run["gt"]["gts"], run["gt"]["file_names"],
                        run["gt"]["densitys"], seen)
    assert run["map"] == [float(w) for w in want] and seen == {"placeholder": [4], "empty": [3]}
    from_golden = restated_map(golden["dt_rows"], golden["dt_file_names"], golden["dt_densitys"], golden["gt_rows"], golden["gt_file_names"],
                               golden["gt_densitys"], {"placeholder": [], "empty": []})
    assert run["map"] == [float(w) for w in from_golden]   # the reference's own statistics files give the same five values


def test_generate_opticalflow_encodes_every_label(motion, run, tmp_path):
    """The command's loop: a file goes to the GPU once, its labels through time_surface_pairs.  Without cv2.optflow the pairs are
    what is saved; a second run finds every output and writes nothing."""
    flow_dir, surface_dir = str(tmp_path / "optical_flow_buffer"), str(tmp_path / "time_surface_buffer")
    n_labels = sum(len(motion_data.label_times(name)) for name in motion_data.FILES)
    assert motion.generate_opticalflow(run["raw"], "gen1", flow_dir, surface_dir) == n_labels
    assert motion.generate_opticalflow(run["raw"], "gen1", flow_dir, surface_dir) == 0
    if motion._tvl1() is None:
        from frlw_evd_amd import dat_io
        for name in motion_data.FILES:
            rec = motion_data.records(name)
            f_event = dat_io.DatFile(os.path.join(run["raw"], "test", name + "_td.dat"))
            for sl in dat_io.flow_label_slices(f_event, motion_data.label_times(name)):
                got = np.load(os.path.join(surface_dir, f"{name}_{sl['label_time']}.npy"))
                assert np.array_equal(got, motion.time_surface_numpy(rec[sl["start_count"]:sl["end_count"]], motion_data.SENSOR))
    else:
        assert len(os.listdir(flow_dir)) == n_labels
