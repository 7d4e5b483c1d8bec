"""Motion-level evaluation, the host half (no GPU): label slices, the numpy restatement of the time surface, the isolation filter
and the clamp against tests/golden/motion.npz (written by the reference, tests/golden/make_golden_motion.py), the bucket edges,
and ``motion_level_map`` against a restatement written here that buckets literally and scores with tests/coco_literal.py."""
import os
import re

import numpy as np
import pytest
from numpy.lib import recfunctions as rfn

import coco_literal
import motion_data
from frlw_evd_amd import _lib, dat_io, evaluator, motion, settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "motion.npz")))


@pytest.fixture(scope="module")
def raw_dir(tmp_path_factory):
    return motion_data.build(str(tmp_path_factory.mktemp("motion_cpu")), with_flows=False)


# ---- label slices ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(motion_data.FILES))
def test_flow_label_slices_equal_the_reference_loader(golden, raw_dir, name):
    f_event = dat_io.DatFile(os.path.join(raw_dir, "test", name + "_td.dat"))
    got = [[sl["start_count"], sl["end_count"] - sl["start_count"]] for sl in dat_io.flow_label_slices(f_event, motion_data.label_times(name))]
    assert got == golden[f"slices_{name}"].tolist()
    if name == "seqM":
        assert got[0][0] == 0 and got[-1][1] == 0   # the first label resets the loader, the last lies behind the recording


# ---- time surface -------------------------------------------------------------------------------------------------------------
def test_numpy_time_surface_equals_the_reference(golden):
    rec = motion_data.surface_stream()
    for i, (name, (lo, hi)) in enumerate(motion_data.surface_windows().items()):
        got = motion.time_surface_numpy(rec[lo:hi], motion_data.FRAME)
        assert got.dtype == np.uint8 and got.shape == (2,) + motion_data.FRAME
        assert np.array_equal(got, golden["surface_pairs"][i]), name
    assert np.array_equal(motion.time_surface_numpy(motion_data.late_stream(), motion_data.FRAME), golden["late_pair"])


def test_surface_fixture_holds_its_cases(golden):
    """What the windows are there for, read off the golden itself."""
    rec, win, pairs = motion_data.surface_stream(), motion_data.surface_windows(), golden["surface_pairs"]
    names = list(win)
    assert not pairs[names.index("all_outside")].any() and not pairs[names.index("empty")].any()
    v1, v2 = pairs[names.index("cutoff")]
    assert v1[9, 7] > 0 and v2[9, 7] > v1[9, 7]      # hit on both sides of end - 50 ms: two different last writers
    assert v1[10, 8] == 0 and v2[10, 8] > 0           # hit only behind it
    lo, hi = win["swapped"]
    t = rec["t"][lo:hi].astype(np.int64)
    assert (np.diff(t) < 0).any()                     # the stretch is not time-sorted
    for name in motion_data.HOST_WINDOWS:
        lo, hi = win[name]
        ev = synth_in_frame(rec[lo:hi])
        assert len(ev) and ev.max() - ev.min() <= 50000
    assert motion_data.late_stream()["t"].min() > 2 ** 31


def synth_in_frame(rec):
    w = rec["_"].astype(np.int64)
    ok = ((w & 16383) < motion_data.FRAME[1]) & (((w >> 14) & 16383) < motion_data.FRAME[0])
    return rec["t"][ok].astype(np.int64)


# ---- isolation filter and clamp -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(motion_data.isolation_cases()))
def test_isolated_boxes_equal_the_reference(golden, name):
    rows = motion_data.isolation_cases()[name]
    assert [int(i) for i in motion.isolated_boxes(rows)] == golden[f"keep_{name}"].tolist()


def test_isolated_boxes_five_box_case():
    """Not a score NMS: both members of an overlapping pair go."""
    assert [int(i) for i in motion.isolated_boxes(motion_data.isolation_cases()["five"])] == [4]


def label_rows(kind, name):
    """(label time, rows of that label) as the statistics scripts select them."""
    src = rfn.structured_to_unstructured(motion_data.boxes(name))
    det_names, det_rows = motion_data.detections()
    for t in np.unique(src[:, 0]):
        if kind == "gt":
            yield t, src[src[:, 0] == t]
        else:
            d = det_rows[det_names == name]
            yield t, d[(d[:, 0] >= t - 4999) & (d[:, 0] <= t + 4999)]


@pytest.mark.parametrize("kind", ["gt", "dt"])
@pytest.mark.parametrize("name", sorted(motion_data.FILES))
def test_isolated_and_clamped_rows_equal_the_reference_files(golden, kind, name):
    """float64 label rows (gt) and float32 recorded detections (dt), in the rows' own dtype."""
    got = [motion._label_rows(rows, motion_data.SENSOR)[0] for _, rows in label_rows(kind, name)]
    got = np.concatenate(got)
    want = golden[f"{kind}_rows"][golden[f"{kind}_file_names"] == name]
    assert got.dtype == want.dtype == (np.float64 if kind == "gt" else np.float32)
    assert np.array_equal(got, want)


def test_clamp_boxes_edge_cases():
    rows = np.array([[1, 400, 100, 30, 30, 0, 1, 0],       # wholly outside the frame: both corners land on W - 1
                     [1, -20, -10, 60, 50, 1, 1, 0],       # negative corners
                     [1, 250, 180, 80, 90, 1, 1, 0],       # leaves the frame at the far side: W - 1, H - 1, not W, H
                     [1, 10.5, 20.25, 30.75, 40.5, 0, 1, 0]], dtype=np.float64)
    out, corners = motion.clamp_boxes(rows, (240, 304))
    assert out[:, 1:5].tolist() == [[303, 100, 0, 30], [0, 0, 40, 40], [250, 180, 53, 59], [10.5, 20.25, 30.75, 40.5]]
    assert corners.tolist() == [[303, 100, 303, 130], [0, 0, 40, 40], [250, 180, 303, 239], [10.5, 20.25, 41.25, 60.75]]
    assert rows[0, 1] == 400                                 # the input is not written
    out32, _ = motion.clamp_boxes(rows.astype(np.float32), (240, 304))
    assert out32.dtype == np.float32
    boxes, div = motion.integer_boxes(out, corners, [0, 0, 1, 2])
    assert boxes.tolist() == [[0, 303, 303, 100, 130], [0, 0, 40, 0, 40], [1, 250, 303, 180, 239], [2, 10, 41, 20, 60]]
    # int(y2 - y1) * int(x2 - x1), not the slice's pixel count: 40 * 30 where the slice holds 40 x 31 pixels
    assert div.tolist() == [0 + 1e-8, 1600 + 1e-8, 59 * 53 + 1e-8, 40 * 30 + 1e-8]


# ---- buckets ----------------------------------------------------------------------------------------------------------------------
def test_bucket_edges_are_the_references():
    assert settings.MOTION_LEVEL_EDGES == {
        "gen1": [0.0, 0.09472751189131885, 0.2538587115258659, 0.6169536673563197, 1.703355726917305, 1000],
        "gen4": [0.0, 0.061864120261698595, 0.47486729209948575, 1.4415784200310098, 4.20493449274388, 1000]}


def test_no_fixture_density_lies_at_a_bucket_edge(golden):
    """The GPU test allows the densities four times ``density_bound`` (relative) off the reference's float32 sums: no density of
    the fixture may come that close to an edge, so bucket membership cannot flip."""
    bound = 4 * float(golden["density_bound"])
    assert 0 < bound < 1e-5
    for d in np.concatenate([golden["gt_densitys"], golden["dt_densitys"]]).astype(np.float64):
        for e in settings.MOTION_LEVEL_EDGES["gen1"][1:]:
            assert abs(d - e) > 2 * bound * max(abs(d), e)


def literal_scorer(gt_list, dt_list, time_tol, classes, height, width):
    return tuple(coco_literal.literal_eval(gt_list, dt_list, len(classes), time_tol)[2][:6])


def restated_map(dts, names_dt, dens_dt, gts, names_gt, dens_gt, seen):
    """motion_level_evaluation.py:53-80 on GEN1, statement by statement; an empty bucket gives -1.0 (the product's documented
    deviation: the reference would hand pycocotools an empty result list)."""
    edges = [0.0, 0.09472751189131885, 0.2538587115258659, 0.6169536673563197, 1.703355726917305, 1000]
    results = []
    for i in range(0, len(edges) - 1):
        dt, gt = [], []
        for file_name in np.unique(names_gt):
            dt.append(dts[(names_dt == file_name) & (dens_dt >= edges[i]) & (dens_dt < edges[i + 1])])
            gt.append(gts[(names_gt == file_name) & (dens_gt >= edges[i]) & (dens_gt < edges[i + 1])])
        gt1, dt1 = [], []
        for l1, l2 in zip(map(evaluator.filter_boxes_gen1, gt), map(evaluator.filter_boxes_gen1, dt)):
            if len(l1) > 0:
                gt1.append(l1)
                if len(l2) == 0:
                    dt1.append(np.array([[l1[0, 0], 0, 0, 0, 0, 0, 0, 0]]))
                    seen["placeholder"].append(i)
                else:
                    dt1.append(l2)
        if not gt1:
            seen["empty"].append(i)
            results.append(-1.0)
            continue
        results.append(coco_literal.literal_eval(gt1, dt1, 2, 4999)[2][0])
    return results


def golden_stats(golden):
    return ({"dts": golden["dt_rows"], "file_names": golden["dt_file_names"], "densitys": golden["dt_densitys"]},
            {"gts": golden["gt_rows"], "file_names": golden["gt_file_names"], "densitys": golden["gt_densitys"]})


def test_motion_level_map_equals_the_literal_restatement(golden, capsys):
    stats_dt, stats_gt = golden_stats(golden)
    seen = {"placeholder": [], "empty": []}
    want = restated_map(stats_dt["dts"], stats_dt["file_names"], stats_dt["densitys"], stats_gt["gts"], stats_gt["file_names"],
                        stats_gt["densitys"], seen)
    got = motion.motion_level_map(stats_dt, stats_gt, "gen1", metric_fn=literal_scorer)
    assert len(got) == 5 and [float(g) for g in got] == [float(w) for w in want]
    assert seen == {"placeholder": [4], "empty": [3]}      # ground truth without a detection; no ground truth at all
    assert got[3] == -1.0 and 0.0 <= got[4] < 0.05 and max(got[:3]) > 0.1
    printed = capsys.readouterr().out.splitlines()
    assert printed[0] == "0 0.0 0.09472751189131885" and printed[4] == "4 1.703355726917305 1000" and printed[5] == str(got)


# ---- commands and exports ---------------------------------------------------------------------------------------------------------
def test_script_flags_parse():
    a = motion.PARSERS["generate_opticalflow"]().parse_args(["-raw_dir", "R"])
    assert (a.raw_dir, a.dataset) == ("R", "gen1")
    a = motion.PARSERS["motion_level_statistics_gt"]().parse_args(["-raw_dir", "R", "-dataset", "gen4"])
    assert (a.raw_dir, a.dataset) == ("R", "gen4")
    a = motion.PARSERS["motion_level_statistics_dt"]().parse_args(["-raw_dir", "R", "--dataset", "gen4", "-exp_name", "E"])
    assert (a.raw_dir, a.dataset, a.exp_name) == ("R", "gen4", "E")
    a = motion.PARSERS["motion_level_evaluation"]().parse_args(["-exp_name", "E"])
    assert (a.dataset, a.exp_name) == ("gen1", "E")
    for which in motion.PARSERS:
        text = open(os.path.join(ROOT, which + ".py")).read()
        assert f'motion.main("{which}")' in text


def test_statistics_dt_refuses_a_missing_record(tmp_path):
    with pytest.raises(FileNotFoundError):
        motion.statistics_dt(str(tmp_path), "gen1", "nothing_recorded", log_dir=str(tmp_path / "log"))
    assert not os.path.exists(tmp_path / "log" / "nothing_recorded" / "summarise.npz")


def test_exports_are_declared():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "frlw_evd.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in ("frlw_time_surface_workspace_bytes", "frlw_time_surface_batch", "frlw_box_flow_sums", "frlw_motion_counts"):
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    # host-only answers: two 64-bit key planes per window behind the header, and the window limit
    small = lib.frlw_time_surface_workspace_bytes(1000, 1, 24, 40)
    assert lib.frlw_time_surface_workspace_bytes(1000, 3, 24, 40) - small == 2 * 2 * 24 * 40 * 8
    assert lib.frlw_time_surface_workspace_bytes(1000, 65, 24, 40) == 0 and lib.frlw_time_surface_workspace_bytes(1000, 0, 24, 40) == 0
