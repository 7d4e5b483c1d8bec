"""COCO mAP host side without a GPU: the literal checker on hand cases, the windowing and CSR packing against the
reference's own records (tests/golden/coco_windows.npz), the host-only workspace query and the opt-in flags."""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coco_literal as lit  # noqa: E402

from frlw_evd_amd import _lib, coco_eval  # noqa: E402

EPS1 = 1.0 / (1.0 + np.spacing(1))  # 0.9999999999999998


def img(boxes, t=1_000_000, dtype=np.float64, score=None):
    """rows [t, x, y, w, h, class, score, 0] of one image; boxes: (x, y, w, h, class[, score])."""
    r = np.zeros((len(boxes), 8), dtype)
    for i, b in enumerate(boxes):
        r[i, 0] = t
        r[i, 1:6] = b[:5]
        r[i, 6] = b[5] if len(b) > 5 else 1.0
    return r


def test_hand_one_exact_match():
    p, r, st = lit.literal_eval([img([(10, 10, 50, 50, 0)])], [img([(10, 10, 50, 50, 0, .7)])], 1)
    for a in (0, 2):  # all, medium (2500 px)
        assert np.all(p[:, :, 0, a, :] == EPS1) and np.all(r[:, 0, a, :] == 1.0)
    assert np.all(p[:, :, 0, 1, :] == -1) and np.all(p[:, :, 0, 3, :] == -1)
    assert p[0, 0, 0, 0, 0] == 0.9999999999999998


def test_hand_two_gts_one_detection():
    p, r, st = lit.literal_eval([img([(10, 10, 50, 50, 0), (150, 100, 50, 50, 0)])], [img([(10, 10, 50, 50, 0, .7)])], 1)
    assert p[:, :, 0, 0, 2].mean(axis=1)[0] == 0.5049504950495048
    assert np.all(r[:, 0, 0, :] == 0.5)
    assert abs(st[0] - 0.5049504950495048) < 1e-15


def test_hand_fp_above_tp():
    p, r, st = lit.literal_eval([img([(10, 10, 50, 50, 0)])], [img([(200, 150, 50, 50, 0, .9), (10, 10, 50, 50, 0, .8)])], 1)
    assert np.all(p[:, :, 0, 0, 2] == 0.5) and st[0] == 0.5
    assert np.all(r[:, 0, 0, 0] == 0.0) and np.all(r[:, 0, 0, 2] == 1.0)  # maxDets 1 keeps the fp only


def test_hand_tp_fp_tp():
    gt = img([(10, 10, 50, 50, 0), (150, 100, 50, 50, 0)])
    dt = img([(10, 10, 50, 50, 0, .9), (80, 180, 40, 40, 0, .8), (150, 100, 50, 50, 0, .7)])
    p, r, st = lit.literal_eval([gt], [dt], 1)
    assert p[:, :, 0, 0, 2].mean(axis=1)[0] == 0.834983498349835
    assert abs(st[0] - 0.834983498349835) < 1e-15


def test_hand_area_1024_is_small_and_medium():
    p, r, st = lit.literal_eval([img([(10, 10, 32, 32, 0)])], [img([(10, 10, 32, 32, 0, .5)])], 1)
    assert np.all(p[:, :, 0, 1, :] == EPS1) and np.all(p[:, :, 0, 2, :] == EPS1) and np.all(p[:, :, 0, 3, :] == -1)


def test_hand_class_without_gt_is_excluded():
    p, r, st = lit.literal_eval([img([(10, 10, 50, 50, 0)])], [img([(10, 10, 50, 50, 0, .5), (100, 100, 30, 30, 1, .4)])], 2)
    assert np.all(p[:, :, 1] == -1) and np.all(r[:, 1] == -1)
    assert st[0] == pytest.approx(EPS1, abs=1e-15)


def test_hand_no_detection_raises():
    with pytest.raises(ValueError):
        lit.literal_eval([img([(10, 10, 50, 50, 0)])], [np.zeros((0, 8))], 1)
    with pytest.raises(ValueError):
        coco_eval.coco_eval_arrays([img([(10, 10, 50, 50, 0)])], [np.zeros((0, 8))])


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "coco_windows.npz"))


@pytest.mark.parametrize("case", ["files", "unsorted", "straddle", "placeholder"])
def test_windows_and_packing_equal_the_reference(golden, case):
    z = golden
    n = int(z[f"{case}_nfiles"])
    gts = [z[f"{case}_gt_{f}"] for f in range(n)]
    dts = [z[f"{case}_dt_{f}"] for f in range(n)]
    tol = int(z[f"{case}_tol"])
    # the restated _to_coco_format over the restated windows: the reference's records, value and type for value
    gw, dw = coco_eval.windows(gts, dts, tol)
    ds, res = coco_eval.to_coco_format(gw, dw, [{"id": 1}, {"id": 2}])
    assert len(ds["images"]) == int(z[f"{case}_n_img"]) and len(res) == len(z[f"{case}_dt_image"])
    assert [a["area"] for a in ds["annotations"]] == z[f"{case}_gt_area"].tolist()
    assert [a["category_id"] for a in ds["annotations"]] == z[f"{case}_gt_cat"].tolist()
    assert [float(b[2] * b[3]) for b in (x["bbox"] for x in res)] == z[f"{case}_dt_area"].tolist()
    # the CSR packing: rows of categories 1..2 only, same order
    p = coco_eval.pack(gts, dts, 2, tol)
    assert p["n_img"] == int(z[f"{case}_n_img"]) and p["n_results"] == len(z[f"{case}_dt_image"])
    for pre in ("gt", "dt"):
        cat = z[f"{case}_{pre}_cat"]
        keep = (cat >= 1) & (cat <= 2)
        assert np.array_equal(p[f"{pre}_cls"], (cat[keep] - 1).astype(np.int32)), pre
        assert p[f"{pre}_box"].tobytes() == z[f"{case}_{pre}_box"][keep].tobytes(), pre
        assert p[f"{pre}_area"].tobytes() == z[f"{case}_{pre}_area"][keep].tobytes(), pre
        image = np.repeat(np.arange(1, p["n_img"] + 1), np.diff(p[f"{pre}_off"]))
        assert np.array_equal(image, z[f"{case}_{pre}_image"][keep]), pre
    keep = (z[f"{case}_dt_cat"] >= 1) & (z[f"{case}_dt_cat"] <= 2)
    assert p["dt_score"].tobytes() == z[f"{case}_dt_score"][keep].tobytes()
    # and the literal checker's own windowing agrees
    lg, ld = lit.literal_windows(gts, dts, tol)
    assert [len(w) for w in lg] == [len(w) for w in gw] and all(a.tobytes() == b.tobytes() for a, b in zip(ld, dw))


def test_float32_area_keeps_its_rounding(golden):
    a = golden["placeholder_dt_area"]
    assert float(np.float32(0.1) * np.float32(10240.0)) in a.tolist()
    assert float(np.float64(np.float32(0.1)) * 10240.0) not in a.tolist()


def test_workspace_query_is_host_only():
    lib = _lib.load()
    small = lib.frlw_coco_workspace_bytes(10, 50, 500, 2)
    big = lib.frlw_coco_workspace_bytes(50_000, 500_000, 5_000_000, 2)
    assert 0 < small < big and big > 5_000_000 * 40
    assert lib.frlw_coco_workspace_bytes(10, 50, 500, 0) == 0
    assert lib.frlw_coco_workspace_bytes(10, 50, 500, 255) == 0
    assert lib.frlw_coco_workspace_bytes(-1, 50, 500, 2) == 0
    assert lib.frlw_coco_workspace_bytes(0, 0, 0, 2) > 0


def test_eval_rejects_bad_sizes_without_a_device():
    lib = _lib.load()
    assert lib.frlw_coco_eval(None, None, None, None, 0, None, None, None, None, None, 0, 1, 0, None, None, None, 0,
                              None, None, None) == _lib.FRLW_ERR_ARG


def test_metric_flag_on_both_entry_points():
    import test as test_entry
    import train as train_entry
    for mod in (train_entry, test_entry):
        assert mod.build_parser().parse_args([]).metric == "none"
        assert mod.build_parser().parse_args(["--metric", "coco"]).metric == "coco"
        with pytest.raises(SystemExit):
            mod.build_parser().parse_args(["--metric", "voc"])


def test_settings_without_metric_attribute(tmp_path):
    from frlw_evd_amd.settings import Setting_test, Setting_train_val
    ns = types.SimpleNamespace(local_rank=0, resume_exp=None, exp_name="E", exp_type="yolox", log_path=str(tmp_path) + "/",
                               dataset="gen1", bbox_path=None, data_path=None, event_volume_bins=8, batch_size=2,
                               num_cpu_workers=1, nodes=1, augmentation=True, record=None)
    assert Setting_train_val(ns).metric == "none" and Setting_test(ns).metric == "none"
    assert Setting_test(types.SimpleNamespace(**vars(ns), metric="coco")).metric == "coco"


def test_experiment_takes_the_scorer_only_when_asked():
    from frlw_evd_amd import exp
    base = dict(event_volume_bins=8, dataset_name="gen1")
    assert exp.yolox(types.SimpleNamespace(**base)).metric_fn is None
    assert exp.yolox(types.SimpleNamespace(**base, metric="none")).metric_fn is None
    assert exp.yolox(types.SimpleNamespace(**base, metric="coco")).metric_fn is coco_eval.evaluate_detection


def test_summary_lines_format():
    lines = coco_eval.summary_lines(np.array([0.5, 0.75, 0.25, -1, 0.1, 0.2, 0.3, 0.4, 0.45, -1, 0.5, 0.6]))
    assert len(lines) == 12
    assert lines[0] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 0.500"
    assert lines[1] == " Average Precision  (AP) @[ IoU=0.50      | area=   all | maxDets=100 ] = 0.750"
    assert lines[3] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area= small | maxDets=100 ] = -1.000"
    assert lines[6] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ] = 0.300"


def test_stats_of_matches_the_literal_summary():
    rng = np.random.default_rng(3)
    prec = rng.uniform(0, 1, (10, 101, 2, 4, 3))
    prec[:, :, 1, 1] = -1
    rec = rng.uniform(0, 1, (10, 2, 4, 3))
    rec[:, 0, 3] = -1
    assert coco_eval.stats_of(prec, rec).tobytes() == lit.literal_stats(prec, rec).tobytes()
