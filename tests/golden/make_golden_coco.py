#!/usr/bin/env python3
"""Golden records of the COCO hand-off, produced by the REFERENCE's own ``evaluate/src/metrics/coco_eval.py``
(evaluate_detection -> _match_times -> _to_coco_format -> _coco_eval) with ``pycocotools`` stubbed: the stub ``COCO`` /
``COCOeval`` capture the ``dataset`` and ``results`` the reference builds (and the area ``COCO.loadRes`` gives a
result, w * h of its bbox values).  No score is computed here.

    python tests/golden/make_golden_coco.py     # rewrites tests/golden/coco_windows.npz
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("FRLW_REFERENCE", "/root/reference")
sys.path.insert(0, REF)

CAPTURED = {}


class StubCOCO:
    def __init__(self):
        self.dataset = {}

    def createIndex(self):
        pass

    def loadRes(self, results):
        CAPTURED["dataset"] = self.dataset
        CAPTURED["results"] = results
        return self


class StubParams:
    imgIds = None


class StubCOCOeval:
    def __init__(self, gt, dt, iou_type):
        assert iou_type == "bbox"
        self.params = StubParams()
        self.stats = np.zeros(12)

    def evaluate(self):
        CAPTURED["imgIds"] = np.asarray(self.params.imgIds)

    def accumulate(self):
        pass

    def summarize(self):
        pass


def stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m


stub("pycocotools")
stub("pycocotools.coco", COCO=StubCOCO)
stub("pycocotools.cocoeval", COCOeval=StubCOCOeval)

from evaluate.src.metrics.coco_eval import evaluate_detection  # noqa: E402


def rows(rng, t, dtype, score=True, cls_hi=2):
    n = len(t)
    r = np.zeros((n, 8), dtype)
    r[:, 0] = t
    r[:, 1] = rng.uniform(0, 280, n)
    r[:, 2] = rng.uniform(0, 220, n)
    r[:, 3] = rng.uniform(3, 120, n)
    r[:, 4] = rng.uniform(3, 120, n)
    r[:, 5] = rng.integers(0, cls_hi + 1, n)   # cls_hi: one class outside the label map
    r[:, 6] = rng.uniform(0, 1, n) if score else 1.0
    r[:, 7] = rng.integers(0, 5, n)
    return r


def cases():
    rng = np.random.default_rng(4711)
    out = []
    # several files, sorted times, float32 detections
    gts, dts = [], []
    for f in range(4):
        tg = np.sort(rng.choice([1_000_000, 1_050_000, 1_100_000, 1_149_999], size=int(rng.integers(1, 7))))
        td = np.sort(rng.integers(950_000, 1_200_000, size=int(rng.integers(0, 12))))
        gts.append(rows(rng, tg, np.float64))
        dts.append(rows(rng, td, np.float32))
    gts.append(np.zeros((0, 8)))  # empty gt file: skipped
    dts.append(rows(rng, [1_000_000], np.float32))
    out.append(("files", gts, dts, 50_000))
    # unsorted and duplicate timestamps (gt and dt), float64 detections
    tg = np.array([2_000_000, 1_000_000, 1_000_000, 3_000_000, 2_000_000, 1_500_000], np.float64)
    td = np.array([1_000_000, 3_000_000, 1_000_000, 2_000_000, 1_500_000, 1_490_000, 2_000_000, 900_000], np.float64)
    out.append(("unsorted", [rows(rng, tg, np.float64)], [rows(rng, td, np.float64)], 20_000))
    # detections straddling the time window: t - tol - 1, t - tol, t + tol, t + tol + 1
    tol = 4999
    tg = np.array([1_000_000, 1_000_000, 1_020_000], np.float64)
    td = np.array([1_000_000 - tol - 1, 1_000_000 - tol, 1_000_000, 1_000_000 + tol, 1_000_000 + tol + 1, 1_020_000 + tol,
                   1_020_000 + tol + 1], np.float64)
    out.append(("straddle", [rows(rng, tg, np.float64)], [rows(rng, td, np.float32)], tol))
    # the evaluator's placeholder row (float64 zeros at the gt time), areas exactly 1024 / 9216 in float32 and float64
    g = rows(rng, [5_000_000] * 3, np.float64)
    g[0, 3:5] = (32.0, 32.0)
    g[1, 3:5] = (96.0, 96.0)
    ph = np.array([[5_000_000, 0, 0, 0, 0, 0, 0, 0]], np.float64)
    d32 = rows(rng, [5_000_000] * 3, np.float32)
    d32[0, 3:5] = (32.0, 32.0)
    d32[1, 3:5] = (0.1, 10240.0)  # float32 product != float64 product
    d32[2, 5] = -0.5             # int() truncates toward zero: class 0
    out.append(("placeholder", [g, g.copy()], [ph, d32], 50_000))
    return out


def main():
    out = {}
    for name, gts, dts, tol in cases():
        CAPTURED.clear()
        evaluate_detection(gts, dts, classes=("car", "pedestrian"), height=240, width=304, time_tol=tol)
        ds, res = CAPTURED["dataset"], CAPTURED["results"]
        out[f"{name}_tol"] = np.array(tol)
        out[f"{name}_nfiles"] = np.array(len(gts))
        for f, (g, d) in enumerate(zip(gts, dts)):
            out[f"{name}_gt_{f}"] = g
            out[f"{name}_dt_{f}"] = d
        out[f"{name}_n_img"] = np.array(len(ds["images"]))
        out[f"{name}_img_ids"] = np.array([im["id"] for im in ds["images"]])
        a = ds["annotations"]
        out[f"{name}_gt_image"] = np.array([x["image_id"] for x in a], np.int64)
        out[f"{name}_gt_cat"] = np.array([x["category_id"] for x in a], np.int64)
        out[f"{name}_gt_area"] = np.array([x["area"] for x in a], np.float64)
        out[f"{name}_gt_box"] = np.array([[float(v) for v in x["bbox"]] for x in a], np.float64).reshape(-1, 4)
        out[f"{name}_dt_image"] = np.array([x["image_id"] for x in res], np.int64)
        out[f"{name}_dt_cat"] = np.array([x["category_id"] for x in res], np.int64)
        out[f"{name}_dt_score"] = np.array([x["score"] for x in res], np.float64)
        out[f"{name}_dt_box"] = np.array([[float(v) for v in x["bbox"]] for x in res], np.float64).reshape(-1, 4)
        out[f"{name}_dt_area"] = np.array([float(x["bbox"][2] * x["bbox"][3]) for x in res], np.float64)  # loadRes
    path = os.path.join(HERE, "coco_windows.npz")
    np.savez_compressed(path, **out)
    print("coco_windows.npz", os.path.getsize(path), "bytes;", {k: int(out[k]) for k in out if k.endswith("_n_img")})


if __name__ == "__main__":
    main()
