"""COCO bounding-box mAP of the evaluator's paired box lists, scored on the GPU (reference:
evaluate/src/metrics/coco_eval.py:15-168, which hands the windows to pycocotools' COCOeval).

``evaluate_detection`` has the reference's signature and returns its 6-tuple (AP, AP50, AP75, AP_small, AP_medium,
AP_large), so it is a drop-in ``metric_fn`` for ``evaluator.evaluate``.  The windowing (``match_times``, :47-86) and the
COCO records (``to_coco_format``, :116-168) are restated here; the windows are packed as CSR arrays in a few numpy
operations per file and ``frlw_coco_eval`` (csrc/coco_eval.hip) computes COCOeval's ``precision`` / ``recall`` arrays,
bit for bit.  The 12 summary numbers are their means, taken here as pycocotools' ``summarize`` takes them.
"""
from __future__ import annotations

import numpy as np
import torch

# pycocotools Params.setDetParams, built the way it builds them: AP50 / AP75 select thresholds by ==.
IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
AREA_LBL = ["all", "small", "medium", "large"]
MAX_DETS = [1, 10, 100]


def match_times(all_ts, gt_boxes, dt_boxes, time_tol):
    """coco_eval.py:47-86: the two-pointer walk over the sorted unique ground-truth times ``all_ts``.  Returns the
    window bounds (lo_gt, hi_gt, lo_dt, hi_dt) as int64 arrays; the windows are ``gt_boxes[lo_gt[i]:hi_gt[i]]`` and
    ``dt_boxes[lo_dt[i]:hi_dt[i]]``.  Sorted times take searchsorted (the walk's result then); otherwise the walk runs
    literally, which is what it does on times that are not sorted."""
    gt_t = np.asarray(gt_boxes[:, 0], dtype=np.float64)
    dt_t = np.asarray(dt_boxes[:, 0], dtype=np.float64)
    lo, hi = all_ts - time_tol, all_ts + time_tol
    if np.all(gt_t[1:] >= gt_t[:-1]) and np.all(dt_t[1:] >= dt_t[:-1]):
        lo_g = np.searchsorted(gt_t, all_ts, "left")
        hi_g = np.maximum(np.searchsorted(gt_t, all_ts, "right"), lo_g)
        lo_d = np.searchsorted(dt_t, lo, "left")
        hi_d = np.maximum(np.searchsorted(dt_t, hi, "right"), lo_d)
        return lo_g.astype(np.int64), hi_g.astype(np.int64), lo_d.astype(np.int64), hi_d.astype(np.int64)
    n_g, n_d, n = len(gt_t), len(dt_t), len(all_ts)
    out = np.zeros((4, n), np.int64)
    low_g = high_g = low_d = high_d = 0
    for s, ts in enumerate(all_ts):
        while low_g < n_g and gt_t[low_g] < ts:
            low_g += 1
        high_g = max(low_g, high_g)
        while high_g < n_g and gt_t[high_g] <= ts:
            high_g += 1
        while low_d < n_d and dt_t[low_d] < lo[s]:
            low_d += 1
        high_d = max(low_d, high_d)
        while high_d < n_d and dt_t[high_d] <= hi[s]:
            high_d += 1
        out[:, s] = (low_g, high_g, low_d, high_d)
    return out[0], out[1], out[2], out[3]


def windows(gt_boxes_list, dt_boxes_list, time_tol=50000):
    """coco_eval.py:30-43: per file (both lists non-empty) one window per unique ground-truth time -> the flattened
    lists of (gt rows, dt rows), the COCO images 1..N in order."""
    gts, dts = [], []
    for gt, dt in zip(gt_boxes_list, dt_boxes_list):
        if gt.shape[0] == 0 or dt.shape[0] == 0:
            continue
        lg, hg, ld, hd = match_times(np.unique(gt[:, 0]), gt, dt, time_tol)
        gts += [gt[a:b] for a, b in zip(lg, hg)]
        dts += [dt[a:b] for a, b in zip(ld, hd)]
    return gts, dts


def to_coco_format(gts, detections, categories, height=240, width=304):
    """coco_eval.py:116-168: the COCO ``dataset`` (images, annotations, categories) and the ``results`` list that
    ``_coco_eval`` gives pycocotools.  A per-box loop: the GPU path packs arrays instead (``pack``); this form is the
    record of what those arrays mean."""
    images, annotations, results = [], [], []
    for n, (gt, pred) in enumerate(zip(gts, detections)):
        im_id = n + 1
        images.append({"date_captured": "2019", "file_name": "n.a", "id": im_id, "license": 1, "url": "",
                       "height": height, "width": width})
        for b in gt:
            annotations.append({"area": float(b[3] * b[4]), "iscrowd": False, "image_id": im_id,
                                "bbox": [b[1], b[2], b[3], b[4]], "category_id": int(b[5]) + 1,
                                "id": len(annotations) + 1})
        for b in pred:
            results.append({"image_id": im_id, "category_id": int(b[5]) + 1, "score": float(b[6]),
                            "bbox": [b[1], b[2], b[3], b[4]]})
    dataset = {"info": {}, "licenses": [], "type": "instances", "images": images, "annotations": annotations,
               "categories": categories}
    return dataset, results


def _ranges(lo, hi):
    """Concatenation of arange(lo[i], hi[i]) for all i."""
    n = hi - lo
    total = int(n.sum())
    if total == 0:
        return np.zeros(0, np.int64)
    return np.repeat(lo - (np.cumsum(n) - n), n) + np.arange(total)


def _columns(rows, n_cls):
    """box (n, 4) f64, area = w * h in the rows' own dtype then widened (loadRes / ``float(area)``), class 0-based,
    score, and which rows have a category of the label map (``int(row[5]) + 1`` in 1..n_cls)."""
    cls = np.trunc(np.asarray(rows[:, 5], dtype=np.float64))
    keep = (cls >= 0) & (cls < n_cls)
    area = (rows[:, 3] * rows[:, 4]).astype(np.float64)
    return rows[:, 1:5].astype(np.float64), area, np.where(keep, cls, -1).astype(np.int32), \
        rows[:, 6].astype(np.float64), keep


def pack(gt_boxes_list, dt_boxes_list, n_cls, time_tol=50000):
    """The windows of ``windows`` as CSR arrays, rows of categories outside the label map dropped (COCOeval keeps only
    params.catIds).  Returns a dict: gt_box, gt_area, gt_cls, gt_off, dt_box, dt_area, dt_cls, dt_score, dt_off, n_img,
    n_results (= len(results), every detection row of every window, dropped categories included)."""
    parts = {k: [] for k in ("gt_box", "gt_area", "gt_cls", "dt_box", "dt_area", "dt_cls", "dt_score")}
    g_cnt, d_cnt, n_results = [], [], 0
    for gt, dt in zip(gt_boxes_list, dt_boxes_list):
        if gt.shape[0] == 0 or dt.shape[0] == 0:
            continue
        lg, hg, ld, hd = match_times(np.unique(gt[:, 0]), gt, dt, time_tol)
        n_results += int((hd - ld).sum())
        for (lo, hi, rows, pre, cnt) in ((lg, hg, gt, "gt_", g_cnt), (ld, hd, dt, "dt_", d_cnt)):
            box, area, cls, score, keep = _columns(rows, n_cls)
            idx = _ranges(lo, hi)
            kept_before = np.concatenate([[0], np.cumsum(keep)])
            cnt.append(kept_before[hi] - kept_before[lo])
            idx = idx[keep[idx]]
            parts[pre + "box"].append(box[idx])
            parts[pre + "area"].append(area[idx])
            parts[pre + "cls"].append(cls[idx])
            if pre == "dt_":
                parts["dt_score"].append(score[idx])
    out = {}
    for k, v in parts.items():
        shape = (0, 4) if k.endswith("box") else (0,)
        dtype = np.int32 if k.endswith("cls") else np.float64
        out[k] = np.ascontiguousarray(np.concatenate(v)) if v else np.zeros(shape, dtype)
    for pre, cnt in (("gt_", g_cnt), ("dt_", d_cnt)):
        c = np.concatenate(cnt) if cnt else np.zeros(0, np.int64)
        out[pre + "off"] = np.concatenate([[0], np.cumsum(c)]).astype(np.int64)
    out["n_img"] = len(out["gt_off"]) - 1
    out["n_results"] = n_results
    return out


def coco_eval_packed(p, n_cls, device=None):
    """COCOeval.evaluate() + accumulate() of packed windows on the GPU -> (precision (10, 101, K, 4, 3),
    recall (10, K, 4, 3)) as float64 numpy arrays.  Runs on the current torch stream of ``device``."""
    import ctypes as C

    from . import _lib
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    n_img, n_gt, n_dt = int(p["n_img"]), len(p["gt_area"]), len(p["dt_area"])
    nbytes = int(lib.frlw_coco_workspace_bytes(n_img, n_gt, n_dt, n_cls))
    if nbytes <= 0:
        raise ValueError(f"frlw_coco_eval: unsupported sizes (images {n_img}, ground truths {n_gt}, detections {n_dt}, "
                         f"classes {n_cls})")

    def d(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    t = {k: d(p[k]) for k in ("gt_box", "gt_area", "gt_cls", "gt_off", "dt_box", "dt_area", "dt_score", "dt_cls", "dt_off")}
    thr, rec = d(IOU_THRS), d(REC_THRS)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    precision = torch.empty((len(IOU_THRS), len(REC_THRS), n_cls, len(AREA_RNG), len(MAX_DETS)), dtype=torch.float64, device=dev)
    recall = torch.empty((len(IOU_THRS), n_cls, len(AREA_RNG), len(MAX_DETS)), dtype=torch.float64, device=dev)
    ptr = {k: v.data_ptr() for k, v in t.items()}
    _lib.check(lib.frlw_coco_eval(ptr["gt_box"], ptr["gt_area"], ptr["gt_cls"], ptr["gt_off"], n_gt,
                                  ptr["dt_box"], ptr["dt_area"], ptr["dt_score"], ptr["dt_cls"], ptr["dt_off"], n_dt,
                                  n_img, n_cls, thr.data_ptr(), rec.data_ptr(), ws.data_ptr(), C.c_int64(nbytes),
                                  precision.data_ptr(), recall.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
               "frlw_coco_eval")
    return precision.cpu().numpy(), recall.cpu().numpy()


def stats_of(precision, recall):
    """COCOeval.summarize()'s 12 numbers: the mean of the selected entries > -1, else -1."""
    def one(ap, iou_thr=None, area="all", max_dets=100):
        aind = [i for i, lbl in enumerate(AREA_LBL) if lbl == area]
        mind = [i for i, m in enumerate(MAX_DETS) if m == max_dets]
        s = precision if ap else recall
        if iou_thr is not None:
            s = s[np.where(iou_thr == IOU_THRS)[0]]
        s = s[:, :, :, aind, mind] if ap else s[:, :, aind, mind]
        return -1.0 if len(s[s > -1]) == 0 else float(np.mean(s[s > -1]))
    return np.array([one(1), one(1, .5), one(1, .75), one(1, area="small"), one(1, area="medium"), one(1, area="large"),
                     one(0, max_dets=1), one(0, max_dets=10), one(0), one(0, area="small"), one(0, area="medium"),
                     one(0, area="large")])


_SUMMARY = [(1, None, "all", 100), (1, .5, "all", 100), (1, .75, "all", 100), (1, None, "small", 100),
            (1, None, "medium", 100), (1, None, "large", 100), (0, None, "all", 1), (0, None, "all", 10),
            (0, None, "all", 100), (0, None, "small", 100), (0, None, "medium", 100), (0, None, "large", 100)]


def summary_lines(stats):
    """The 12 lines COCOeval.summarize() prints."""
    fmt = " {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}"
    lines = []
    for v, (ap, thr, area, md) in zip(stats, _SUMMARY):
        iou = "{:0.2f}:{:0.2f}".format(IOU_THRS[0], IOU_THRS[-1]) if thr is None else "{:0.2f}".format(thr)
        lines.append(fmt.format("Average Precision" if ap else "Average Recall", "(AP)" if ap else "(AR)", iou, area, md, v))
    return lines


def summarize(stats):
    for line in summary_lines(stats):
        print(line)


def coco_eval_arrays(gt_boxes_list, dt_boxes_list, classes=("car", "pedestrian"), height=240, width=304, time_tol=50000):
    """The inputs of ``evaluate_detection`` -> (precision (10, 101, K, 4, 3), recall (10, K, 4, 3), stats (12,)), laid
    out like COCOeval.eval['precision'] / ['recall'] / .stats."""
    n_cls = len(classes)
    p = pack(gt_boxes_list, dt_boxes_list, n_cls, time_tol)
    if p["n_results"] == 0:  # COCO.loadRes indexes the first result
        raise ValueError("evaluate_detection: no detection in any window (pycocotools' loadRes needs at least one)")
    precision, recall = coco_eval_packed(p, n_cls)
    return precision, recall, stats_of(precision, recall)


def evaluate_detection(gt_boxes_list, dt_boxes_list, classes=("car", "pedestrian"), height=240, width=304, time_tol=50000):
    """coco_eval.py:15-44 -> (AP, AP50, AP75, AP_small, AP_medium, AP_large) as Python floats.  Prints nothing (the
    reference's pycocotools prints the summary on every rank): ``summarize(coco_eval_arrays(...)[2])`` prints it."""
    _, _, stats = coco_eval_arrays(gt_boxes_list, dt_boxes_list, classes, height, width, time_tol)
    return tuple(float(s) for s in stats[:6])
