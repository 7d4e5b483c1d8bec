"""A deliberately slow, line-by-line numpy restatement of what the reference's evaluate_detection asks of pycocotools
(COCO.loadRes, COCOeval.evaluate / evaluateImg / accumulate / summarize; iouType 'bbox', default params, no crowd).
It loops per image, category, area range and threshold, and shares no code or data layout with
frlw_evd_amd.coco_eval or csrc/coco_eval.hip: it is the checker the GPU scorer is compared against.
"""
import numpy as np

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
MAX_DETS = [1, 10, 100]


def literal_windows(gt_boxes_list, dt_boxes_list, time_tol):
    gts, dts = [], []
    for gt_boxes, dt_boxes in zip(gt_boxes_list, dt_boxes_list):
        if gt_boxes.shape[0] == 0 or dt_boxes.shape[0] == 0:
            continue
        low_gt = high_gt = low_dt = high_dt = 0
        for ts in np.unique(gt_boxes[:, 0]):
            while low_gt < len(gt_boxes) and gt_boxes[low_gt, 0] < ts:
                low_gt += 1
            high_gt = max(low_gt, high_gt)
            while high_gt < len(gt_boxes) and gt_boxes[high_gt, 0] <= ts:
                high_gt += 1
            low, high = ts - time_tol, ts + time_tol
            while low_dt < len(dt_boxes) and dt_boxes[low_dt, 0] < low:
                low_dt += 1
            high_dt = max(low_dt, high_dt)
            while high_dt < len(dt_boxes) and dt_boxes[high_dt, 0] <= high:
                high_dt += 1
            gts.append(gt_boxes[low_gt:high_gt])
            dts.append(dt_boxes[low_dt:high_dt])
    return gts, dts


def _iou(d, g):
    """maskApi.c bbIou without crowd, one pair."""
    w = min(d[2] + d[0], g[2] + g[0]) - max(d[0], g[0])
    if w <= 0:
        return 0.0
    h = min(d[3] + d[1], g[3] + g[1]) - max(d[1], g[1])
    if h <= 0:
        return 0.0
    i = w * h
    u = d[2] * d[3] + g[2] * g[3] - i
    return i / u


def evaluate_img(gt, dt, a_rng, max_det):
    """COCOeval.evaluateImg for one (image, category, area range).  gt / dt: lists of dicts."""
    if len(gt) == 0 and len(dt) == 0:
        return None
    g_ign = [1 if (g["area"] < a_rng[0] or g["area"] > a_rng[1]) else 0 for g in gt]
    gtind = np.argsort(g_ign, kind="mergesort")
    gt = [gt[i] for i in gtind]
    g_ign = [g_ign[i] for i in gtind]
    dtind = np.argsort([-d["score"] for d in dt], kind="mergesort")
    dt = [dt[i] for i in dtind[0:max_det]]
    T, G, D = len(IOU_THRS), len(gt), len(dt)
    gtm = np.zeros((T, G))
    dtm = np.zeros((T, D))
    dt_ig = np.zeros((T, D))
    ious = [[_iou(d["bbox"], g["bbox"]) for g in gt] for d in dt]
    if G > 0 and D > 0:
        for tind, t in enumerate(IOU_THRS):
            for dind in range(D):
                iou = min([t, 1 - 1e-10])
                m = -1
                for gind in range(G):
                    if gtm[tind, gind] > 0:
                        continue
                    if m > -1 and g_ign[m] == 0 and g_ign[gind] == 1:
                        break
                    if ious[dind][gind] < iou:
                        continue
                    iou = ious[dind][gind]
                    m = gind
                if m == -1:
                    continue
                dt_ig[tind, dind] = g_ign[m]
                dtm[tind, dind] = gt[m]["id"]
                gtm[tind, m] = dt[dind]["id"]
    a = np.array([d["area"] < a_rng[0] or d["area"] > a_rng[1] for d in dt]).reshape((1, D))
    dt_ig = np.logical_or(dt_ig, np.logical_and(dtm == 0, np.repeat(a, T, 0)))
    return {"dtMatches": dtm, "dtScores": [d["score"] for d in dt], "gtIgnore": np.array(g_ign, dtype=np.int64),
            "dtIgnore": dt_ig}


def literal_eval(gt_boxes_list, dt_boxes_list, n_cls, time_tol=50000):
    """-> precision (10, 101, K, 4, 3), recall (10, K, 4, 3), stats (12,)."""
    gts_w, dts_w = literal_windows(gt_boxes_list, dt_boxes_list, time_tol)
    n_img = len(gts_w)
    gt_by = {}
    dt_by = {}
    ann_id = 0
    for im in range(n_img):
        for b in gts_w[im]:
            ann_id += 1
            cat = int(b[5]) + 1
            if 1 <= cat <= n_cls:
                gt_by.setdefault((im, cat), []).append({"id": ann_id, "area": float(b[3] * b[4]),
                                                        "bbox": [float(v) for v in b[1:5]]})
    res_id = 0
    for im in range(n_img):
        for b in dts_w[im]:
            res_id += 1
            cat = int(b[5]) + 1
            if 1 <= cat <= n_cls:
                dt_by.setdefault((im, cat), []).append({"id": res_id, "area": float(b[3] * b[4]), "score": float(b[6]),
                                                        "bbox": [float(v) for v in b[1:5]]})
    if res_id == 0:
        raise ValueError("no results")
    T, R, K, A, M = len(IOU_THRS), len(REC_THRS), n_cls, len(AREA_RNG), len(MAX_DETS)
    # evaluateImg per (category, area, image), cached per (category, area) at maxDets[-1]
    evals = {}
    for k in range(K):
        for a, a_rng in enumerate(AREA_RNG):
            evals[k, a] = [evaluate_img(gt_by.get((im, k + 1), []), dt_by.get((im, k + 1), []), a_rng, MAX_DETS[-1])
                           for im in range(n_img)]
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    for k in range(K):
        for a in range(A):
            for m, max_det in enumerate(MAX_DETS):
                E = [e for e in evals[k, a] if e is not None]
                if len(E) == 0:
                    continue
                dt_scores = np.concatenate([e["dtScores"][0:max_det] for e in E])
                inds = np.argsort(-dt_scores, kind="mergesort")
                dtm = np.concatenate([e["dtMatches"][:, 0:max_det] for e in E], axis=1)[:, inds]
                dt_ig = np.concatenate([e["dtIgnore"][:, 0:max_det] for e in E], axis=1)[:, inds]
                gt_ig = np.concatenate([e["gtIgnore"] for e in E])
                npig = np.count_nonzero(gt_ig == 0)
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dt_ig))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros((R,))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = pr.tolist()
                    q = q.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    idx = np.searchsorted(rc, REC_THRS, side="left")
                    try:
                        for ri, pi in enumerate(idx):
                            q[ri] = pr[pi]
                    except IndexError:
                        pass
                    precision[t, :, k, a, m] = np.array(q)
    return precision, recall, literal_stats(precision, recall)


def literal_stats(precision, recall):
    lbl = ["all", "small", "medium", "large"]

    def summ(ap, iou_thr=None, area="all", max_dets=100):
        aind = [i for i, x in enumerate(lbl) if x == area]
        mind = [i for i, x in enumerate(MAX_DETS) if x == max_dets]
        if ap == 1:
            s = precision
            if iou_thr is not None:
                s = s[np.where(iou_thr == IOU_THRS)[0]]
            s = s[:, :, :, aind, mind]
        else:
            s = recall
            if iou_thr is not None:
                s = s[np.where(iou_thr == IOU_THRS)[0]]
            s = s[:, :, aind, mind]
        return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])

    st = np.zeros((12,))
    st[0] = summ(1)
    st[1] = summ(1, iou_thr=.5)
    st[2] = summ(1, iou_thr=.75)
    st[3] = summ(1, area="small")
    st[4] = summ(1, area="medium")
    st[5] = summ(1, area="large")
    st[6] = summ(0, max_dets=1)
    st[7] = summ(0, max_dets=10)
    st[8] = summ(0, max_dets=100)
    st[9] = summ(0, area="small")
    st[10] = summ(0, area="medium")
    st[11] = summ(0, area="large")
    return st
