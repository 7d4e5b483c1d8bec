"""Motion-level evaluation -- mAP as a function of how fast the objects move (the reference's README 4.2, 5.1 step 1 and 5.2:
``generate_opticalflow.py``, ``motion_level_statistics_gt.py``, ``motion_level_statistics_dt.py``, ``motion_level_evaluation.py``).

* ``time_surface_pairs``: the two time surfaces TV-L1 is run on, for every label window of a file in one launch sequence
  (``frlw_time_surface_batch``, csrc/motion.hip), byte for byte what ``generate_timesurface`` + ``.astype(np.uint8)`` give.  The
  TV-L1 solver is by default the third-party call it is in the reference (``cv2.optflow``).
* ``tvl1_flow``: the native Dual TV-L1 solver (``frlw_tvl1_flow_batch``, csrc/tvl1.hip) on the pairs where they lie in HBM,
  opt-in through ``generate_opticalflow(..., solver="native")`` / ``-solver native``: its agreement with OpenCV is unmeasured.
* ``isolated_boxes`` / ``clamp_boxes`` / ``box_flow_density``: per box the mean flow magnitude, the magnitude sum on the GPU
  (``frlw_box_flow_sums``); ``statistics_gt`` / ``statistics_dt`` write the reference's two ``.npz`` files.
* ``motion_level_map``: five density buckets, the Prophesee box filters, the COCO scorer -> five mAP values.

Two deliberate deviations: ``statistics_dt`` raises ``FileNotFoundError`` where ``summarise.npz`` is missing (the reference calls
``os.mkdir`` on that path and then fails to load the directory); ``motion_level_map`` answers -1.0, COCO's "nothing to score", for a
bucket that holds no ground truth in any file (the reference hands pycocotools an empty result list, which raises).
"""
from __future__ import annotations

import argparse
import ctypes as C
import os

import numpy as np
import torch
from numpy.lib import recfunctions as rfn

from . import _lib, dat_io
from . import event_representation as er
from .dataset import GEN1_CLASSES, GEN4_CLASSES
from .evaluator import filter_boxes_gen1, filter_boxes_large
from .settings import MOTION_LEVEL_EDGES

SHAPES = {"gen1": (240, 304), "gen4": (720, 1280)}   # every other -dataset value counts as gen4, as in the scripts
FLOW_WINDOW = 500000   # generate_opticalflow.py:106,110
CUT = 50000            # :79,83
TOL = 4999             # motion_level_statistics_dt.py:51, motion_level_evaluation.py:22
FLOW_GROUP_BYTES = 256 << 20   # flows uploaded per box-sum call (a 1280x720 flow is 7 MB)
TVL1_GROUP_BYTES = 1 << 30     # workspace of one tvl1_flow call (a 1280x720 pair asks for 87 MB, a GEN1 pair for 7 MB)
SOLVERS = ("cv2", "native")


def _shape(dataset):
    return SHAPES["gen1" if dataset == "gen1" else "gen4"]


# ------------------------------------------------------------------------------------------------
# 1. time-surface pairs
# ------------------------------------------------------------------------------------------------
def time_surface_numpy(records, shape):
    """generate_opticalflow.py:176-187 and generate_timesurface (:72-92) in numpy, for the DAT records of ONE window -> the uint8
    pair ``(2, H, W)``.  The per-event loop is an indexed assignment (for a repeated index numpy keeps the last value, the loop's
    last writer); every other statement is the script's, in its order, so numpy's own division and cast decide a window whose
    events span 50 ms or less."""
    H, W = int(shape[0]), int(shape[1])
    rec = np.asarray(records)
    w = rec["_"].astype(np.uint32)
    events = np.stack([w & 16383, (w >> 14) & 16383, rec["t"], (w >> 28) & 1], axis=1).astype(float)
    events = events[(events[:, 0] < W) & (events[:, 1] < H)]
    volume1, volume2 = np.zeros((H, W)), np.zeros((H, W))
    if len(events) > 0:
        end_stamp = events[:, 2].max()
        start_stamp = events[:, 2].min()
        x, y, t = events[:, 0].astype(np.int64), events[:, 1].astype(np.int64), events[:, 2]
        early = t < end_stamp - CUT
        volume1[y[early], x[early]] = t[early]
        volume2[y, x] = t
        with np.errstate(all="ignore"):
            volume1 = volume1 - start_stamp
            volume2 = volume2 - start_stamp - CUT
            volume1 = volume1 / (end_stamp - CUT - start_stamp) * 255
            volume2 = volume2 / (end_stamp - CUT - start_stamp) * 255
            volume1 = np.where(volume1 < 0, 0, volume1)
            volume2 = np.where(volume2 < 0, 0, volume2)
    with np.errstate(all="ignore"):
        return np.stack([volume1.astype(np.uint8), volume2.astype(np.uint8)])


def motion_counts():
    """Calls the library has served in this process: (frlw_time_surface_batch, frlw_box_flow_sums)."""
    c = (C.c_uint64 * 2)()
    _lib.check(_lib.load().frlw_motion_counts(c), "frlw_motion_counts")
    return int(c[0]), int(c[1])


def time_surface_pairs(dat, ranges, shape, check=True):
    """The time-surface pairs of the record windows ``ranges[i] = (lo, hi)`` of the raw DAT tensor ``dat`` (on the GPU): returns
    ``(pairs, tally)``, ``pairs`` a ``(n, 2, H, W)`` uint8 CUDA tensor -- ``volume1.astype(np.uint8), volume2.astype(np.uint8)`` of
    generate_opticalflow.py:187 per window -- and ``tally = {"calls": device calls, "host_windows": windows computed in numpy}``.
    Windows may overlap, nest or be empty; more than 64 take several calls.  A window whose in-bounds events span 50 ms or less
    (``den <= 0``) is computed by ``time_surface_numpy`` from the records copied back: the device reports every window's stamp
    range, which is read once per call (one synchronisation).  ``check``: also read the status word of the call."""
    H, W = int(shape[0]), int(shape[1])
    n = er._records(dat)
    rng = er._ranges(ranges, n)   # any number of them: cut into calls of 64 below
    d, desc = er._events_dat(dat)
    lib = _lib.load()
    out = torch.empty((len(rng), 2, H, W), dtype=torch.uint8, device=d.device)
    tally = {"calls": 0, "host_windows": 0}
    for b0 in range(0, len(rng), _lib.MAX_SEQUENCES):
        part = rng[b0:b0 + _lib.MAX_SEQUENCES]
        B = len(part)
        need = lib.frlw_time_surface_workspace_bytes(n, B, H, W)
        if need == 0:
            raise NotImplementedError("shape outside the time-surface path")
        ws = er._slot_workspace(need, d.device, "time_surface")
        stamps = torch.empty((B, 2), dtype=torch.int64, device=d.device)
        pairs = out[b0:b0 + B]
        rc = lib.frlw_time_surface_batch(C.byref(desc), (C.c_int64 * B)(*[r[0] for r in part]), (C.c_int64 * B)(*[r[1] for r in part]),
                                         B, H, W, er._ptr(pairs), er._ptr(stamps), er._ptr(ws), ws.numel(), er._stream())
        er._run(rc, "time_surface_pairs", ws, check, "input outside the time-surface path")
        tally["calls"] += 1
        st = stamps.cpu().numpy()
        for i in np.flatnonzero((st[:, 1] >= 0) & (st[:, 1] - CUT - st[:, 0] <= 0)):
            lo, hi = part[i]
            host = d.view(torch.uint8).reshape(-1, 8)[lo:hi].cpu().numpy().view(dat_io.DAT_DTYPE).reshape(-1)
            pairs[i].copy_(torch.from_numpy(time_surface_numpy(host, (H, W))))
            tally["host_windows"] += 1
    return out, tally


_TVL1_WORKSPACES = {}


def tvl1_counts():
    """(calls of frlw_tvl1_flow_batch served, kernel launches they enqueued) in this process."""
    c = (C.c_uint64 * 2)()
    _lib.check(_lib.load().frlw_tvl1_counts(c), "frlw_tvl1_counts")
    return int(c[0]), int(c[1])


def tvl1_plan(shape, nscales=5, scale_step=0.8):
    """``frlw_tvl1_plan``: the level shapes of the solver's pyramid, the full frame first; [] = a side below 16."""
    hw = (C.c_int * (2 * _lib.TVL1_MAX_LEVELS))()
    n = _lib.load().frlw_tvl1_plan(int(shape[0]), int(shape[1]), int(nscales), float(scale_step), hw)
    return [(int(hw[2 * i]), int(hw[2 * i + 1])) for i in range(n)]


def tvl1_flow(pairs, params=None, return_iters=False):
    """Dual TV-L1 flow of every pair of ``pairs``, a ``(n, 2, H, W)`` uint8 CUDA tensor as ``time_surface_pairs`` returns it ->
    ``(n, H, W, 2)`` float32 on the same device, ``[..., 0]`` the x component: what ``box_flow_sums`` reads, no copy in between.
    ``params``: a dict of ``_lib.FrlwTvl1Params.DEFAULTS`` overrides (OpenCV's defaults when None).  Any ``n``: the pairs go out in
    groups of at most 64 whose workspace stays under TVL1_GROUP_BYTES.  ``return_iters``: also the ``(n, levels, warps)`` int32
    tensor of inner iterations run (level 0 = the full frame).  A pair's flow does not depend on its group or its place in it."""
    if not torch.is_tensor(pairs) or not pairs.is_cuda:
        raise ValueError("pairs must be a CUDA tensor")
    if pairs.dtype != torch.uint8 or pairs.dim() != 4 or pairs.shape[1] != 2:
        raise ValueError("pairs must be a (n, 2, H, W) uint8 tensor")
    n, H, W = int(pairs.shape[0]), int(pairs.shape[2]), int(pairs.shape[3])
    if H < 16 or W < 16:
        raise ValueError(f"a {H} x {W} frame has a side below 16: no pyramid level")
    prm = _lib.FrlwTvl1Params(**(params or {}))
    lib = _lib.load()
    levels = len(tvl1_plan((H, W), prm.nscales, prm.scale_step))
    one = lib.frlw_tvl1_workspace_bytes(1, H, W, C.byref(prm))
    if one == 0 or levels == 0:
        raise ValueError("parameters or shape outside the TV-L1 path")
    group = _lib.MAX_SEQUENCES
    while group > 1 and lib.frlw_tvl1_workspace_bytes(group, H, W, C.byref(prm)) > TVL1_GROUP_BYTES:
        group -= 1
    p = pairs.contiguous()
    flows = torch.empty((n, H, W, 2), dtype=torch.float32, device=p.device)
    iters = torch.empty((n, levels, prm.warps), dtype=torch.int32, device=p.device) if return_iters else None
    for b0 in range(0, n, group):
        B = min(group, n - b0)
        need = lib.frlw_tvl1_workspace_bytes(B, H, W, C.byref(prm))
        key = (p.device.index, torch.cuda.current_stream().cuda_stream)
        ws = _TVL1_WORKSPACES.get(key)
        if ws is None or ws.numel() < need:   # (no encoder header in this workspace: a plain buffer, kept per device and stream)
            ws = _TVL1_WORKSPACES[key] = torch.empty(need, dtype=torch.uint8, device=p.device)
        _lib.check(lib.frlw_tvl1_flow_batch(er._ptr(p[b0:b0 + B]), B, H, W, C.byref(prm), er._ptr(flows[b0:b0 + B]),
                                            er._ptr(iters[b0:b0 + B]) if return_iters else None, er._ptr(ws), ws.numel(), er._stream()),
                   "frlw_tvl1_flow_batch")
    return (flows, iters) if return_iters else flows


# ------------------------------------------------------------------------------------------------
# 2. box statistics
# ------------------------------------------------------------------------------------------------
def isolated_boxes(rows):
    """The scripts' ``nms`` (motion_level_statistics_gt.py:12-43) on rows whose columns 1..4 are corners, in the rows' own dtype ->
    the kept indices.  Not a score NMS: a box that overlaps a LATER one by more than 0.1 is removed together with every box it
    overlaps, so only boxes that stand alone are kept."""
    x1, y1, x2, y2 = rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4]
    areas = (x2 - x1) * (y2 - y1)
    order = np.arange(len(rows))
    keep = []
    while order.size > 0:
        i = order[0]
        keep.append(i)
        xx1 = np.maximum(x1[i], x1[order[1:]])
        yy1 = np.maximum(y1[i], y1[order[1:]])
        xx2 = np.minimum(x2[i], x2[order[1:]])
        yy2 = np.minimum(y2[i], y2[order[1:]])
        w = np.maximum(1e-28, xx2 - xx1)
        h = np.maximum(1e-28, yy2 - yy1)
        inter = w * h
        ovr = inter / (areas[i] + areas[order[1:]] - inter)
        inds = np.where(ovr <= 0.1)[0]
        if len(inds) != len(ovr):
            keep.pop()
        order = order[inds + 1]
    return keep


def clamp_boxes(rows, shape):
    """The scripts' chain of comparisons (motion_level_statistics_gt.py:103-127) on rows ``[t, x, y, w, h, ...]``, literally and in
    the rows' own dtype: ``x1`` / ``x2`` at or beyond ``W`` become ``W - 1``, below 0 become 0, ``y`` likewise with ``H``.  Returns
    ``(rows rewritten as x1, y1, x2 - x1, y2 - y1, corners)``; ``corners`` is ``(n, 4)`` float64 ``[x1, y1, x2, y2]`` (``x2`` cannot
    be had back from ``x1 + (x2 - x1)`` in floating point, and ``box_flow_density`` slices by ``int(x2)``)."""
    H, W = int(shape[0]), int(shape[1])
    out = np.array(rows, copy=True)
    corners = np.zeros((len(out), 4), np.float64)
    for j in range(len(out)):
        x1, y1, x2, y2 = out[j, 1], out[j, 2], out[j, 3] + out[j, 1], out[j, 4] + out[j, 2]
        if x1 >= W:
            x1 = W - 1
        if x1 < 0:
            x1 = 0
        if x2 >= W:
            x2 = W - 1
        if x2 < 0:
            x2 = 0
        if y1 >= H:
            y1 = H - 1
        if y1 < 0:
            y1 = 0
        if y2 >= H:
            y2 = H - 1
        if y2 < 0:
            y2 = 0
        out[j, 1] = x1
        out[j, 2] = y1
        out[j, 3] = x2 - x1
        out[j, 4] = y2 - y1
        corners[j] = (x1, y1, x2, y2)
    return out, corners


def integer_boxes(rows, corners, flow_index):
    """What the density statement (motion_level_statistics_gt.py:130) makes of clamped rows: the slice
    ``[int(y1):int(y2), int(x1):int(x2)]`` as int32 rows ``[flow index, x0, x1, y0, y1]`` and the divisor
    ``int(y2 - y1) * int(x2 - x1) + 1e-8`` -- the differences as the rows hold them (taken in the rows' dtype), NOT the slice's
    pixel count: ``int(y2 - y1)`` and ``int(y2) - int(y1)`` differ for fractional boxes."""
    n = len(rows)
    boxes = np.zeros((n, 5), np.int32)
    div = np.zeros(n, np.float64)
    flow_index = np.broadcast_to(np.asarray(flow_index, dtype=np.int64), (n,))
    for j in range(n):
        x1, y1, x2, y2 = (corners[j, k] for k in range(4))
        boxes[j] = (flow_index[j], int(x1), int(x2), int(y1), int(y2))
        div[j] = int(rows[j, 4]) * int(rows[j, 3]) + 1e-8
    return boxes, div


def box_flow_sums(flows, boxes):
    """``frlw_box_flow_sums``: ``flows`` ``(T, H, W, 2)`` float32 on the GPU, ``boxes`` ``(N, 5)`` int32 ``[flow, x0, x1, y0, y1]``
    (numpy or tensor) -> ``(N,)`` float64 CUDA tensor of magnitude sums.  A non-empty box must lie inside the frame and name a
    flow of the batch (``ValueError``)."""
    if not flows.is_cuda or flows.dtype != torch.float32 or flows.dim() != 4 or flows.shape[3] != 2:
        raise ValueError("flows must be a (T, H, W, 2) float32 CUDA tensor")
    f = flows.contiguous()
    T, H, W = int(f.shape[0]), int(f.shape[1]), int(f.shape[2])
    b = boxes.cpu().numpy() if torch.is_tensor(boxes) else np.asarray(boxes)
    b = np.ascontiguousarray(b, dtype=np.int32).reshape(-1, 5)
    full = (b[:, 1] < b[:, 2]) & (b[:, 3] < b[:, 4])
    bad = full & ((b[:, 0] < 0) | (b[:, 0] >= T) | (b[:, 1] < 0) | (b[:, 3] < 0) | (b[:, 2] > W) | (b[:, 4] > H))
    if bad.any():
        raise ValueError(f"box {b[np.flatnonzero(bad)[0]].tolist()} leaves the {T} flows of {H}x{W}")
    out = torch.empty((len(b),), dtype=torch.float64, device=f.device)
    if len(b):
        bd = torch.from_numpy(b).to(f.device)
        _lib.check(_lib.load().frlw_box_flow_sums(er._ptr(f), T, H, W, er._ptr(bd), len(b), er._ptr(out), er._stream()),
                   "frlw_box_flow_sums")
    return out


def box_flow_density(flows, rows, flow_index, corners):
    """The density of motion_level_statistics_gt.py:130 for clamped ``rows`` / ``corners`` (``clamp_boxes``) on the flows
    ``flows[flow_index]`` (an int or one index per row) -> ``(n,)`` float64 numpy: the magnitude sum of the integer slice from the
    GPU, divided on the host by ``int(y2 - y1) * int(x2 - x1) + 1e-8``."""
    boxes, div = integer_boxes(rows, corners, flow_index)
    return box_flow_sums(flows, boxes).cpu().numpy() / div


def _unstructured_boxes(bbox_file):
    """``rfn.structured_to_unstructured`` of a ``*_bbox.npy`` file, as the statistics scripts read it (:80-86): one float64 row per
    box, the columns in the file's field order."""
    return rfn.structured_to_unstructured(np.load(bbox_file))


def _densities(jobs, flow_path, device):
    """``jobs``: ``(label_time, rows, corners)`` of one file in label order -> the densities, row after row.  The file's flows are
    uploaded in groups of at most FLOW_GROUP_BYTES and each group's boxes go through one ``frlw_box_flow_sums`` call."""
    out, group, held = [], [], 0

    def flush():
        if not group:
            return
        flows = torch.from_numpy(np.stack([g[0] for g in group])).to(device)
        rows = np.concatenate([g[1] for g in group])
        corners = np.concatenate([g[2] for g in group])
        index = np.concatenate([np.full(len(g[1]), k, np.int64) for k, g in enumerate(group)])
        out.extend(box_flow_density(flows, rows, index, corners).tolist())
        del group[:]

    for label_time, rows, corners in jobs:
        flow = np.load(flow_path(label_time))   # a missing flow raises here, as in the scripts -- boxes or not
        if len(rows) == 0:
            continue
        flow = np.ascontiguousarray(flow, dtype=np.float32)
        if group and (held + flow.nbytes > FLOW_GROUP_BYTES or flow.shape != group[0][0].shape):
            flush()
            held = 0
        group.append((flow, rows, corners))
        held += flow.nbytes
    flush()
    return out


def _label_rows(rows, shape):
    """One label's rows ``[t, x, y, w, h, ...]`` -> the isolated ones, clamped (:96-127)."""
    as_corners = rows.copy()
    as_corners[:, 3] = rows[:, 3] + rows[:, 1]
    as_corners[:, 4] = rows[:, 4] + rows[:, 2]
    return clamp_boxes(rows[isolated_boxes(as_corners)], shape)


def statistics_gt(raw_dir, dataset, flow_dir="optical_flow_buffer", out_dir="statistics_result", device="cuda"):
    """motion_level_statistics_gt.py:45-140: every isolated ground-truth box of ``<raw_dir>/test`` with the flow density inside it ->
    ``<out_dir>/gt_<dataset>.npz`` (``file_names``, ``gts``, ``densitys``).  Files, unique label times and boxes in the script's
    order.  Returns the path."""
    shape = _shape(dataset)
    os.makedirs(out_dir, exist_ok=True)
    root = os.path.join(raw_dir, "test")
    files = [name[:-7] for name in os.listdir(root) if name[-3:] == "dat"]
    file_names, gt, densitys = [], [], []
    for file_name in files:
        dat_bbox = _unstructured_boxes(os.path.join(root, file_name + "_bbox.npy"))
        jobs = []
        for unique_time in np.unique(dat_bbox[:, 0]):
            rows, corners = _label_rows(dat_bbox[dat_bbox[:, 0] == unique_time], shape)
            jobs.append((unique_time, rows, corners))
            file_names += [file_name] * len(rows)
            gt += list(rows)
        densitys += _densities(jobs, lambda t: os.path.join(flow_dir, file_name + "_{0}.npy".format(int(t))), device)
    path = os.path.join(out_dir, "gt_" + dataset + ".npz")
    print([np.quantile(densitys, q / 100) for q in range(0, 100, 5)] if densitys else [])
    np.savez(path, file_names=file_names, gts=gt, densitys=densitys)
    return path


def statistics_dt(raw_dir, dataset, exp_name, flow_dir="optical_flow_buffer", log_dir="log", device="cuda"):
    """motion_level_statistics_dt.py:44-152: the recorded detections of ``<log_dir>/<exp_name>/summarise.npz`` within 4999 us of a
    label, isolated, clamped, with their flow density -> ``<log_dir>/<exp_name>/summarise_stats.npz`` (``file_names``, ``dts``,
    ``densitys``).  A missing ``summarise.npz`` raises ``FileNotFoundError`` (the reference makes a directory of that name).
    Returns the path."""
    shape = _shape(dataset)
    result_path = os.path.join(log_dir, exp_name, "summarise.npz")
    if not os.path.exists(result_path):
        raise FileNotFoundError(f"{result_path}: record the detections first (test.py --record)")
    root = os.path.join(raw_dir, "test")
    files = [name[:-9] for name in os.listdir(root) if name[-3:] == "npy"]
    f_bbox = np.load(result_path)
    dts, file_names = f_bbox["dts"], f_bbox["file_names"]
    densitys, file_names2, dt = [], [], []
    for file_name in files:
        gt_bbox = _unstructured_boxes(os.path.join(root, file_name + "_bbox.npy"))
        dt_bbox = dts[file_names == file_name]
        jobs = []
        for unique_time in np.unique(gt_bbox[:, 0]):
            rows, corners = _label_rows(dt_bbox[(dt_bbox[:, 0] >= unique_time - TOL) & (dt_bbox[:, 0] <= unique_time + TOL)], shape)
            jobs.append((unique_time, rows, corners))
            file_names2 += [file_name] * len(rows)
            dt += list(rows)
        densitys += _densities(jobs, lambda t: os.path.join(flow_dir, file_name + "_{0}.npy".format(int(t))), device)
    path = os.path.join(log_dir, exp_name, "summarise_stats.npz")
    np.savez(path, file_names=file_names2, dts=dt, densitys=densitys)
    return path


# ------------------------------------------------------------------------------------------------
# 3. bucketed mAP
# ------------------------------------------------------------------------------------------------
def motion_level_map(stats_dt, stats_gt, dataset, metric_fn=None):
    """motion_level_evaluation.py:38-80 on the contents of ``summarise_stats.npz`` (``stats_dt``: ``dts``, ``file_names``,
    ``densitys``) and ``gt_<dataset>.npz`` (``stats_gt``: ``gts``, ...): per density bucket ``[e[i], e[i + 1])`` of
    ``settings.MOTION_LEVEL_EDGES`` the rows of every file are filtered (``filter_boxes_gen1`` / ``filter_boxes_large``), files
    without ground truth are dropped, a file without a detection gets the one-row placeholder, and the COCO scorer gives the mAP.
    Returns the five values; a bucket without any ground truth gives -1.0.  ``metric_fn``: the scorer,
    ``coco_eval.evaluate_detection`` on the GPU when None.  Prints what the script prints."""
    if metric_fn is None:
        from .coco_eval import evaluate_detection as metric_fn
    gen1 = dataset == "gen1"
    shape = _shape(dataset)
    filter_boxes = filter_boxes_gen1 if gen1 else filter_boxes_large
    classes = GEN1_CLASSES if gen1 else GEN4_CLASSES
    edges = MOTION_LEVEL_EDGES["gen1" if gen1 else "gen4"]
    dts, file_names_dt, densitys_dt = stats_dt["dts"], stats_dt["file_names"], stats_dt["densitys"]
    gts, file_names_gt, densitys_gt = stats_gt["gts"], stats_gt["file_names"], stats_gt["densitys"]
    results = []
    for i in range(len(edges) - 1):
        print(i, edges[i], edges[i + 1])
        gt_list, dt_list = [], []
        for file_name in np.unique(file_names_gt):
            dt_bbox = filter_boxes(dts[(file_names_dt == file_name) & (densitys_dt >= edges[i]) & (densitys_dt < edges[i + 1])])
            gt_bbox = filter_boxes(gts[(file_names_gt == file_name) & (densitys_gt >= edges[i]) & (densitys_gt < edges[i + 1])])
            if len(gt_bbox) > 0:
                gt_list.append(gt_bbox)
                dt_list.append(np.array([[gt_bbox[0, 0], 0, 0, 0, 0, 0, 0, 0]]) if len(dt_bbox) == 0 else dt_bbox)
        if not gt_list:
            results.append(-1.0)
            continue
        results.append(float(metric_fn(gt_list, dt_list, time_tol=TOL, classes=classes, height=shape[0], width=shape[1])[0]))
    print(results)
    return results


# ------------------------------------------------------------------------------------------------
# 4. commands
# ------------------------------------------------------------------------------------------------
def _tvl1():
    """``cv2.optflow.DualTVL1OpticalFlow_create`` where OpenCV's contrib module is installed, else None."""
    try:
        import cv2
        return cv2.optflow.DualTVL1OpticalFlow_create
    except (ImportError, AttributeError):
        return None


def generate_opticalflow(raw_dir, dataset="gen1", flow_dir="optical_flow_buffer", surface_dir="time_surface_buffer", device="cuda",
                         solver=None):
    """generate_opticalflow.py:94-193: per label of ``<raw_dir>/test`` the time-surface pair of the 500 ms in front of it and the
    TV-L1 flow between the two -> ``<flow_dir>/<file>_<t>.npy``.  A file goes to HBM once and its labels through
    ``time_surface_pairs``; labels whose output exists are skipped.  ``solver``: None -- ``cv2.optflow`` where it is installed,
    else the pairs themselves are saved under ``<surface_dir>/<file>_<t>.npy`` for a machine that has it; ``"cv2"`` -- the same
    solver, its absence an error; ``"native"`` -- ``tvl1_flow`` on the pairs where they lie (cv2 is not imported).  Returns the
    number of files written."""
    shape = _shape(dataset)
    if solver not in (None,) + SOLVERS:
        raise ValueError(f"solver must be one of {SOLVERS} or None")
    create = None if solver == "native" else _tvl1()
    if solver == "cv2" and create is None:
        raise SystemExit("-solver cv2: cv2.optflow is not installed (-solver native runs the built-in Dual TV-L1)")
    save_pairs = create is None and solver != "native"
    target = surface_dir if save_pairs else flow_dir
    if save_pairs:
        print(f"cv2.optflow is not installed: saving the time-surface pairs under {surface_dir}/ instead of TV-L1 flows")
    os.makedirs(target, exist_ok=True)
    root = os.path.join(raw_dir, "test")
    n_files = 0
    for file_name in [name[:-7] for name in os.listdir(root) if name[-3:] == "dat"]:
        boxes = np.load(os.path.join(root, file_name + "_bbox.npy"))
        f_event = dat_io.DatFile(os.path.join(root, file_name + "_td.dat"))
        jobs = [(sl["start_count"], sl["end_count"], os.path.join(target, file_name + "_{0}.npy".format(sl["label_time"])))
                for sl in dat_io.flow_label_slices(f_event, np.unique(boxes["t" if "t" in boxes.dtype.names else "ts"]), FLOW_WINDOW)]
        jobs = [j for j in jobs if not os.path.exists(j[2])]
        if not jobs:
            continue
        dat = f_event.to_device(device=device)
        for j0 in range(0, len(jobs), _lib.MAX_SEQUENCES):
            part = jobs[j0:j0 + _lib.MAX_SEQUENCES]
            pairs = time_surface_pairs(dat, [(lo, hi) for lo, hi, _ in part], shape)[0]
            if solver == "native":
                out = tvl1_flow(pairs).cpu().numpy()
            else:
                pairs = pairs.cpu().numpy()
                out = pairs if create is None else [create().calc(pair[0], pair[1], None) for pair in pairs]
            for item, (_, _, path) in zip(out, part):
                np.save(path, item, allow_pickle=True)
                n_files += 1
    return n_files


def _parser(flags, solver=False):
    p = argparse.ArgumentParser(description="visualize one or several event files along with their boxes")
    for flag, default in flags:
        p.add_argument(*flag, type=str, **({} if default is None else {"default": default}))
    if solver:   # not one of the script's own flags: absent = cv2.optflow where installed, else the pairs are saved
        p.add_argument("-solver", choices=SOLVERS, default=None, help="the TV-L1 solver: OpenCV's, or the built-in one (opt-in)")
    return p


PARSERS = {   # the scripts' own flags and defaults
    "generate_opticalflow": lambda: _parser([(("-raw_dir",), None), (("-dataset", "--dataset"), "gen1")], solver=True),
    "motion_level_statistics_gt": lambda: _parser([(("-raw_dir",), None), (("-dataset", "--dataset"), None)]),
    "motion_level_statistics_dt": lambda: _parser([(("-raw_dir",), None), (("-dataset", "--dataset"), "gen1"), (("-exp_name",), None)]),
    "motion_level_evaluation": lambda: _parser([(("-dataset", "--dataset"), "gen1"), (("-exp_name",), None)]),
}


def main(which, argv=None):
    args = PARSERS[which]().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("the motion-level commands run on the GPU: no ROCm device is visible (there is no CPU fallback)")
    if which == "generate_opticalflow":
        print(f"{which}: {generate_opticalflow(args.raw_dir, args.dataset, solver=args.solver)} files written")
    elif which == "motion_level_statistics_gt":
        print(f"{which}: {statistics_gt(args.raw_dir, args.dataset)}")
    elif which == "motion_level_statistics_dt":
        print(f"{which}: {statistics_dt(args.raw_dir, args.dataset, args.exp_name)}")
    else:
        stats_dt = np.load(os.path.join("log", args.exp_name, "summarise_stats.npz"))
        stats_gt = np.load(os.path.join("statistics_result", "gt_" + args.dataset + ".npz"))
        motion_level_map(stats_dt, stats_gt, args.dataset)
