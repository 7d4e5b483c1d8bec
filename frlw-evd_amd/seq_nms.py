"""Seq-NMS on the detections of a recording (the reference's ``core/Others/seqnms/seq_nms.py``, which ``YOLOXHead(seq_nms=True)``
would call and ``model.py`` leaves switched off): boxes of neighbouring frames are linked, the best-scoring path is selected again
and again, its boxes are rescored and the boxes it overlaps are cut out of the graph.  The whole loop runs on the GPU
(``frlw_seq_nms``, csrc/seq_nms.hip), float64 in the reference's operation order; DESIGN.md's Seq-NMS section has the rules.

* ``seq_nms``: lists of ``(n, 6)`` frames ``[x1, y1, x2, y2, score, class]`` of one recording or of a batch of recordings.
* ``rescore_frames``: the per-frame rows of ``stream.StreamDetector`` -- confidence rescored, the sequence id written as track.
* ``rescore_records``: the same on a structured ``*_bbox.npy`` array.

Beyond the reference: every selected sequence gets an id (``track``), boxes suppressed by a sequence are flagged, and
``isolated="skip"`` goes on where the reference stops (``"stop"``: as soon as one single box outranks every remaining path).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from . import event_representation as er

METRICS = ("avg", "max")
ISOLATED = ("stop", "skip")
MAX_VIDEOS = _lib.MAX_SEQUENCES
MAX_FRAMES = _lib.SEQ_NMS_MAX_FRAMES
MAX_BOXES = _lib.SEQ_NMS_MAX_BOXES
_WORKSPACES = {}


def _options(link_thr, nms_thr, metric, isolated, max_sequences):
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {METRICS}")
    if isolated not in ISOLATED:
        raise ValueError(f"isolated must be one of {ISOLATED}")
    link_thr, nms_thr, max_sequences = float(link_thr), float(nms_thr), int(max_sequences)
    if not (0.0 < link_thr <= 1.0 and 0.0 < nms_thr <= 1.0):
        raise ValueError("link_thr and nms_thr must lie in (0, 1]")
    if not 1 <= max_sequences < 2 ** 31:
        raise ValueError("max_sequences must be at least 1")
    return link_thr, nms_thr, METRICS.index(metric), ISOLATED.index(isolated), max_sequences


def _is_batch(frames):
    return len(frames) > 0 and isinstance(frames[0], (list, tuple))


def pack(videos):
    """Lists of ``(n, 6)`` frames -> (boxes float32 (T, 4), scores float64 (T,), labels int32 (T,), frame_start int32, video_start
    int32), with the host checks of ``seq_nms``."""
    if not 1 <= len(videos) <= MAX_VIDEOS:
        raise ValueError(f"1..{MAX_VIDEOS} recordings per call")
    rows, counts, vstart = [], [], [0]
    for frames in videos:
        if len(frames) > MAX_FRAMES:
            raise ValueError(f"{len(frames)} frames: at most {MAX_FRAMES} per recording")
        for fr in frames:
            a = np.asarray(fr, dtype=np.float64).reshape(-1, 6)
            if len(a) > MAX_BOXES:
                raise ValueError(f"{len(a)} boxes in a frame: at most {MAX_BOXES}")
            rows.append(a)
            counts.append(len(a))
        vstart.append(len(counts))
    cat = np.concatenate(rows, axis=0) if rows else np.zeros((0, 6))
    if not np.isfinite(cat).all():
        raise ValueError("boxes, scores and classes must be finite")
    if (cat[:, 4] < 0).any():
        raise ValueError("scores must be >= 0")
    fstart = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return (np.ascontiguousarray(cat[:, :4], dtype=np.float32), np.ascontiguousarray(cat[:, 4]), cat[:, 5].astype(np.int32), fstart,
            np.asarray(vstart, dtype=np.int32))


def run_packed(boxes, scores, labels, fstart, vstart, link_thr, nms_thr, metric, isolated, max_sequences, device=None,
               workspace_bytes=None):
    """One ``frlw_seq_nms`` call on packed arrays -> (scores float64, seq int32, flags uint8, status int32 per recording), numpy.
    ``workspace_bytes``: hand the library a workspace of that size instead of what it asks for (tests)."""
    lib = _lib.load()
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    T, NF, NV = len(scores), len(fstart) - 1, len(vstart) - 1
    need = lib.frlw_seq_nms_workspace_bytes(T, NF, NV)
    if need == 0:
        raise ValueError("sizes over the limits of frlw_seq_nms")
    with torch.cuda.device(device):
        if workspace_bytes is None:
            key = (device.index, torch.cuda.current_stream().cuda_stream)
            ws = _WORKSPACES.get(key)
            if ws is None or ws.numel() < need:
                ws = _WORKSPACES[key] = torch.empty(need, dtype=torch.uint8, device=device)
        else:
            ws = torch.empty(max(int(workspace_bytes), 8), dtype=torch.uint8, device=device)
        b = torch.from_numpy(boxes).to(device)
        s = torch.from_numpy(scores).to(device)
        lab = torch.from_numpy(labels).to(device)
        out_s = torch.empty(T, dtype=torch.float64, device=device)
        out_q = torch.empty(T, dtype=torch.int32, device=device)
        out_f = torch.empty(T, dtype=torch.uint8, device=device)
        status = torch.zeros(NV, dtype=torch.int32, device=device)
        fs = np.ascontiguousarray(fstart, dtype=np.int32)
        vs = np.ascontiguousarray(vstart, dtype=np.int32)
        rc = lib.frlw_seq_nms(er._ptr(b) if T else None, er._ptr(s) if T else None, er._ptr(lab) if T else None,
                              fs.ctypes.data_as(C.POINTER(C.c_int32)), vs.ctypes.data_as(C.POINTER(C.c_int32)), NV, link_thr, nms_thr,
                              metric, isolated, max_sequences, er._ptr(out_s) if T else None, er._ptr(out_q) if T else None,
                              er._ptr(out_f) if T else None, er._ptr(status), er._ptr(ws),
                              ws.numel() if workspace_bytes is None else int(workspace_bytes), er._stream())
        _lib.check(rc, "frlw_seq_nms")
        return out_s.cpu().numpy(), out_q.cpu().numpy(), out_f.cpu().numpy(), status.cpu().numpy()


def seq_nms(frames, link_thr=0.5, nms_thr=0.3, metric="avg", isolated="stop", max_sequences=65536, return_status=False):
    """``frames``: a list of ``(n_i, 6)`` arrays ``[x1, y1, x2, y2, score, class]``, one per frame of a recording in time order, or a
    list of such lists for a batch of recordings (one call for all).  Boxes are taken as float32, scores as float64.  Returns per
    frame ``(scores float64, seq int32, suppressed bool)``: the rescored score, the 1-based order of selection of the box's
    sequence (0: none) and whether a sequence the box is not on suppressed it; for a batch, one such list per recording.
    ``ValueError``: a score that is negative or not finite, more than 4096 frames, more than 64 boxes in a frame, more than 64
    recordings.  ``return_status``: also the status word per recording (``_lib.SEQ_NMS_TRUNCATED``: ``max_sequences`` reached)."""
    opts = _options(link_thr, nms_thr, metric, isolated, max_sequences)
    batch = _is_batch(frames)
    videos = list(frames) if batch else [frames]
    if not videos:
        return ([], np.zeros(0, np.int32)) if return_status else []
    boxes, scores, labels, fstart, vstart = pack(videos)
    if len(scores) == 0:
        out_s, out_q, out_f, status = scores, np.zeros(0, np.int32), np.zeros(0, np.uint8), np.zeros(len(videos), np.int32)
    else:
        out_s, out_q, out_f, status = run_packed(boxes, scores, labels, fstart, vstart, *opts)
    res = []
    for v in range(len(videos)):
        per = []
        for f in range(vstart[v], vstart[v + 1]):
            lo, hi = fstart[f], fstart[f + 1]
            per.append((out_s[lo:hi].copy(), out_q[lo:hi].copy(), (out_f[lo:hi] & 1).astype(bool)))
        res.append(per)
    out = res if batch else res[0]
    return (out, status if batch else status[:1]) if return_status else out


def rows_to_frames(rows):
    """``StreamDetector`` rows ``[t, x, y, w, h, class, confidence, track]`` of every frame -> ``(frames, picks)``: the ``(n, 6)``
    float64 frames ``seq_nms`` takes (corners ``x + w``, ``y + h`` in the rows' float32) and per frame the row indices sent -- all of
    them, or in a frame of more than 64 boxes the 64 of highest confidence (ties: the lower index), in row order."""
    frames, picks = [], []
    for r in rows:
        r = np.asarray(r, dtype=np.float32).reshape(-1, 8)
        pick = np.arange(len(r))
        if len(r) > MAX_BOXES:
            pick = np.sort(np.argsort(-r[:, 6], kind="stable")[:MAX_BOXES])
        q = r[pick]
        fr = np.zeros((len(q), 6), np.float64)
        fr[:, 0], fr[:, 1], fr[:, 2], fr[:, 3] = q[:, 1], q[:, 2], q[:, 1] + q[:, 3], q[:, 2] + q[:, 4]
        fr[:, 4], fr[:, 5] = q[:, 6], q[:, 5]
        frames.append(fr)
        picks.append(pick)
    return frames, picks


def apply_to_rows(rows, picks, results, drop_suppressed=False, seq_offset=0):
    """Write ``results`` (``seq_nms``'s per-frame triples for the picked rows) into copies of ``rows``: confidence =
    ``float32(rescored)``, track = the sequence id (``+ seq_offset`` where it is not 0); rows that were not sent keep their
    confidence and get track 0.  ``drop_suppressed``: flagged rows are removed."""
    out = []
    for r, pick, (sc, seq, sup) in zip(rows, picks, results):
        r = np.array(r, dtype=np.float32, copy=True).reshape(-1, 8)
        r[:, 7] = 0
        r[pick, 6] = sc.astype(np.float32)
        r[pick, 7] = np.where(seq > 0, seq + seq_offset, 0)
        if drop_suppressed:
            keep = np.ones(len(r), bool)
            keep[pick] = ~sup
            r = r[keep]
        out.append(r)
    return out


def rescore_frames(rows, link_thr=0.5, nms_thr=0.3, metric="avg", isolated="stop", max_sequences=65536, drop_suppressed=False):
    """``rows``: one ``(n_i, 8)`` float32 array ``[t, x, y, w, h, class, confidence, track]`` per frame, as ``StreamDetector.boxes``
    returns them.  Returns ``(new rows, number of sequences)``.  A recording of more than 4096 frames is processed in stretches of
    4096 whose sequences do not link across the cut; ids go on counting."""
    rows = list(rows)
    out, n_seq = [], 0
    for lo in range(0, len(rows), MAX_FRAMES):
        part = rows[lo:lo + MAX_FRAMES]
        frames, picks = rows_to_frames(part)
        res = seq_nms(frames, link_thr, nms_thr, metric, isolated, max_sequences)
        out += apply_to_rows(part, picks, res, drop_suppressed, n_seq)
        n_seq += max([int(q.max()) for _, q, _ in res if len(q)], default=0)
    return out, n_seq


def rescore_records(rec, stamps=None, **options):
    """The same on a structured ``*_bbox.npy`` array (fields ``t, x, y, w, h, class_id, class_confidence, track_id``), for a
    detection file that already exists.  The records of one ``t`` are one frame; frames follow each other in ascending ``t``.
    ``stamps``: the frame grid, so that a frame without a detection breaks the links across it (without it, the file's own
    timestamps are the frames, and two frames either side of an empty one count as neighbours).  Returns ``(records, number of
    sequences)``; the records keep their order (``drop_suppressed=True`` removes the flagged ones)."""
    rec = np.asarray(rec)
    t = rec["t"].astype(np.int64)
    grid = np.unique(t) if stamps is None else np.asarray(stamps, dtype=np.int64)
    if stamps is not None and (len(np.unique(grid)) != len(grid) or (np.diff(grid) < 0).any() or not np.isin(t, grid).all()):
        raise ValueError("stamps must be ascending, distinct and hold every t of the records")
    order = np.argsort(t, kind="stable")
    first, behind = np.searchsorted(t[order], grid, side="left"), np.searchsorted(t[order], grid, side="right")
    members = [order[a:b] for a, b in zip(first, behind)]
    rows = []
    for m in members:
        r = np.zeros((len(m), 8), np.float32)
        for j, name in enumerate(("x", "y", "w", "h", "class_id", "class_confidence")):
            r[:, j + 1] = rec[name][m]
        rows.append(r)
    drop = bool(options.pop("drop_suppressed", False))
    n_seq = 0
    keep = np.ones(len(rec), bool)
    out = rec.copy()
    for lo in range(0, len(rows), MAX_FRAMES):
        part = rows[lo:lo + MAX_FRAMES]
        frames, picks = rows_to_frames(part)
        res = seq_nms(frames, **options)
        new = apply_to_rows(part, picks, res, False, n_seq)
        for m, r, pick, (_, _, sup) in zip(members[lo:lo + MAX_FRAMES], new, picks, res):
            out["class_confidence"][m] = r[:, 6]
            out["track_id"][m] = r[:, 7].astype(np.uint32)
            if drop:
                keep[m[pick[sup]]] = False
        n_seq += max([int(q.max()) for _, q, _ in res if len(q)], default=0)
    return out[keep], n_seq
