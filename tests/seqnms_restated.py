"""Seq-NMS restated in plain numpy / Python, with the ``isolated`` switch: what the GPU kernels are held to, bit for bit.  In
``stop`` mode it is itself held to the reference's answers (tests/golden/seqnms.npz, tests/test_seq_nms_cpu.py).

Everything is recomputed from scratch in every round: the edge matrices are the only state besides the scores.  float64 throughout,
every operation rounded on its own, in the reference's order (``score + best``, ``area_i + area_j - iw * ih``, ``sum / len``).
"""
import numpy as np


def areas_of(boxes):
    return (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])


def overlaps(box, boxes, areas):
    """IoU of one box against ``boxes`` whose areas are given: 0 unless both extents of the intersection are > 0."""
    iw = np.minimum(box[2], boxes[:, 2]) - np.maximum(box[0], boxes[:, 0])
    ih = np.minimum(box[3], boxes[:, 3]) - np.maximum(box[1], boxes[:, 1])
    ua = (box[2] - box[0]) * (box[3] - box[1]) + areas - iw * ih
    with np.errstate(all="ignore"):
        iou = iw * ih / ua
    return np.where((iw > 0) & (ih > 0), iou, 0.0)


def split(frames):
    """``(n, 6)`` frames -> per frame (boxes float64 widened from float32, scores float64, labels int32)."""
    boxes, scores, labels = [], [], []
    for fr in frames:
        a = np.asarray(fr, dtype=np.float64).reshape(-1, 6)
        boxes.append(a[:, :4].astype(np.float32).astype(np.float64))
        scores.append(a[:, 4].copy())
        labels.append(a[:, 5].astype(np.int32))
    return boxes, scores, labels


def link(boxes, labels, link_thr):
    """edges[f][i, j]: box i of frame f has an edge to box j of frame f + 1."""
    edges = []
    for f in range(len(boxes) - 1):
        nxt = areas_of(boxes[f + 1])
        e = np.zeros((len(boxes[f]), len(boxes[f + 1])), bool)
        for i, box in enumerate(boxes[f]):
            e[i] = (overlaps(box, boxes[f + 1], nxt) >= link_thr) & (labels[f][i] == labels[f + 1])
        edges.append(e)
    return edges


def best_sequence(edges, scores, skip):
    """-> (start frame, path, sum) of the best root, or (0, [], 0.0) when no root beats 0.  ``skip``: a root without an out-edge
    is no candidate."""
    F = len(scores)
    val = [None] * F
    succ = [None] * F
    val[F - 1] = scores[F - 1].copy()
    succ[F - 1] = np.full(len(scores[F - 1]), -1)
    for f in range(F - 2, -1, -1):
        val[f] = scores[f].copy()
        succ[f] = np.full(len(scores[f]), -1)
        for i in range(len(scores[f])):
            js = np.flatnonzero(edges[f][i])
            if len(js):
                k = js[int(np.argmax(val[f + 1][js]))]   # the first maximum: the lowest j
                val[f][i] = scores[f][i] + val[f + 1][k]
                succ[f][i] = k
    best, start, at = 0.0, 0, -1
    for f in range(F):
        for i in range(len(scores[f])):
            if f > 0 and edges[f - 1][:, i].any():
                continue
            if skip and succ[f][i] < 0:
                continue
            if val[f][i] > best:   # strict: ties stay with the lowest frame, then the lowest box
                best, start, at = val[f][i], f, i
    if at < 0:
        return 0, [], 0.0
    path = [at]
    while succ[start + len(path) - 1][path[-1]] >= 0:
        path.append(int(succ[start + len(path) - 1][path[-1]]))
    return start, path, best


def seq_nms(frames, link_thr=0.5, nms_thr=0.3, metric="avg", isolated="stop", max_sequences=65536):
    """-> (per frame (scores float64, seq int32, suppressed bool), selections [(start frame, path, sum)], truncated)."""
    boxes, scores, labels = split(frames)
    F = len(boxes)
    seq = [np.zeros(len(s), np.int32) for s in scores]
    sup = [np.zeros(len(s), bool) for s in scores]
    selections, truncated = [], False
    if F == 0:
        return [], selections, truncated
    edges = link(boxes, labels, link_thr)
    while True:
        start, path, total = best_sequence(edges, scores, isolated == "skip")
        if len(path) <= 1:
            break
        selections.append((start, list(path), float(total)))
        if metric == "avg":
            new = total / len(path)
        else:
            new = 0.0
            for k, i in enumerate(path):
                if scores[start + k][i] > new:
                    new = scores[start + k][i]
        for k, i in enumerate(path):
            f = start + k
            scores[f][i] = new
            seq[f][i] = len(selections)
            gone = overlaps(boxes[f][i], boxes[f], areas_of(boxes[f])) >= nms_thr   # every class, the box itself included
            sup[f] |= gone & (np.arange(len(gone)) != i)
            if f < F - 1:
                edges[f][gone, :] = False
            if f > 0:
                edges[f - 1][:, gone] = False
        if len(selections) >= max_sequences:
            truncated = True
            break
    return list(zip(scores, seq, sup)), selections, truncated
