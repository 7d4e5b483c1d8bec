#!/usr/bin/env python3
"""Golden answers of Seq-NMS, produced by RUNNING the reference's ``core/Others/seqnms/seq_nms.py`` on the fabricated cases of
tests/seqnms_data.py (regenerated from seeds on both sides; nothing of the reference is copied).

The reference cannot be called through its front door on this numpy: ``build_box_sequences`` ends in ``np.array(box_graph)``, which
raises on a ragged graph, and ``_seq_nms`` indexes ``keep_ind`` (sized by frame 0) with a box index of another frame.  So

  * the module is loaded with a ``np`` whose ``array`` hands its argument back (everything else is numpy's),
  * the loop is driven here over the reference's own ``find_best_sequence``, ``rescore_sequence`` and ``delete_sequence``, without
    ``keep_ind``,
  * ``compute_overlap`` (a Cython unit) is stood in for by this project's numpy statement of its formulas (``Overlap`` below).

Per case and metric ('avg', 'max'): ``<case>_<metric>_sel`` int64 rows [start frame, length, first box ..., padded with -1],
``<case>_<metric>_sum`` float64 (the selected sums) and ``<case>_<metric>_scores`` float64 (the final scores, frame after frame).

    python tests/golden/make_golden_seqnms.py          # needs /root/reference; rewrites tests/golden/seqnms.npz
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("FRLW_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import seqnms_data  # noqa: E402


class Overlap:
    """The formulas of compute_overlap.pyx in numpy, float64: areas without + 1; an overlap is 0 unless iw > 0 and ih > 0."""

    @staticmethod
    def compute_area(boxes):
        return (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])

    @staticmethod
    def compute_overlap_areas_given(boxes, query_boxes, query_areas):
        out = np.zeros((len(boxes), len(query_boxes)), np.float64)
        for n, b in enumerate(boxes):
            iw = np.minimum(b[2], query_boxes[:, 2]) - np.maximum(b[0], query_boxes[:, 0])
            ih = np.minimum(b[3], query_boxes[:, 3]) - np.maximum(b[1], query_boxes[:, 1])
            ua = (b[2] - b[0]) * (b[3] - b[1]) + query_areas - iw * ih
            with np.errstate(all="ignore"):
                out[n] = np.where((iw > 0) & (ih > 0), iw * ih / ua, 0.0)
        return out

    @classmethod
    def compute_overlap(cls, boxes, query_boxes):
        return cls.compute_overlap_areas_given(boxes, query_boxes, cls.compute_area(query_boxes))


class NumpyWithPlainArray:
    """numpy, except that ``array`` returns its argument (the ragged edge lists stay lists)."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def array(x, *args, **kw):
        return x


def load_reference():
    pkg = types.ModuleType("ref_seqnms")
    pkg.__path__ = []
    sys.modules["ref_seqnms"] = pkg
    ov = types.ModuleType("ref_seqnms.compute_overlap")
    ov.compute_area, ov.compute_overlap = Overlap.compute_area, Overlap.compute_overlap
    ov.compute_overlap_areas_given = Overlap.compute_overlap_areas_given
    sys.modules["ref_seqnms.compute_overlap"] = ov
    spec = importlib.util.spec_from_file_location("ref_seqnms.seq_nms", os.path.join(REF, "core", "Others", "seqnms", "seq_nms.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["ref_seqnms.seq_nms"] = mod
    spec.loader.exec_module(mod)
    mod.np = NumpyWithPlainArray()
    return mod


def run_reference(mod, frames, metric, link_thr=0.5, nms_thr=0.3):
    boxes = [np.asarray(f[:, :4], dtype=np.float32) for f in frames]
    scores = [np.asarray(f[:, 4], dtype=np.float64).copy() for f in frames]
    labels = [np.asarray(f[:, 5], dtype=np.int32) for f in frames]
    graph = mod.build_box_sequences(boxes, scores, labels, linkage_threshold=link_thr)
    selections = []
    while True:
        start, seq, best = mod.find_best_sequence(graph, scores)
        if len(seq) <= 1:
            break
        selections.append((int(start), [int(i) for i in seq], float(best)))
        mod.rescore_sequence(seq, scores, start, best, score_metric=metric)
        mod.delete_sequence(seq, start, scores, boxes, graph, suppress_threshold=nms_thr)
        assert len(selections) < 10_000
    return selections, scores


def main():
    mod = load_reference()
    out = {}
    for name, frames in seqnms_data.cases().items():
        for metric in ("avg", "max"):
            selections, scores = run_reference(mod, frames, metric)
            width = 2 + max([len(p) for _, p, _ in selections], default=0)
            sel = np.full((len(selections), width), -1, np.int64)
            for k, (start, path, _) in enumerate(selections):
                sel[k, 0], sel[k, 1] = start, len(path)
                sel[k, 2:2 + len(path)] = path
            out[f"{name}_{metric}_sel"] = sel
            out[f"{name}_{metric}_sum"] = np.asarray([s for _, _, s in selections], dtype=np.float64)
            out[f"{name}_{metric}_scores"] = np.concatenate(scores) if scores else np.zeros(0)
            print(name, metric, "frames", len(frames), "boxes", sum(len(f) for f in frames), "sequences", len(selections),
                  "lengths", [len(p) for _, p, _ in selections][:12])
    path = os.path.join(HERE, "seqnms.npz")
    np.savez_compressed(path, **out)
    print(f"seqnms.npz: {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
