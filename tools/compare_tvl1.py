#!/usr/bin/env python3
"""The native Dual TV-L1 solver (``motion.tvl1_flow``) against OpenCV's (``cv2.optflow.DualTVL1OpticalFlow_create().calc``) on the
time-surface pairs of the test dataset's labels (tests/motion_data.py) -- for a machine that has BOTH a GPU and OpenCV's contrib
module; where either is missing the tool says so and measures nothing.  Writes ``profiles/tvl1_vs_opencv.txt``:

  per label and over all labels the endpoint error ||native - OpenCV|| in pixels: median, 90th, 99th percentile and maximum;
  per ground-truth box (isolated and clamped as ``statistics_gt`` does) the flow density of both solvers, their largest absolute
  and relative difference, and the number of boxes whose motion-level bucket (settings.MOTION_LEVEL_EDGES) changes.

Until this has run somewhere, the agreement of the two solvers is UNMEASURED and ``-solver native`` stays opt-in.

``python tools/compare_tvl1.py [--out profiles/tvl1_vs_opencv.txt]``
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tvl1_vs_opencv.txt"))
    args = ap.parse_args()
    import torch
    from frlw_evd_amd import dat_io, motion
    from frlw_evd_amd.settings import MOTION_LEVEL_EDGES
    create = motion._tvl1()
    if create is None:
        raise SystemExit("cv2.optflow is not installed: nothing is measured")
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    import motion_data
    edges = np.asarray(MOTION_LEVEL_EDGES["gen1"])
    lines, all_epe, d_native, d_cv = [f"# tools/compare_tvl1.py on {torch.cuda.get_device_name(0)}"], [], [], []
    with tempfile.TemporaryDirectory() as root:
        raw = motion_data.build(root, with_flows=False)
        for name in motion_data.FILES:
            f_event = dat_io.DatFile(os.path.join(raw, "test", name + "_td.dat"))
            slices = dat_io.flow_label_slices(f_event, motion_data.label_times(name), motion.FLOW_WINDOW)
            pairs = motion.time_surface_pairs(f_event.to_device(device="cuda"), [(s["start_count"], s["end_count"]) for s in slices],
                                              motion_data.SENSOR)[0]
            native = motion.tvl1_flow(pairs)
            host = pairs.cpu().numpy()
            theirs = np.stack([create().calc(p[0], p[1], None) for p in host]).astype(np.float32)
            epe = np.sqrt(((native.cpu().numpy() - theirs) ** 2).sum(-1))
            rows = motion._unstructured_boxes(os.path.join(raw, "test", name + "_bbox.npy"))
            for k, s in enumerate(slices):
                all_epe.append(epe[k].ravel())
                lab, corners = motion._label_rows(rows[rows[:, 0] == s["label_time"]], motion_data.SENSOR)
                if len(lab):
                    d_native += motion.box_flow_density(native, lab, k, corners).tolist()
                    d_cv += motion.box_flow_density(torch.from_numpy(theirs).cuda(), lab, k, corners).tolist()
                lines.append(json.dumps({"file": name, "label": int(s["label_time"]), "epe_median": float(np.median(epe[k])),
                                         "epe_p90": float(np.quantile(epe[k], 0.9)), "epe_p99": float(np.quantile(epe[k], 0.99)),
                                         "epe_max": float(epe[k].max()), "opencv_mean_magnitude": float(np.sqrt((theirs[k] ** 2).sum(-1)).mean())}))
    e = np.concatenate(all_epe)
    a, b = np.asarray(d_native), np.asarray(d_cv)
    moved = int((np.searchsorted(edges, a, side="right") != np.searchsorted(edges, b, side="right")).sum())
    lines.append(json.dumps({"what": "all labels", "epe_median": float(np.median(e)), "epe_p90": float(np.quantile(e, 0.9)),
                             "epe_p99": float(np.quantile(e, 0.99)), "epe_max": float(e.max())}))
    lines.append(json.dumps({"what": "box densities", "boxes": len(a), "largest_abs_difference": float(np.abs(a - b).max()),
                             "largest_rel_difference": float((np.abs(a - b) / np.maximum(np.abs(b), 1e-12)).max()),
                             "boxes_that_change_bucket": moved}))
    print("\n".join(lines))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
