#!/usr/bin/env python3
"""Golden vectors of the motion-level evaluation, produced by RUNNING the reference on the fabricated inputs of
tests/motion_data.py (regenerated from seeds on both sides; nothing of the reference is copied):

  * ``PSEELoader.seek_time`` + ``load_delta_t`` as generate_opticalflow.py:171-176 calls them, one loader per file, the cursor
    carried from label to label                                                                   -> slices_<file> [first record, count]
  * ``generate_timesurface`` (generate_opticalflow.py:72-92, loaded with ``runpy`` under a non-main name; ``numba.jit`` stubbed by
    the identity, ``cv2`` by an empty module) behind the harness lines :177-187                   -> surface_pairs, late_pair
  * ``nms`` of motion_level_statistics_gt.py                                                       -> keep_<case>
  * motion_level_statistics_gt.py and motion_level_statistics_dt.py run as ``__main__`` in a temporary working directory
                                                                                                   -> gt_* / dt_* (the arrays of both files)
  * density_bound: the largest relative difference between the reference's densities (float32 numpy sums) and the same statement
    with the magnitude summed in float64 -- the GPU test allows four times that.

    python tests/golden/make_golden_motion.py          # needs /root/reference; rewrites tests/golden/motion.npz
"""
import os
import runpy
import sys
import tempfile
import types

import numpy as np
from numpy.lib import recfunctions as rfn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("FRLW_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
sys.path.insert(0, REF)


def stub(name, **attrs):
    m = sys.modules.get(name) or types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def identity_jit(*args, **kw):
    if len(args) == 1 and callable(args[0]) and not kw:
        return args[0]
    return lambda fn: fn


stub("cv2")
stub("numba", jit=identity_jit)

import motion_data  # noqa: E402
from make_golden_dat import numpy2_shim  # noqa: E402


def reference_pair(generate_timesurface, rec, shape):
    """generate_opticalflow.py:177-187 on the records ``load_delta_t`` would return."""
    events = rfn.structured_to_unstructured(psee_events(rec))[:, [1, 2, 0, 3]].astype(float)
    events = events[(events[:, 0] < shape[1]) & (events[:, 1] < shape[0])]
    volume1, volume2 = np.zeros(shape), np.zeros(shape)
    with np.errstate(all="ignore"):
        volume1, volume2 = generate_timesurface(events, volume1, volume2, 0)
        return np.stack([volume1.astype(np.uint8), volume2.astype(np.uint8)])


def psee_events(rec):
    """Raw DAT records -> the (t, x, y, p) structured array PSEELoader hands out (src/io/dat_events_tools.py:96-98)."""
    out = np.zeros(len(rec), dtype=[("t", "u4"), ("x", "u2"), ("y", "u2"), ("p", "u1")])
    w = rec["_"].astype(np.uint32)
    out["t"] = rec["t"]
    out["x"] = np.bitwise_and(w, 16383)
    out["y"] = np.right_shift(np.bitwise_and(w, 268419072), 14)
    out["p"] = np.right_shift(np.bitwise_and(w, 268435456), 28)
    return out


def run_script(script, argv, cwd):
    old_argv, old_cwd = sys.argv, os.getcwd()
    sys.argv = [script] + argv
    os.chdir(cwd)
    try:
        runpy.run_path(os.path.join(REF, script), run_name="__main__")
    finally:
        sys.argv = old_argv
        os.chdir(old_cwd)


def main():
    from src.io import psee_loader
    numpy2_shim()
    out = {}
    # ---- time surfaces --------------------------------------------------------------------------------------------------
    gen = runpy.run_path(os.path.join(REF, "generate_opticalflow.py"), run_name="reference_generate_opticalflow")["generate_timesurface"]
    rec = motion_data.surface_stream()
    out["surface_pairs"] = np.stack([reference_pair(gen, rec[lo:hi], motion_data.FRAME) for lo, hi in motion_data.surface_windows().values()])
    out["late_pair"] = reference_pair(gen, motion_data.late_stream(), motion_data.FRAME)
    # ---- isolation filter -------------------------------------------------------------------------------------------------
    nms = runpy.run_path(os.path.join(REF, "motion_level_statistics_gt.py"), run_name="reference_statistics_gt")["nms"]
    for name, rows in motion_data.isolation_cases().items():
        out[f"keep_{name}"] = np.asarray(nms(rows), dtype=np.int64)
    # ---- label slices and the two statistics scripts ------------------------------------------------------------------
    with tempfile.TemporaryDirectory() as tmp:
        raw = motion_data.build(tmp)
        for name in motion_data.FILES:
            loader = psee_loader.PSEELoader(os.path.join(raw, "test", name + "_td.dat"))
            rows = []
            for t in motion_data.label_times(name):
                end_time = int(t)
                start_time = end_time - 500000
                loader.seek_time(start_time)
                pos = (loader._file.tell() - loader._start) // loader._ev_size
                rows.append([int(pos), len(loader.load_delta_t(int(end_time - start_time)))])
            out[f"slices_{name}"] = np.asarray(rows, dtype=np.int64)
            del loader
        run_script("motion_level_statistics_gt.py", ["-raw_dir", raw, "-dataset", "gen1"], tmp)
        run_script("motion_level_statistics_dt.py", ["-raw_dir", raw, "-dataset", "gen1", "-exp_name", motion_data.EXP_NAME], tmp)
        gt = np.load(os.path.join(tmp, "statistics_result", "gt_gen1.npz"))
        dt = np.load(os.path.join(tmp, "log", motion_data.EXP_NAME, "summarise_stats.npz"))
        out["gt_file_names"], out["gt_rows"], out["gt_densitys"] = gt["file_names"], gt["gts"], gt["densitys"]
        out["dt_file_names"], out["dt_rows"], out["dt_densitys"] = dt["file_names"], dt["dts"], dt["densitys"]
    # ---- how far numpy's float32 sums lie from the float64 sum of the same magnitudes ---------------------------------
    # (the reference's statement again, only np.sum(..., dtype=float64); the corners come from the product's clamp, which the CPU
    # test pins to the rows above)
    from frlw_evd_amd import motion
    worst = 0.0
    for kind in ("gt", "dt"):
        dens = out[f"{kind}_densitys"]
        want = restated_densities(motion, out[f"{kind}_file_names"], kind)
        assert len(want) == len(dens)
        for a, b in zip(np.asarray(dens, np.float64), want):
            if b != 0:
                worst = max(worst, abs(a - b) / abs(b))
            else:
                assert a == 0
    out["density_bound"] = np.array(worst)
    path = os.path.join(HERE, "motion.npz")
    np.savez_compressed(path, **out)
    print(f"motion.npz: {os.path.getsize(path) / 1024:.0f} KiB; largest relative difference float32 sum vs float64 sum: {worst:.3e}")
    print({k: (v.dtype, v.shape) for k, v in out.items()})
    print("gt densities", np.asarray(out["gt_densitys"], np.float64))
    print("dt densities", np.asarray(out["dt_densitys"], np.float64))


def restated_densities(motion, names, kind):
    """Per row of a statistics file, in its order: the density with a float64 sum.  The rows are walked per file and label as the
    product walks them, so row i here is row i there."""
    out = []
    order = []
    for n in names:
        if n not in order:
            order.append(n)
    det_names, det_rows = motion_data.detections()
    for name in order:
        src = rfn.structured_to_unstructured(motion_data.boxes(name))
        for t in np.unique(src[:, 0]):
            if kind == "gt":
                sel = src[src[:, 0] == t]
            else:
                d = det_rows[det_names == name]
                sel = d[(d[:, 0] >= t - 4999) & (d[:, 0] <= t + 4999)]
            clamped, corners = motion._label_rows(sel, motion_data.SENSOR)
            f = motion_data.flow(name, int(t))
            for r, c in zip(clamped, corners):
                x1, y1, x2, y2 = (int(v) for v in c)
                mag = np.sqrt(f[y1:y2, x1:x2, 0] ** 2 + f[y1:y2, x1:x2, 1] ** 2)
                out.append(np.sum(mag, dtype=np.float64) / (int(r[4]) * int(r[3]) + 1e-8))
    return out


if __name__ == "__main__":
    main()
