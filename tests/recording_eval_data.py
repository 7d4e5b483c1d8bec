"""What the recording-evaluation tests share: the fabricated dataset of tests/harness_data.py with ``train/seqB`` copied into
``test/`` as a second sequence (so batches cross a file boundary), the sample lists the commands' slicers plan for it, the
entry-point cases with their weight seeds, checkpoints of recipe weights, and -- without any GPU code -- the CPU oracle's volumes of
a case through the torch CPU forward (what test_recording_eval_cpu.py uses to show that the seeds give real boxes).
"""
import os
import shutil

import numpy as np

import harness_data
from frlw_evd_amd import dat_io, generate

SENSOR, TARGET = generate.SHAPES["gen1"]
# DATA_DIR name -> (event_volume_bins, the command of frlw_evd_amd.generate that writes it)
REPRESENTATIONS = {
    "EventVolume250000": (5, "generate_eventvolume"),
    "EventCountImage50000": (1, "generate_eventcountimage"),
    "SurfaceOfActiveEvents1e-05": (1, "generate_surfaceofactiveevents"),
    "SurfaceOfActiveEvents2.5e-06": (1, "generate_surfaceofactiveevents"),   # the second lambda: a channel offset into the chain's volume
    "taf": (8, "generate_taf"),
}
# entry-point cases: experiment, representation, --event_volume_bins, stem, weight seed (and head bias shifts, see recipe_weights).
# They are chosen on the CPU: test_recording_eval_cpu.py::test_cpu_forward_finds_boxes asserts that the oracle's volumes through
# the torch CPU forward of these weights give 1..200 boxes on at least half of the evaluated frames (observed: 54 on each of the
# 7 frames for yolox, 40..50 for yolox_taf_bfm).
ENTRY_CASES = {
    "yolox": dict(exp_type="yolox", exp_class="yolox", representation="EventVolume250000", bins=5, stem="focus", weight_seed=1004,
                  obj_shift=-1.05, wh_shift=1.5),
    "yolox_taf_bfm": dict(exp_type="yolox_taf_bfm", exp_class="yoloxtafBFM", representation="taf", bins=4, stem="bfm", weight_seed=41),
}


def build_dataset(root):
    """(raw_dir, label_dir): tests/harness_data.py's dataset with ``train/seqB`` also under ``test/``."""
    raw, lab = harness_data.build(root)
    shutil.copy(os.path.join(raw, "train", "seqB_td.dat"), os.path.join(raw, "test", "seqB_td.dat"))
    shutil.copy(os.path.join(lab, "train", "seqB_bbox.npy"), os.path.join(lab, "test", "seqB_bbox.npy"))
    return raw, lab


def split_sequences(lab):
    """The sequences of the test split in the order propheseeDataset lists them."""
    return [f[:-9] for f in os.listdir(os.path.join(lab, "test")) if f[-3:] == "npy"]


def slices(raw, lab, name, kind):
    """The label slices the command of ``kind`` plans for one test sequence (``dat_io.*_label_slices``, host arithmetic)."""
    f_event = dat_io.DatFile(os.path.join(raw, "test", name + "_td.dat"))
    times = generate.read_label_times(os.path.join(lab, "test", name + "_bbox.npy"))
    if kind == "taf":
        return f_event, list(dat_io.taf_label_slices(f_event, times, 10000, 8, 50000000))
    if kind == "ev":
        return f_event, list(dat_io.ev_label_slices(f_event, times, [250000, 500000, 1000000]))
    if kind == "eci":
        return f_event, list(dat_io.eci_label_slices(f_event, times, [50000, 100000, 200000]))
    return f_event, list(dat_io.sae_label_slices(f_event, times))


def planned_samples(raw, lab, kind):
    """(sequence, label_time) of every file the command of ``kind`` writes for the test split, in the file route's order."""
    return [(name, sl["label_time"]) for name in split_sequences(lab) for sl in slices(raw, lab, name, kind)[1]]


def recipe_weights(case):
    """(module on the CPU, its state dict): the detector of the case with recipe weights of the case's seed; ``obj_shift`` is added to
    the objectness biases of the head and ``wh_shift`` to its width / height biases.  (The Event Volume's inputs are a few 1/255: with
    the plain recipe every anchor passes obj > 0.3 with a box of a few pixels, which the Prophesee filter drops.)"""
    from frlw_evd_amd.yolox import build_yolox
    from frlw_evd_amd.yolox.model import recipe_state_dict
    net = build_yolox(2 * case["bins"], 2, stem=case["stem"])
    state = recipe_state_dict(net, seed=case["weight_seed"])
    for name in state:
        if name.startswith("head.obj_preds.") and name.endswith(".bias"):
            state[name] = state[name] + case.get("obj_shift", 0.0)
        if name.startswith("head.reg_preds.") and name.endswith(".bias"):
            state[name] = state[name].clone()
            state[name][2:4] += case.get("wh_shift", 0.0)
    return net, state


def build_net(case):
    net, state = recipe_weights(case)
    net.load_state_dict(state)
    return net.eval()


def write_checkpoint(log_root, case, exp_name="R"):
    """``<log_root>/<exp_name>/checkpoints/best_epoch.pth`` with the case's weights, as ``saveCheckpoint`` lays it out."""
    import torch
    path = os.path.join(log_root, exp_name, "checkpoints")
    os.makedirs(path, exist_ok=True)
    state = {"module." + k: v for k, v in recipe_weights(case)[1].items()}
    torch.save({"state_dict": state, "epoch": 0}, os.path.join(path, "best_epoch.pth"))
    return os.path.join(path, "best_epoch.pth")


GEN4_SENSOR, GEN4_TARGET = generate.SHAPES["gen4"]
GEN4_LABELS = [400_000, 700_000, 703_000, 1_000_000, 1_150_000, 1_300_000]   # the last one lies behind the last event


def build_gen4_dataset(root):
    """(raw_dir, label_dir) with one 1 Mpx test sequence of 250 000 events over 1.2 s: the sensor is larger than the detector
    input, so the commands move the events (coordinate maps) and encode at the target shape -- the hand-off does no resize."""
    from frlw_evd_amd import synth
    raw, lab = os.path.join(root, "raw"), os.path.join(root, "label")
    os.makedirs(os.path.join(raw, "test"))
    os.makedirs(os.path.join(lab, "test"))
    H, W = GEN4_SENSOR
    rec = synth.to_dat8(synth.synth_events(5201, 250_000, W, H, 1_200_000, hotspot=True, t_offset=1_000))
    dat_io.write_dat(os.path.join(raw, "test", "seqG_td.dat"), rec, H, W)
    boxes = np.zeros(2 * len(GEN4_LABELS), dtype=harness_data.BBOX_DTYPE)
    boxes["t"] = np.repeat(GEN4_LABELS, 2)
    boxes["x"], boxes["y"], boxes["w"], boxes["h"] = 300, 200, 160, 120
    boxes["class_id"] = np.tile([0, 2], len(GEN4_LABELS))
    boxes["class_confidence"] = 1.0
    np.save(os.path.join(lab, "test", "seqG_bbox.npy"), boxes)
    return raw, lab


def oracle_inputs(raw, lab, case):
    """[(sequence, label_time, float32 (C, 256, 320))]: the detector inputs of the case from the CPU oracle -- encode at the sensor
    shape, uint8, nearest resize, ``/255`` -- for the labels the command plans.  No GPU code."""
    from oracle import oracle as orc
    out = []
    for name in split_sequences(lab):
        if case["representation"] == "taf":
            K = 8
            f_event, sls = slices(raw, lab, name, "taf")
            state, stale = None, 0
            for sl in sls:
                if sl["fresh"]:
                    state = np.full(SENSOR + (2, K), -6000, np.float32)
                stale = stale + 1 if sl["bins"] <= 0 else 0
                if sl["bins"] > 0:
                    view, state = orc.taf_stream_dat8(np.array(f_event.records[sl["start_count"]:sl["end_count"]]), SENSOR, SENSOR, K,
                                                      sl["start_time"], 10000, sl["bins"], state)
                    vol = orc.leaky_transform(view.reshape(K, 2, *SENSOR))
                else:   # the stale volume, transformed again (generate_taf.py:226-227)
                    vol = np.ascontiguousarray(state.transpose(3, 2, 0, 1))
                    for _ in range(1 + stale):
                        vol = orc.leaky_transform(vol)
                u8 = np.ascontiguousarray(orc.quantize_u8(vol)[::-1]).reshape(2 * K, *SENSOR)[:2 * case["bins"]]
                out.append((name, sl["label_time"], u8))
        else:
            tw = int(case["representation"][len("EventVolume"):])
            f_event, sls = slices(raw, lab, name, "ev")
            for sl in sls:
                vol = orc.ev_stream_dat8(np.array(f_event.records[sl["start_count"]:sl["end_count"]]), SENSOR, SENSOR, 5, sl["end_time"], tw)
                out.append((name, sl["label_time"], orc.quantize_u8(vol, clip255=True)))
    return [(name, t, orc.resize_nearest(u8.astype(np.float32), TARGET) / np.float32(255)) for name, t, u8 in out]


def real_rows(rows):
    """Rows of an evaluator list entry that are detections (the all-zero row stands for none)."""
    rows = np.asarray(rows)
    return int((rows[:, 1:7] != 0).any(axis=1).sum())
