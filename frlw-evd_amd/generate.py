"""The four offline pre-processing harnesses of the reference -- the ``__main__`` blocks of ``generate_eventcountimage.py``,
``generate_eventvolume.py``, ``generate_surfaceofactiveevents.py`` and ``generate_taf.py`` -- over the gfx950 encoders:
same command line (``-raw_dir -label_dir -target_dir -dataset``), same walk over ``train / val / test``, same label slicing
(``dat_io.*_label_slices``, pinned to the reference's own ``PSEELoader`` calls), same output tree and file names, and the
same bytes in every file (Event Count Image / Event Volume bit for bit; SAE / TAF within 1 LSB in <= 1e-4 of the bytes --
``exp`` / ``log1p`` come from different math libraries).  Pinned end to end by tests/golden/harness.npz, which the reference's
scripts wrote on a fabricated dataset (tests/golden/make_golden_harness.py).

Each ``*_td.dat`` file goes to HBM ONCE as raw 8-byte records (``DatFile.to_device``); every label is a record range of that
tensor: bit-unpacking, window selection, f64 time normalisation, the coordinate down-scale, encode, nearest resize and uint8
quantisation all run on the device, only the finished uint8 file comes back.

The per-file body of every command is a generator of ``(label_time, uint8 volume on the GPU at the encode shape)`` in label order
(``eci_volumes``, ``ev_volumes``, ``sae_volumes``, ``taf_volumes``); the commands are writers over them, and
``recording_dataset.RecordingLoader`` hands the same volumes to the detector without the files.
"""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch

from . import dat_io
from . import event_representation as er

SHAPES = {"gen4": ((720, 1280), (512, 640)), "gen1": ((240, 304), (256, 320))}  # sensor, detector input (all four scripts)


def _parser(default_dataset):
    p = argparse.ArgumentParser(description="visualize one or several event files along with their boxes")
    p.add_argument("-raw_dir", type=str)      # "train, val, test" level directory of the datasets, data source
    p.add_argument("-label_dir", type=str)    # "train, val, test" level directory of the datasets, annotations
    p.add_argument("-target_dir", type=str)   # output directory
    p.add_argument("-dataset", type=str, default=default_dataset)
    return p


def read_label_times(bbox_file):
    """``np.unique(dat_bbox['t'])`` of a ``*_bbox.npy`` file (generate_taf.py:146-151): an .npy of a structured array whose
    timestamp field is ``t`` (``ts`` in older files, src/io/npy_events_tools.py:57)."""
    boxes = np.load(bbox_file)
    name = "t" if "t" in boxes.dtype.names else "ts"
    return np.unique(boxes[name])


def _sequences(raw_dir, label_dir):
    """(mode, sequence name, event file, bbox file) in the order the reference walks them (generate_taf.py:112-146)."""
    for mode in ("train", "val", "test"):
        file_dir = os.path.join(raw_dir, mode)
        try:
            files = os.listdir(file_dir)
        except Exception:
            continue
        for name in [f[:-7] for f in files if f[-3:] == "dat"]:
            yield mode, name, os.path.join(file_dir, name + "_td.dat"), os.path.join(label_dir, mode, name + "_bbox.npy")


def _geometry(dataset, device):
    shape, target = SHAPES["gen4" if dataset == "gen4" else "gen1"]
    if target[0] < shape[0]:   # down-scale: the events are moved, the encode runs at the target shape (generate_taf.py:216-219)
        xmap, ymap = er.coordinate_maps(shape, target, device)
        return shape, target, target, xmap, ymap
    return shape, target, shape, None, None   # encode natively, then nearest-resize the volume up (:221-222)


def _write(u8, enc_shape, target, path):
    """uint8 volume (C, h, w) at the encode shape -> nearest resize to the target shape (a no-op when equal) -> file."""
    if tuple(enc_shape) != tuple(target):
        u8 = er.resize_nearest(u8, target)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    u8.cpu().numpy().tofile(path)


# ---- generate_eventcountimage.py:66-185 ---------------------------------------------------------------------------------
ECI_EVENTS_WINDOWS = {"gen4": [400000, 800000, 1200000], "gen1": [50000, 100000, 200000]}


def eci_events_windows(dataset):
    return ECI_EVENTS_WINDOWS["gen4" if dataset == "gen4" else "gen1"]


def eci_volumes(f_event, dat, label_times, enc, xmap, ymap, events_windows, select=None):
    """The Event Count Images of one file, in label order: yields ``(label_time, [volume per window of events_windows])``, or
    with ``select=N`` (one of ``events_windows``) ``(label_time, volume of window N)`` -- uint8 (2, h, w) at the encode shape, views
    of the encoder's output on the GPU.  The slices always come from the full window list (the memory the harness keeps depends
    on the largest).  Every (label, window) is a record range of ``dat`` -- the windows of a label are nested, they end at the same
    record -- so the file's ranges go through the batched encoder, up to 64 per call, instead of one call and one
    synchronisation each."""
    if select is not None and select not in events_windows:
        raise ValueError(f"select: one of {list(events_windows)}")
    windows = list(events_windows) if select is None else [select]
    jobs = []   # (lo, hi, label time)
    for sl in dat_io.eci_label_slices(f_event, label_times, events_windows):
        for n in windows:
            jobs.append((max(sl["tail_start"], sl["end_count"] - n), sl["end_count"], sl["label_time"]))
    held = []   # the windows of a label may lie in two calls
    for j0 in range(0, len(jobs), er._lib.MAX_SEQUENCES):
        part = jobs[j0:j0 + er._lib.MAX_SEQUENCES]
        _, u8 = er.encode_eci_batch(dat, [(lo, hi) for lo, hi, _ in part], enc, want_f32=False, want_u8=True, xmap=xmap, ymap=ymap)
        for b, (_, _, label_time) in enumerate(part):
            held.append(u8[b])
            if len(held) == len(windows):
                yield label_time, (held if select is None else held[0])
                held = []


def generate_eventcountimage(raw_dir, label_dir, target_dir, dataset="gen4", device="cuda"):
    events_windows = eci_events_windows(dataset)
    _, target, enc, xmap, ymap = _geometry(dataset, device)
    os.makedirs(target_dir, exist_ok=True)
    n_files = 0
    for mode, name, event_file, bbox_file in _sequences(raw_dir, label_dir):
        f_event = dat_io.DatFile(event_file)
        dat = f_event.to_device(device=device)
        for label_time, vols in eci_volumes(f_event, dat, read_label_times(bbox_file), enc, xmap, ymap, events_windows):
            for n, u8 in zip(events_windows, vols):
                _write(u8, enc, target, os.path.join(target_dir, f"EventCountImage{n}", mode, f"{name}_{label_time}.npy"))
                n_files += 1
    return n_files


# ---- generate_eventvolume.py:63-172 -------------------------------------------------------------------------------------
EV_TIME_WINDOWS = [250000, 500000, 1000000]
# Gathered records per encode_ev_ranges call: the call copies its windows' records (8 bytes each) and partitions the copy (two
# 4-byte record arrays), so 4 M records bound the workspace at about 64 MB plus the per-window tables -- and 64 one-second GEN1
# label windows (some 125 000 events each in the test recordings) still fit one call.  A single window above it goes alone.
EV_RECORD_BUDGET = 4_000_000


def ev_jobs(slices, tw, prefix, times=None):
    """The Event Volume jobs of one file and one time window ``tw``, in label order: ``(lo, hi, end_time, path)`` per slice of
    ``dat_io.ev_label_slices`` -- records ``[lo, hi)``, window end, output file ``<prefix>_<label_time>.npy``.  ``times``: the
    file's time column on the host (time-sorted, as every bisection of ``DatFile`` assumes); with it ``lo`` moves up to the first
    record with ``t > end_time - tw`` -- the encoder drops the records in front of it anyway (:139), so they need not be copied."""
    jobs = []
    for sl in slices:
        lo, hi, end = int(sl["start_count"]), int(sl["end_count"]), int(sl["end_time"])
        if times is not None and end - tw >= 0 and hi > lo:
            lo += int(np.searchsorted(times[lo:hi], end - tw, side="right"))
        jobs.append((lo, hi, end, f"{prefix}_{sl['label_time']}.npy"))
    return jobs


def ev_parts(jobs, max_windows=er._lib.MAX_SEQUENCES, budget=EV_RECORD_BUDGET):
    """``jobs`` cut, in order, into the parts one ``encode_ev_ranges`` call takes: at most ``max_windows`` windows and at most
    ``budget`` gathered records (a single job above the budget is a part of its own)."""
    parts, cur, held = [], [], 0
    for job in jobs:
        n = job[1] - job[0]
        if cur and (len(cur) >= max_windows or held + n > budget):
            parts.append(cur)
            cur, held = [], 0
        cur.append(job)
        held += n
    if cur:
        parts.append(cur)
    return parts


def _eventvolume_loop(dat, part, enc, tw, bins, xmap, ymap):
    """One call and one synchronisation per window: what the command did before encode_ev_ranges, and still does for a part the
    ranged path does not take (a window of 2^20 us or more, a frame with too many tiles, a device that failed the self-test)."""
    # events with t > end_time - tw, t* = (t - (end_time - tw)) / tw (:139-141); > 255 -> 255, uint8 (:155-157)
    return [er.encode_ev_dat(dat[lo:hi], enc, end, tw, bins, want_f32=False, want_u8=True, xmap=xmap, ymap=ymap)[1]
            for lo, hi, end, _ in part]


def ev_volumes(f_event, dat, label_times, enc, xmap, ymap, select, time_windows=EV_TIME_WINDOWS, bins=5, slices=None):
    """The Event Volumes of one file for the time window ``select`` (one of ``time_windows``), in label order: yields
    ``(label_time, uint8 (2 * bins, h, w))`` at the encode shape on the GPU.  The slices always come from the full
    ``time_windows`` (``start_count`` and the 10 M cap depend on the largest); ``slices``: ``list(dat_io.ev_label_slices(...))``
    when the caller has it already.  The label slices of a file overlap (each reaches ``max(time_windows)`` back), so a window
    is a record RANGE of ``dat``: the ranges go through ``encode_ev_ranges``, up to 64 per call, instead of one call and one
    synchronisation each; a part the ranged path does not take runs per window."""
    tw = int(select)
    if tw not in time_windows:
        raise ValueError(f"select: one of {list(time_windows)}")
    if slices is None:
        slices = list(dat_io.ev_label_slices(f_event, label_times, time_windows))
    jobs = [job[:3] + (sl["label_time"],) for job, sl in zip(ev_jobs(slices, tw, "", f_event._t), slices)]
    max_windows = er.ev_ranges_max_windows(enc, tw)
    for part in ev_parts(jobs, max(max_windows, 1)):
        try:
            if max_windows == 0:
                raise NotImplementedError
            _, u8 = er.encode_ev_ranges(dat, [(lo, hi) for lo, hi, _, _ in part], enc, [end for _, _, end, _ in part], tw, bins,
                                        want_f32=False, want_u8=True, xmap=xmap, ymap=ymap)
        except NotImplementedError:
            u8 = _eventvolume_loop(dat, part, enc, tw, bins, xmap, ymap)
        for b, (_, _, _, label_time) in enumerate(part):
            yield label_time, u8[b]


def generate_eventvolume(raw_dir, label_dir, target_dir, dataset="gen1", device="cuda"):
    time_windows = EV_TIME_WINDOWS
    bins = 5
    _, target, enc, xmap, ymap = _geometry(dataset, device)
    os.makedirs(target_dir, exist_ok=True)
    n_files = 0
    for mode, name, event_file, bbox_file in _sequences(raw_dir, label_dir):
        f_event = dat_io.DatFile(event_file)
        dat = f_event.to_device(device=device)
        slices = list(dat_io.ev_label_slices(f_event, read_label_times(bbox_file), time_windows))
        for tw in time_windows:
            for label_time, u8 in ev_volumes(f_event, dat, None, enc, xmap, ymap, tw, time_windows, bins, slices):
                _write(u8, enc, target, os.path.join(target_dir, f"EventVolume{tw}", mode, f"{name}_{label_time}.npy"))
                n_files += 1
    return n_files


# ---- generate_surfaceofactiveevents.py:82-215 ---------------------------------------------------------------------------
SAE_LAMDAS = [0.00001, 0.0000025, 0.000001]
SAE_TIME_WINDOWS = [554126, 2216505, 5541263]


def sae_steps(slices, mode, time_window=SAE_TIME_WINDOWS):
    """The chain of one file, in label order: ``(lo, hi, now, window_us, emit)`` per slice of ``dat_io.sae_label_slices`` and
    window.  The test split runs all of ``time_window`` on a label, each on the memory the previous one left (:178-194), the other
    splits only the largest; ``now`` is the label time, and only the last window of a label emits -- the volume the file keeps
    (:199-200)."""
    windows = list(time_window) if mode == "test" else [max(time_window)]
    steps = []
    for sl in slices:
        for j, tw in enumerate(windows):
            steps.append((int(sl["start_count"]), int(sl["end_count"]), int(sl["label_time"]), int(tw), j == len(windows) - 1))
    return steps


def sae_parts(steps, max_steps=er._lib.MAX_SEQUENCES):
    """``steps`` in parts of at most ``max_steps``, what one ``encode_sae_chain`` call takes (a part may end between the steps of
    one label: the memory carries over)."""
    return [steps[i:i + max_steps] for i in range(0, len(steps), max_steps)]


def sae_volumes(f_event, dat, label_times, mode, enc, xmap, ymap, lamdas=SAE_LAMDAS, select=None):
    """The Surfaces of Active Events of one file, in label order: yields ``(label_time, uint8 (2 * len(lamdas), h, w))`` at the
    encode shape on the GPU -- channels ``2j, 2j + 1`` belong to ``lamdas[j]`` -- or with ``select=lam`` (one of ``lamdas``)
    only those two channels (a view).  The chain always runs all of ``sae_steps(..., mode)`` with all of ``lamdas``: the labels
    of a file are a chain -- the per-pixel memory goes from label to label -- which ``encode_sae_chain`` runs as one call per 64
    steps; the memory is carried from part to part and starts anew with every file."""
    if select is not None and select not in lamdas:
        raise ValueError(f"select: one of {list(lamdas)}")
    memory = None
    steps = sae_steps(dat_io.sae_label_slices(f_event, label_times), mode)
    for part in sae_parts(steps):
        _, u8, memory = er.encode_sae_chain(dat, part, enc, lamdas, memory, want_f32=False, want_u8=True, xmap=xmap, ymap=ymap)
        emitted = 0
        for _, _, label_time, _, emit in part:
            if not emit:
                continue
            vol = u8[emitted].view(len(lamdas), 2, enc[0], enc[1])
            emitted += 1
            yield label_time, (vol.view(2 * len(lamdas), enc[0], enc[1]) if select is None else vol[list(lamdas).index(select)])


def generate_surfaceofactiveevents(raw_dir, label_dir, target_dir, dataset="gen1", device="cuda"):
    lamdas = SAE_LAMDAS
    _, target, enc, xmap, ymap = _geometry(dataset, device)
    os.makedirs(target_dir, exist_ok=True)
    n_files = 0
    for mode, name, event_file, bbox_file in _sequences(raw_dir, label_dir):
        f_event = dat_io.DatFile(event_file)
        dat = f_event.to_device(device=device)
        for label_time, vol in sae_volumes(f_event, dat, read_label_times(bbox_file), mode, enc, xmap, ymap, lamdas):
            for j, lam in enumerate(lamdas):
                _write(vol[2 * j:2 * j + 2], enc, target, os.path.join(target_dir, f"SurfaceOfActiveEvents{lam}", mode, f"{name}_{label_time}.npy"))
                n_files += 1
    return n_files


# ---- generate_taf.py:78-243 ---------------------------------------------------------------------------------------------
def taf_chains(slices, last_time_of, events_window_abin=10000, max_snapshots=er._lib.MAX_SEQUENCES):
    """The labels of one file (the dicts of ``dat_io.taf_label_slices``, in order) grouped into chains, each a list of slices that
    one ``encode_taf_chain`` call encodes: the records ``[first start_count, last end_count)`` from the first ``start_time``, one
    step of ``bins`` windows per label.  ``last_time_of(slice)``: the timestamp of the slice's last record (``end_count - 1``),
    ``None`` for a slice without records.  Host arithmetic only.

    A label joins the running chain only if ALL of these hold; anything else starts a new chain, and a chain of one label is the
    per-label call:

    * it is not ``fresh`` (its FIFO state continues the previous label's);
    * ``bins > 0`` -- a label that rounds onto the previous one is the double-transform branch of ``encode_taf_label``: it needs
      the state at that point and stays alone, as does a chain's first label;
    * its ``start_time`` lies on the chain's window grid right behind the windows so far (a label whose predecessor was clipped
      to ``total_time()`` is off the grid);
    * the previous label's last record is strictly earlier than that label's ``end_time``: ``DatFile.seek_time`` can land inside
      a run of equal timestamps, whose earlier part the per-label call clamps into the label's last window -- the chain would
      move it to the next window;
    * the chain holds fewer than ``max_snapshots`` labels."""
    chains, cur, windows = [], [], 0
    for sl in slices:
        join = bool(cur) and not sl["fresh"] and sl["bins"] > 0 and cur[-1]["bins"] > 0 and len(cur) < max_snapshots
        if join:
            join = sl["start_time"] == cur[0]["start_time"] + windows * events_window_abin and sl["start_count"] == cur[-1]["end_count"]
        if join:
            last = last_time_of(cur[-1])
            join = last is None or last < cur[-1]["end_time"]
        if not join:
            if cur:
                chains.append(cur)
            cur, windows = [], 0
        cur.append(sl)
        windows += max(sl["bins"], 0)
    if cur:
        chains.append(cur)
    return chains


TAF_WINDOW_US, TAF_BINS, TAF_MIN_EVENT_COUNT = 10000, 8, 50000000   # generate_taf.py's events_window_abin, K, min_event_count


def taf_chain_volumes(f_event, dat, label_times, enc, xmap, ymap):
    """The TAF volumes of one file, one encoder call at a time: yields ``(chain, uint8 (len(chain), K, 2, h, w))`` at the encode
    shape on the GPU, ``chain`` the ``dat_io.taf_label_slices`` dicts of the call's labels in label order.  A run of labels on
    one window grid is one ``encode_taf_chain`` call -- one partition, one tile launch, one synchronisation -- instead of one
    ``encode_taf_label`` call each; a label alone in its chain takes the per-label call."""
    events_window_abin, K = TAF_WINDOW_US, TAF_BINS
    state, stale = None, 0
    slices = list(dat_io.taf_label_slices(f_event, label_times, events_window_abin, K, TAF_MIN_EVENT_COUNT))
    chains = taf_chains(slices, lambda sl: int(f_event._t[sl["end_count"] - 1]) if sl["end_count"] > sl["start_count"] else None,
                        events_window_abin)
    for chain in chains:
        sl = chain[0]
        if sl["fresh"]:
            state = torch.full((enc[0], enc[1], 2, K), -6000.0, device=dat.device)   # :205-209
        # a label that rounds onto the previous one has no window (:181): the reference's `volume` is then STALE -- the
        # previous label's already transformed volume goes through leaky_transform again (:226-227); `stale` counts how
        # many such labels precede this one in a row
        stale = stale + 1 if sl["bins"] <= 0 else 0
        if len(chain) == 1:
            vols = er.encode_taf_label(dat[sl["start_count"]:sl["end_count"]], enc, state, sl["start_time"], events_window_abin,
                                       sl["bins"], K, flip_k=True, xmap=xmap, ymap=ymap, stale_transforms=max(stale - 1, 0))[None]
        else:
            vols = er.encode_taf_chain(dat[sl["start_count"]:chain[-1]["end_count"]], enc, state, sl["start_time"],
                                       events_window_abin, [c["bins"] for c in chain], K, flip_k=True, xmap=xmap, ymap=ymap)
        yield chain, vols


def taf_volumes(f_event, dat, label_times, enc, xmap, ymap):
    """``taf_chain_volumes`` label by label: yields ``(label_time, uint8 (K, 2, h, w))``, newest slot first -- planes ``[:K]`` are
    the ``bins{K/2}`` file, ``[K:]`` the ``bins{K}`` file.  No selection: the FIFO is one state."""
    for chain, vols in taf_chain_volumes(f_event, dat, label_times, enc, xmap, ymap):
        for c, vol in zip(chain, vols):
            yield c["label_time"], vol


def generate_taf(raw_dir, label_dir, target_dir, dataset="gen4", device="cuda"):
    K = TAF_BINS
    _, target, enc, xmap, ymap = _geometry(dataset, device)
    target_dir = os.path.join(target_dir, "taf")
    os.makedirs(target_dir, exist_ok=True)
    n_files = 0
    for mode, name, event_file, bbox_file in _sequences(raw_dir, label_dir):
        os.makedirs(os.path.join(target_dir, mode), exist_ok=True)
        f_event = dat_io.DatFile(event_file)
        dat = f_event.to_device(device=device)
        for chain, vols in taf_chain_volumes(f_event, dat, read_label_times(bbox_file), enc, xmap, ymap):
            if tuple(enc) != tuple(target):   # one resize and one copy to the host per call
                vols = er.resize_nearest(vols.reshape(len(chain) * 2 * K, enc[0], enc[1]), target).reshape(len(chain), K, 2, target[0], target[1])
            vols = vols.cpu().numpy()
            for host, c in zip(vols, chain):
                for part, sub in ((host[:K // 2], f"bins{K // 2}"), (host[K // 2:], f"bins{K}")):   # :229-235
                    path = os.path.join(target_dir, mode, sub, f"{name}_{c['label_time']}.npy")
                    os.makedirs(os.path.dirname(path), exist_ok=True)
                    part.tofile(path)
                    n_files += 1
    return n_files


HARNESSES = {
    "eventcountimage": (generate_eventcountimage, "gen4"),   # the scripts' own -dataset defaults
    "eventvolume": (generate_eventvolume, "gen1"),
    "surfaceofactiveevents": (generate_surfaceofactiveevents, "gen1"),
    "taf": (generate_taf, "gen4"),
}


def main(which, argv=None):
    fn, default_dataset = HARNESSES[which]
    args = _parser(default_dataset).parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("the encoders run on the GPU: no ROCm device is visible (there is no CPU fallback)")
    n = fn(args.raw_dir, args.label_dir, args.target_dir, args.dataset)
    print(f"{which}: {n} files written under {args.target_dir}")


if __name__ == "__main__":
    import sys
    main(sys.argv[1], sys.argv[2:])
