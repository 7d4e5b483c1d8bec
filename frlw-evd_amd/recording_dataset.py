"""Evaluation straight from recordings: ``RecordingLoader`` yields the batches ``dataset.Loader`` yields over the files of a
``generate_*.py`` command -- same samples, same order, same bytes -- without the files.  Every label volume is encoded on the
GPU by the command's own generator (``generate.taf_volumes`` / ``ev_volumes`` / ``eci_volumes`` / ``sae_volumes``: the same
slicing, the same grouping into encoder calls) and stays there; a detector batch is put together from the encoder outputs it
lies in -- it may cross chain, call and file boundaries -- by one launch (``transforms.hand_off``: channel selection, nearest
resize, ``/255``).

Test split only: a volume depends on the FIFO / memory state the labels in front of it left, so the samples come in file
order; training needs random access.
"""
from __future__ import annotations

import os
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import dat_io, generate, transforms
from .dataset import GEN1_CLASSES, GEN4_CLASSES, read_boxes

_PREFIX = {"EventVolume": "ev", "EventCountImage": "eci", "SurfaceOfActiveEvents": "sae"}
_EV_BINS = 5  # generate_eventvolume.py's volume bins


def parse_representation(name, dataset, event_volume_bins=None):
    """``name``: the directory an offline command writes for ``dataset`` (the README's DATA_DIR) -> ``(kind, parameter)``:
    ``("taf", None)``, ``("ev", time window us)``, ``("eci", events N)``, ``("sae", lambda)``.  Anything the command would not
    write is a ``ValueError``; so is, when given, an ``event_volume_bins`` whose ``2 * bins`` channels the kind cannot fill."""
    kind = parameter = None
    if name == "taf":
        kind = "taf"
    else:
        for prefix, k in _PREFIX.items():
            text = name[len(prefix):] if isinstance(name, str) and name.startswith(prefix) else ""
            if not text:
                continue
            if k == "sae":
                try:
                    value = float(text)
                except ValueError:
                    break
                choices = generate.SAE_LAMDAS
            else:
                if not text.isdigit() or str(int(text)) != text:
                    break
                value = int(text)
                choices = generate.EV_TIME_WINDOWS if k == "ev" else generate.eci_events_windows(dataset)
            if value not in choices:
                raise ValueError(f"{name}: the {prefix} command writes {', '.join(f'{prefix}{c}' for c in choices)} for {dataset}")
            kind, parameter = k, choices[choices.index(value)]
            break
    if kind is None:
        raise ValueError(f"{name!r} is no representation directory: taf, EventVolume<tw>, EventCountImage<N> or SurfaceOfActiveEvents<lambda>")
    if event_volume_bins is not None:
        representation_channels(kind, event_volume_bins)
    return kind, parameter


def representation_channels(kind, event_volume_bins):
    """The channels ``2 * event_volume_bins`` a detector takes from a volume of ``kind`` -- the leading planes of TAF (K = 8: all
    16, ``bins4 ++ bins8``; K = 4: the 8 of ``bins4``), all 10 of an Event Volume, the 2 of an Event Count Image or of one
    lambda of the Surface of Active Events.  A count the kind cannot fill is a ``ValueError`` naming the one that fits."""
    fits = {"taf": (generate.TAF_BINS, generate.TAF_BINS // 2), "ev": (_EV_BINS,), "eci": (1,), "sae": (1,)}[kind]
    if event_volume_bins not in fits:
        raise ValueError(f"{kind}: --event_volume_bins {event_volume_bins} does not fit, use "
                         + " or ".join(f"--event_volume_bins {b}" for b in fits))
    return 2 * int(event_volume_bins)


class RecordingLoader:
    """``RecordingLoader(bbox_dir, raw_dir, representation, ...)``: iterating yields ``[imgs (B, C, H, W, 1, 1) float32 on the
    GPU, labels (B, 80, 8) float64 on the GPU, names, stamps]`` like ``Loader(propheseeDataset | propheseeTafDataset)`` over
    ``<data_path>/<representation>``; ``len()`` = batches (the last one may be short).  ``samples``: the planned
    ``(sequence, label_time)`` list, host arithmetic on the recordings' time columns at construction (no GPU)."""

    def __init__(self, bbox_dir, raw_dir, representation, dataset="gen1", input_img_size=[256, 320], img_size=[256, 320],
                 event_volume_bins=5, mode="test", batch_size=1, device="cuda", clipping=False):
        self.kind, self.parameter = parse_representation(representation, dataset)
        self.channels = representation_channels(self.kind, event_volume_bins)
        self.mode, self.dataset, self.clipping = mode, dataset, clipping
        self.input_img_size, self.img_size = input_img_size, img_size
        self.sensor, target = generate.SHAPES["gen4" if dataset == "gen4" else "gen1"]
        if tuple(img_size) != tuple(target):
            raise ValueError(f"img_size {tuple(img_size)}: the {dataset} commands write {target}")
        self.batch_size = int(batch_size)
        if not 1 <= self.batch_size <= transforms.MAX_HAND_OFF:
            raise ValueError(f"batch_size: 1..{transforms.MAX_HAND_OFF} per process")
        self.device = torch.device(device)
        if dataset == "gen1":   # data/dataset.py:52-63, as propheseeDataset
            self.width, self.height, self.object_classes = 304, 240, list(GEN1_CLASSES)
        else:
            self.width, self.height, self.object_classes = 1280, 720, list(GEN4_CLASSES)
        self.root = os.path.join(bbox_dir, mode)
        self.raw_root = os.path.join(raw_dir, mode)
        self.files = [f[:-9] for f in os.listdir(self.root) if f[-3:] == "npy"]  # "<seq>_bbox.npy" -> "<seq>", propheseeDataset's list
        self._boxes, self._stamp = {}, {}
        self.sequences = []   # (name, planned label times): the labels the command writes a file for
        for name in self.files:
            path = self._event_file(name)
            if not os.path.exists(path):   # no recording, no files: createAllBBoxDataset lists nothing either
                continue
            boxes = self._boxes[name] = read_boxes(os.path.join(self.root, name + "_bbox.npy"))
            times = np.unique(boxes["t"])
            self._stamp[name] = {int(t): t for t in times}
            planned = [sl["label_time"] for sl in self._slices(dat_io.DatFile(path), times)]
            if planned:
                self.sequences.append((name, planned))
        self.samples = [(name, t) for name, planned in self.sequences for t in planned]

    def _event_file(self, name):
        return os.path.join(self.raw_root, name + "_td.dat")

    def _slices(self, f_event, times):
        if self.kind == "taf":
            return dat_io.taf_label_slices(f_event, times, generate.TAF_WINDOW_US, generate.TAF_BINS, generate.TAF_MIN_EVENT_COUNT)
        if self.kind == "ev":
            return dat_io.ev_label_slices(f_event, times, generate.EV_TIME_WINDOWS)
        if self.kind == "eci":
            return dat_io.eci_label_slices(f_event, times, generate.eci_events_windows(self.dataset))
        return dat_io.sae_label_slices(f_event, times)

    def __len__(self):
        return (len(self.samples) + self.batch_size - 1) // self.batch_size

    # ---- iteration ------------------------------------------------------------------------------------------------------
    def _load(self, name):
        """(reader thread) the records of one sequence in pinned memory, and its ``DatFile`` for the slicer."""
        f_event = dat_io.DatFile(self._event_file(name))
        host = torch.empty((len(f_event.records), 8), dtype=torch.uint8, pin_memory=self.device.type == "cuda")
        host.numpy()[...] = np.asarray(f_event.records).view(np.uint8).reshape(-1, 8)
        return f_event, host

    def _volumes(self, name, f_event, dat, enc, xmap, ymap):
        """(label_time, uint8 tensor whose first ``channels`` planes are the sample) of one sequence, in label order."""
        times = np.unique(self._boxes[name]["t"])
        if self.kind == "taf":
            return generate.taf_volumes(f_event, dat, times, enc, xmap, ymap)
        if self.kind == "ev":
            return generate.ev_volumes(f_event, dat, times, enc, xmap, ymap, self.parameter, generate.EV_TIME_WINDOWS, _EV_BINS)
        if self.kind == "eci":
            return generate.eci_volumes(f_event, dat, times, enc, xmap, ymap, generate.eci_events_windows(self.dataset), self.parameter)
        return generate.sae_volumes(f_event, dat, times, self.mode, enc, xmap, ymap, generate.SAE_LAMDAS, self.parameter)

    def _batch(self, sources, meta, enc):
        imgs = transforms.hand_off(sources, self.channels, enc, self.img_size)
        labels = []
        for name, t in meta:
            boxes = self._boxes[name]
            labels.append(transforms.sample_labels(boxes[boxes["t"] == t], random, self.input_img_size, (self.height, self.width),
                                                   self.dataset, self.mode, False, self.clipping)[0])
        return [imgs, torch.from_numpy(np.stack(labels)).to(self.device, non_blocking=True), [name for name, _ in meta],
                np.array([t for _, t in meta])]

    def __iter__(self):
        if not self.sequences:
            return
        _, _, enc, xmap, ymap = generate._geometry(self.dataset, self.device)
        sources, meta = [], []   # the running batch: views into encoder outputs (they keep them alive), (name, stamp)
        with ThreadPoolExecutor(1) as reader:
            nxt = reader.submit(self._load, self.sequences[0][0])
            for i, (name, planned) in enumerate(self.sequences):
                f_event, host = nxt.result()
                if i + 1 < len(self.sequences):
                    nxt = reader.submit(self._load, self.sequences[i + 1][0])   # read while this sequence is encoded
                dat = host.to(self.device, non_blocking=True)
                got = 0
                for label_time, vol in self._volumes(name, f_event, dat, enc, xmap, ymap):
                    if label_time != planned[got]:
                        raise RuntimeError(f"{name}: label {label_time} encoded where {planned[got]} was planned")
                    got += 1
                    sources.append(vol)
                    meta.append((name, self._stamp[name][label_time]))
                    if len(sources) == self.batch_size:
                        yield self._batch(sources, meta, enc)
                        sources, meta = [], []
                if got != len(planned):
                    raise RuntimeError(f"{name}: {got} labels encoded, {len(planned)} planned")
                del dat, host, f_event   # one sequence's records at a time; the pending volumes stay (the batch holds them)
        if sources:
            yield self._batch(sources, meta, enc)
