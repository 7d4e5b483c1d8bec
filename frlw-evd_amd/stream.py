"""Detection on a raw recording: boxes at a fixed cadence straight from the ``.dat`` records of one file.

The offline route to the same boxes is ``generate_taf.py`` -> uint8 files -> ``propheseeTafDataset`` -> ``test.py``; it needs
annotation files just to know where to encode, and its FIFO state forces one encode call per frame.  ``StreamDetector`` keeps the
records on the GPU and runs, per group of ``frames_per_call`` frames, ONE ``encode_taf_chain`` (one partition, one tile launch:
the volume after every ``period_us`` of the same pass over the events), the hand-off the dataset classes perform on the files
(channel selection, nearest resize or coordinate maps, ``/255``), one detector forward on the whole group and the evaluator's
rescale to sensor pixels with the Prophesee minimum-size filter.
"""
from __future__ import annotations

import numpy as np
import torch

from . import event_representation as er
from . import transforms
from .evaluator import evaluator

# the fields of a ``*_bbox.npy`` file (src/io/npy_events_tools.py:57-58 names)
BBOX_DTYPE = np.dtype([("t", "<u8"), ("x", "<f4"), ("y", "<f4"), ("w", "<f4"), ("h", "<f4"), ("class_id", "u1"),
                       ("class_confidence", "<f4"), ("track_id", "<u4")])


class StreamDetector:
    """``model``: a ``yolox.model.model`` in eval mode on the GPU with ``2 * input_bins`` input channels.  ``sensor_shape`` /
    ``img_size``: (H, W) of the recording and of the detector input.  ``volume_bins``: the TAF FIFO depth K the encoder runs
    (``generate_taf.py``: 8); ``input_bins``: what the dataset class would read for ``--event_volume_bins`` -- K (the ``bins{K/2}``
    file followed by the ``bins{K}`` file: all 2K channels, newest slot first) or K / 2 (the ``bins{K/2}`` file alone: the newest
    K / 2 slots).  A frame every ``period_us``, a multiple of the FIFO window ``window_us``; ``frames_per_call`` frames (at most
    64) per encode call and per detector batch.  ``seq_nms``: None, or a dict of ``seq_nms.rescore_frames`` arguments (``isolated``,
    ``metric``, ``drop_suppressed``, thresholds): ``run`` then links the boxes of the whole recording, writes the rescored
    confidences and the sequence ids (``track_id``) and leaves the number of sequences in ``self.sequences``.  ``on_volumes``: None,
    or a callable ``run`` calls once per detector batch with ``(u8, enc, stamps, boxes)`` -- the batch's uint8 volumes
    (S, K, 2, h, w) at the encode shape ``enc``, still on the GPU, the frames' timestamps and their boxes before any Seq-NMS
    (``visualize.render`` draws from exactly this)."""

    def __init__(self, model, sensor_shape, img_size, dataset="gen1", volume_bins=8, input_bins=8, period_us=50000,
                 window_us=10000, frames_per_call=32, seq_nms=None, on_volumes=None):
        self.model = model
        self.sensor_shape = (int(sensor_shape[0]), int(sensor_shape[1]))
        self.img_size = (int(img_size[0]), int(img_size[1]))
        self.K, self.input_bins = int(volume_bins), int(input_bins)
        self.period_us, self.window_us = int(period_us), int(window_us)
        if self.window_us <= 0 or self.period_us <= 0 or self.period_us % self.window_us:
            raise ValueError("period_us must be a positive multiple of window_us")
        if self.input_bins == self.K:
            self.channels = 2 * self.K
        elif 2 * self.input_bins == self.K:
            self.channels = self.K          # (K / 2 slots) x 2 polarities
        else:
            raise ValueError("input_bins must be volume_bins (bins{K/2} ++ bins{K}) or volume_bins / 2 (bins{K/2})")
        self.frames_per_call = int(frames_per_call)
        if not 1 <= self.frames_per_call <= er._lib.MAX_SEQUENCES:
            raise ValueError(f"frames_per_call: 1..{er._lib.MAX_SEQUENCES}")
        self.dataset = dataset
        self.seq_nms = None if seq_nms is None else dict(seq_nms)
        self.sequences = 0
        self.on_volumes = on_volumes
        self.evaluator = evaluator(None, self.frames_per_call, 10000, self.sensor_shape[1], self.sensor_shape[0], self.img_size[1],
                                   self.img_size[0], dataset)

    def geometry(self, device):
        """(encode shape, xmap, ymap) as ``generate._geometry`` picks them: a target smaller than the sensor moves the events
        (coordinate maps, encode at the target shape), a larger one encodes natively and resizes the volume up."""
        if self.img_size[0] < self.sensor_shape[0]:
            xmap, ymap = er.coordinate_maps(self.sensor_shape, self.img_size, device)
            return self.img_size, xmap, ymap
        return self.sensor_shape, None, None

    def hand_off(self, u8, enc):
        """uint8 volumes (S, K, 2, h, w) at the encode shape -> detector input (S, C, H, W, 1) float32: the channels the dataset
        class reads for ``input_bins``, nearest resize to ``img_size`` when the shapes differ, ``/255``."""
        u8 = u8.contiguous()
        return transforms.hand_off([u8[s] for s in range(u8.shape[0])], self.channels, enc, self.img_size)[..., 0]

    def boxes(self, outputs, stamps):
        """Detections of one batch (``model.detect``'s list) -> list of (n_i, 8) float32 rows [t, x, y, w, h, class, confidence,
        0] in sensor pixels that pass the dataset's minimum-size filter; the all-zero row that stands for "no detection" is
        dropped."""
        rows, keep = self.evaluator.transform_dt_batch(outputs, stamps)
        return [r[k & (r[:, 1:7] != 0).any(axis=1)] for r, k in zip(rows, keep)]

    def frame_times(self, t_begin, t_end):
        """Frame ``j`` (1-based) is the volume at ``t_begin + j * period_us``: every whole period inside ``[t_begin, t_end]``."""
        n = max(0, (int(t_end) - int(t_begin)) // self.period_us)
        return [int(t_begin) + j * self.period_us for j in range(1, n + 1)]

    def run(self, dat, t_begin, t_end):
        """``dat``: the time-sorted raw records of the recording on the GPU (``DatFile.to_device()``).  The FIFO state starts at
        -6000 at ``t_begin``; frame ``j`` holds the events with ``t_begin <= t < t_begin + j * period_us`` (an event on a frame
        boundary belongs to the later frame).  Returns the boxes of all frames as one structured array with the fields of a
        ``*_bbox.npy`` file (``track_id`` 0 unless ``seq_nms`` is set), in frame order."""
        rows = dat.contiguous().view(torch.uint8).reshape(-1, 8)
        device = rows.device
        enc, xmap, ymap = self.geometry(device)
        times = self.frame_times(t_begin, t_end)
        F = self.frames_per_call
        groups = [times[i:i + F] for i in range(0, len(times), F)]
        out = []
        if groups:
            t = rows.view(torch.int32).reshape(-1, 2)[:, 0].to(torch.int64) & 0xFFFFFFFF
            bounds = torch.tensor([int(t_begin)] + [g[-1] for g in groups], dtype=torch.int64, device=device)
            cuts = torch.searchsorted(t, bounds, right=False).tolist()
            state = torch.full((enc[0], enc[1], 2, self.K), -6000.0, device=device)
            bins = self.period_us // self.window_us
            for g, stamps in enumerate(groups):
                u8 = er.encode_taf_chain(rows[cuts[g]:cuts[g + 1]], enc, state, stamps[0] - self.period_us, self.window_us,
                                         [bins] * len(stamps), self.K, flip_k=True, xmap=xmap, ymap=ymap)
                with torch.no_grad():
                    outputs = self.model.detect(self.hand_off(u8, enc))
                found = self.boxes(outputs, stamps)
                if self.on_volumes is not None:
                    self.on_volumes(u8, enc, stamps, found)
                out += found
        if self.seq_nms is not None:
            from .seq_nms import rescore_frames
            out, self.sequences = rescore_frames(out, **self.seq_nms)
        return to_bbox_records(out, times)


def to_bbox_records(frames, stamps):
    """List of (n_i, 8) rows [t, x, y, w, h, class, confidence, track], one entry per frame, and the frames' timestamps -> one
    structured ``*_bbox.npy`` array (``t`` from ``stamps``: the float32 rows hold it only up to 2^24 us)."""
    rows = np.concatenate(frames, axis=0) if frames else np.zeros((0, 8), np.float32)
    rec = np.zeros(len(rows), dtype=BBOX_DTYPE)
    for j, name in enumerate(BBOX_DTYPE.names):
        rec[name] = rows[:, j]
    rec["t"] = np.repeat(np.asarray(stamps, dtype=np.uint64), [len(f) for f in frames]) if frames else 0
    return rec
