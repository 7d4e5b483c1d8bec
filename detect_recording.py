#!/usr/bin/env python3
"""Detect on a raw recording: ``--dat <file>_td.dat`` or ``--raw <file>.raw`` -> ``<out>.npy``, a structured box array with the fields of a
``*_bbox.npy`` annotation file (``dataset.read_boxes`` reads it back), one set of boxes every ``--period`` microseconds.

The model is built the way ``test.py`` builds it (``--exp_type``, ``--dataset``, ``--event_volume_bins``; ``--resume_exp E`` loads
``<log_path>E/checkpoints/best_epoch.pth``, ``--checkpoint`` any checkpoint file of this build or of the reference).  The events
are encoded on the GPU as the TAF recipes expect them (``generate_taf.py``: K = 8, 10 ms windows) -- every frame of a detector
batch in one encode call (``frlw_evd_amd.stream.StreamDetector``); no annotation file and no representation file is needed.
``--frames DIR [--frames_every N]`` also writes every N-th frame as a PNG, the TAF image with that frame's detections, painted on
the GPU from the volumes the detector just read (``frlw_evd_amd.visualize``).
``--raw`` takes a Prophesee recording as the camera wrote it, in the EVT 2.0, EVT 2.1 or EVT 3.0 encoding (the file's header names
it): the words are decoded to event records on the GPU (``frlw_evd_amd.raw_io``), the sensor shape comes from the file's header
(``--dataset`` names it when the header does not), and the printed summary carries the decode counters."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def recording_source(args):
    """``("dat" | "raw", path)``: exactly one of ``--dat`` / ``--raw`` names the recording."""
    if (args.dat is None) == (args.raw is None):
        raise SystemExit("exactly one of --dat FILE_td.dat / --raw FILE.raw names the recording")
    return ("dat", args.dat) if args.raw is None else ("raw", args.raw)


class _Parser(argparse.ArgumentParser):
    """The check that one recording is named runs behind the parse (neither flag is ``required``)."""

    def parse_args(self, args=None, namespace=None):
        parsed = super().parse_args(args, namespace)
        recording_source(parsed)
        return parsed


def build_parser():
    parser = _Parser(description="Detect on a raw .dat or Prophesee .raw (EVT 2.0, EVT 2.1, EVT 3.0) recording.")
    parser.add_argument("--dat")                         # <sequence>_td.dat
    parser.add_argument("--raw")                         # <sequence>.raw (Prophesee EVT 2.0 / 2.1 / 3.0), instead of --dat
    parser.add_argument("--out", required=True)          # written as <out>.npy
    parser.add_argument("--local_rank", "--local-rank", type=int, default=None)
    parser.add_argument("--resume_exp")
    parser.add_argument("--checkpoint")                  # a checkpoint file, instead of --resume_exp
    parser.add_argument("--exp_type", default="yolox_taf_bfm")
    parser.add_argument("--log_path", default="log/")
    parser.add_argument("--dataset", default="gen1")
    parser.add_argument("--event_volume_bins", type=int, default=8)
    parser.add_argument("--period", type=int, default=50000)          # microseconds between frames
    parser.add_argument("--frames_per_call", type=int, default=32)
    parser.add_argument("--t_begin", type=int, default=0)
    parser.add_argument("--t_end", type=int, default=None)            # default: the last event
    parser.add_argument("--seq_nms", choices=("off", "stop", "skip"), default="off")   # Seq-NMS over the whole recording
    parser.add_argument("--seq_nms_metric", choices=("avg", "max"), default="avg")
    parser.add_argument("--seq_nms_drop", action="store_true")        # remove the boxes a sequence suppresses
    parser.add_argument("--frames")                                   # a directory: one PNG per frame, <stem>_<t>.png
    parser.add_argument("--frames_every", type=int, default=1)        # ... per every N-th frame
    parser.set_defaults(record=None, bbox_path=None, data_path=None, batch_size=1, num_cpu_workers=1, nodes=1, metric="none")
    return parser


def seq_nms_options(args):
    """``StreamDetector``'s ``seq_nms`` argument for the flags: None when off; ``stop`` ends where the reference ends (a single box
    outranks every remaining sequence), ``skip`` goes on until no sequence of two boxes is left."""
    if args.seq_nms == "off":
        return None
    return {"isolated": args.seq_nms, "metric": args.seq_nms_metric, "drop_suppressed": bool(args.seq_nms_drop)}


def frame_stem(dat_path):
    """``<dir>/<sequence>_td.dat`` -> ``<sequence>``: what the frames' file names start with."""
    stem = os.path.basename(dat_path)
    stem = stem[:-4] if stem.endswith((".dat", ".raw")) else stem
    return stem[:-3] if stem.endswith("_td") else stem


class FrameWriter:
    """``StreamDetector``'s ``on_volumes`` callback behind ``--frames``: every ``every``-th frame as ``<dir>/<stem>_<t>.png``, the
    TAF image of all 2K channels (README 7) at the sensor shape with that frame's detections.  Without Seq-NMS the boxes are
    final when the batch arrives: one fused render launch per detector batch.  With it they are final only after the whole
    recording: the batches' backgrounds are rendered without boxes and kept on the host, and ``finish`` overlays the rescored boxes
    that no sequence suppressed (``BGR`` mode) before it writes the files.  The box file may keep the suppressed boxes (no
    ``--seq_nms_drop``), so ``finish`` runs Seq-NMS once more on the boxes it collected, with the drop switched on."""

    def __init__(self, directory, stem, sensor, labelmap, every=1, seq_nms=None):
        if every < 1:
            raise SystemExit("--frames_every: at least 1")
        self.directory, self.stem, self.sensor, self.labelmap, self.every = directory, stem, sensor, labelmap, int(every)
        self.seq_nms = None if seq_nms is None else dict(seq_nms, drop_suppressed=True)
        self.seen = 0
        self.written = 0
        self.backgrounds, self.stamps, self.rows = [], [], []
        os.makedirs(directory, exist_ok=True)

    def path(self, t):
        return os.path.join(self.directory, "{0}_{1}.png".format(self.stem, int(t)))

    def _write(self, images, stamps):
        from frlw_evd_amd import visualize
        for img, t in zip(images.cpu().numpy(), stamps):
            visualize.write_png(self.path(t), img)
            self.written += 1

    def __call__(self, u8, enc, stamps, boxes):
        import torch
        from frlw_evd_amd import visualize
        pick = [j for j in range(len(stamps)) if (self.seen + j) % self.every == 0]
        self.seen += len(stamps)
        self.rows += boxes                          # every frame's boxes: Seq-NMS links across the frames not drawn
        if not pick:
            return
        vol = u8.reshape(u8.shape[0], -1, enc[0], enc[1])
        if len(pick) != len(stamps):
            vol = vol[torch.tensor(pick, device=vol.device)]
        if self.seq_nms is None:
            self._write(visualize.render(vol, "TAF", self.sensor, dt=[boxes[j] for j in pick], labelmap=self.labelmap),
                        [stamps[j] for j in pick])
        else:
            self.backgrounds.append(visualize.render(vol, "TAF", self.sensor).cpu())
            self.stamps += [(self.seen - len(stamps) + j, stamps[j]) for j in pick]

    def finish(self):
        """The Seq-NMS route's second half; nothing to do otherwise."""
        if self.seq_nms is None or not self.stamps:
            return
        import torch
        from frlw_evd_amd import visualize
        from frlw_evd_amd.seq_nms import rescore_frames
        rows, _ = rescore_frames(self.rows, **self.seq_nms)
        backgrounds = torch.cat(self.backgrounds)
        for lo in range(0, len(self.stamps), 64):
            part = self.stamps[lo:lo + 64]
            images = visualize.render(backgrounds[lo:lo + 64].cuda(), "BGR", self.sensor, dt=[rows[j] for j, _ in part],
                                      labelmap=self.labelmap)
            self._write(images, [t for _, t in part])


def build_model(args):
    """The experiment's network as ``test.py`` builds it (``Setting_test`` -> ``_build_all`` -> checkpoint), in eval mode."""
    import train as train_entry
    cls = train_entry.pick_experiment(args.exp_type)
    train_entry.init_distributed(args)
    from frlw_evd_amd.settings import Setting_test
    settings = Setting_test(args)
    if args.checkpoint is not None:
        settings.resume_ckpt_file = args.checkpoint
    exp = cls(settings)
    exp.object_classes = exp._classes()
    exp._build_all()
    if settings.resume_ckpt_file is not None:
        exp.loadCheckpointTest(settings.resume_ckpt_file)
    return exp.model.module.eval(), settings


def main(argv=None):
    import numpy as np
    import torch
    args = build_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("the encoders and the detector run on the GPU: no ROCm device is visible (there is no CPU fallback)")
    from frlw_evd_amd import dat_io
    from frlw_evd_amd.generate import SHAPES
    from frlw_evd_amd.stream import StreamDetector
    net, settings = build_model(args)
    sensor, _ = SHAPES["gen4" if args.dataset == "gen4" else "gen1"]
    kind, rec_path = recording_source(args)
    decode_counters = None
    if kind == "raw":
        from frlw_evd_amd import raw_io
        f_event = raw_io.RawFile(rec_path)
        sensor = f_event.size or sensor
        records, decode_counters = f_event.decode(device=settings.gpu_device, time_shift=True, size=sensor)
        if decode_counters["unsorted"] > 0:
            raise SystemExit("{0}: {1} events are earlier than their predecessor; the detector needs time-sorted records "
                             "(sorting is not done here)".format(rec_path, decode_counters["unsorted"]))
    else:
        f_event = dat_io.DatFile(rec_path)
    writer = None
    if args.frames is not None:
        from frlw_evd_amd.visualize import LABELMAPS
        writer = FrameWriter(args.frames, frame_stem(rec_path), sensor, LABELMAPS["gen4" if args.dataset == "gen4" else "gen1"],
                             args.frames_every, seq_nms_options(args))
    det = StreamDetector(net, sensor, settings.img_size, dataset=args.dataset, volume_bins=8, input_bins=args.event_volume_bins,
                         period_us=args.period, frames_per_call=args.frames_per_call, seq_nms=seq_nms_options(args),
                         on_volumes=writer)
    t_end = f_event.total_time() if args.t_end is None else args.t_end
    if kind == "dat":
        records = f_event.to_device(device=settings.gpu_device)
    boxes = det.run(records, args.t_begin, t_end)
    if writer is not None:
        writer.finish()
    path = args.out if args.out.endswith(".npy") else args.out + ".npy"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.save(path, boxes)
    summary = {"frames": len(det.frame_times(args.t_begin, t_end)), "boxes": int(len(boxes)), "sequences": int(det.sequences),
               "out": path}
    if writer is not None:
        summary["frames_written"] = writer.written
    if decode_counters is not None:
        summary["decode"] = decode_counters
    print(summary)
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()
    return boxes


if __name__ == "__main__":
    main()
