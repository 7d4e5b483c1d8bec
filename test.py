#!/usr/bin/env python3
"""Evaluation entry point with the reference's command line (test.py:9-52): same flags, process-group init and
``Setting_test`` -> ``yolox(settings).test()`` dispatch; ``--resume_exp E`` loads ``<log_path>E/checkpoints/best_epoch.pth``
(a checkpoint written by this build or by the reference: same dict layout and parameter names), ``--record True`` writes
``summarise.npz``.  ``--raw_dir DIR --representation NAME`` (instead of ``--data_path``) evaluates straight from the recordings:
the test split's label volumes are encoded on the GPU as the ``generate_*.py`` command of ``NAME`` (the README's DATA_DIR: ``taf``,
``EventVolume250000``, ...) would write them and handed to the detector without files -- same boxes, same score.  Without
``--data_path`` / ``--bbox_path`` / ``--raw_dir`` the run is synthetic (see train.py); the detections go through the gfx950 engine
(decode + NMS on device) and the evaluator hand-off."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def build_parser():
    parser = argparse.ArgumentParser(description="Test network.")
    parser.add_argument("--local_rank", "--local-rank", type=int, default=None,
                        help="local rank for DistributedDataParallel")
    parser.add_argument("--resume_exp")  # experiment whose best_epoch checkpoint is evaluated
    parser.add_argument("--exp_type", default="basic")
    parser.add_argument("--log_path", default="log/")
    parser.add_argument("--record", type=bool)  # summarise.npz under log_path for visualisation / motion-level evaluation
    parser.add_argument("--dataset", default="gen1")
    parser.add_argument("--bbox_path")
    source = parser.add_mutually_exclusive_group()
    source.add_argument("--data_path")
    source.add_argument("--raw_dir")          # "train, val, test" level directory of the recordings (<mode>/<seq>_td.dat)
    parser.add_argument("--representation")   # with --raw_dir: the directory name the offline command would have written
    parser.add_argument("--event_volume_bins", type=int, default=5)
    parser.add_argument("--batch_size", type=int, default=1)
    parser.add_argument("--num_cpu_workers", type=int, default=-1)
    parser.add_argument("--nodes", type=int, default=1)
    parser.add_argument("--metric", choices=("none", "coco"), default="none")  # coco: score the test split with the GPU COCO mAP
    return parser


def parse_args(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.raw_dir is not None:
        if args.representation is None:
            parser.error("--raw_dir needs --representation (taf, EventVolume<tw>, EventCountImage<N>, SurfaceOfActiveEvents<lambda>)")
        if args.bbox_path is None:   # the README keeps recordings and annotations in one tree
            args.bbox_path = args.raw_dir
    elif args.representation is not None:
        parser.error("--representation goes with --raw_dir")
    return args


def main(argv=None):
    import train as train_entry
    args = parse_args(argv)
    cls = train_entry.pick_experiment(args.exp_type)
    train_entry.init_distributed(args)
    from frlw_evd_amd.settings import Setting_test
    settings = Setting_test(args)
    tester = cls(settings)
    stats = []
    if settings.metric == "coco":  # evaluate/evaluator.py:103-113: the COCO summary, then the score
        from frlw_evd_amd import coco_eval

        def metric_fn(gt_boxes_list, dt_boxes_list, **kw):
            stats.append(coco_eval.coco_eval_arrays(gt_boxes_list, dt_boxes_list, **kw)[2])
            return tuple(float(s) for s in stats[-1][:6])
        tester.metric_fn = metric_fn
    result = tester.test()
    import torch
    if torch.distributed.get_rank() == 0 and isinstance(result, dict):
        n_dt = sum(len(d) for d in result["dt_boxes_list"])
        print({"images": len(result["gt_boxes_list"]), "detections": n_dt, "avg_infer_ms": round(result["avg_infer_ms"], 3)})
    if torch.distributed.get_rank() == 0 and stats:
        coco_eval.summarize(stats[-1])
        print("Current score: ", result[0])
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()
    return result


if __name__ == "__main__":
    main()
