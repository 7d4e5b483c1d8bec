#!/usr/bin/env python3
"""`python visualization.py -item I -end T -volume_bins K -ecd D -bbox_path B -data_path P [-result_path summarise.npz]
-dataset gen1|gen4 -datatype TAF|SurfaceOfActiveEvent|EventCountImage|EventVolume|OpticalFlow -suffix S` -- the reference's
command (visualization.py:315-387, README 7): same flags, same input files, same output names under visualization/.
The image is painted on the GPU (frlw_evd_amd/visualize.py, csrc/render.hip; definitions and deviations: DESIGN.md 3.16) and
written as PNG by the standard library; neither cv2 nor seaborn is needed."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

TOL = 4999
TARGET_PATH = "visualization"
DATA_FOLDER = "test"
SHAPES = {"gen1": ((240, 304), (256, 320)), "gen4": ((720, 1280), (512, 640))}   # (sensor, stored), :347-354
DATATYPES = ("TAF", "SurfaceOfActiveEvent", "EventCountImage", "EventVolume", "OpticalFlow")


def build_parser():
    parser = argparse.ArgumentParser(description="visualize one or several event files along with their boxes")
    parser.add_argument("-item", type=str)              # name of the event file
    parser.add_argument("-end", type=int)               # annotation timestamp
    parser.add_argument("-volume_bins", type=float)     # channels of the representation / 2
    parser.add_argument("-ecd", type=str)               # data_path + ecd = the train / val / test level of the preprocessed data
    parser.add_argument("-bbox_path", type=str)         # the train / val / test level of the dataset (annotations)
    parser.add_argument("-data_path", type=str)
    parser.add_argument("-result_path", type=str, default=None)   # summarise.npz; without it no detections are drawn
    parser.add_argument("-dataset", type=str, default="gen1")
    parser.add_argument("-datatype", type=str)
    parser.add_argument("-suffix", type=str)
    return parser


def dataset_key(dataset):
    return "gen1" if dataset == "gen1" else "gen4"


def output_name(item, end, suffix, datatype, with_result):
    """The file name the reference writes under visualization/ (:214-216, :239-241, :261-263, :291-293, :309-311)."""
    tail = "_result.png" if with_result else ".png"
    if datatype == "OpticalFlow":
        return item + "_{0}".format(int(end)) + "_OpticalFlow" + tail
    return item + "_{0}_".format(int(end)) + suffix + "_" + datatype + tail


def volume_files(args):
    """[(path, channels)] of the raw uint8 files the reference reads for the item (:13-32, :377-381)."""
    name = args.item + "_" + str(args.end) + ".npy"
    bins = args.volume_bins
    if args.datatype == "TAF":
        root = os.path.join(args.data_path, DATA_FOLDER)
        if bins == 4:
            return [(os.path.join(root, "bins{0}".format(int(bins)), name), int(bins * 2))]
        return [(os.path.join(root, "bins{0}".format(int(bins / 2)), name), int(bins)),
                (os.path.join(root, "bins{0}".format(int(bins)), name), int(bins))]
    return [(os.path.join(args.data_path, args.ecd, DATA_FOLDER, name), int(bins * 2))]


def load_volume(args, stored):
    import numpy as np
    return np.concatenate([np.fromfile(path, dtype=np.uint8).reshape(channels, stored[0], stored[1])
                           for path, channels in volume_files(args)], 0)


def main(argv=None):
    import numpy as np
    import torch
    args = build_parser().parse_args(argv)
    if args.datatype not in DATATYPES:
        raise SystemExit("-datatype: one of " + "/".join(DATATYPES))
    if not torch.cuda.is_available():
        raise SystemExit("the renderer runs on the GPU: no ROCm device is visible (there is no CPU fallback)")
    from frlw_evd_amd import visualize
    from frlw_evd_amd.dataset import read_boxes
    sensor, stored = SHAPES[dataset_key(args.dataset)]
    labelmap = visualize.LABELMAPS[dataset_key(args.dataset)]
    dt = None
    if args.result_path is not None:
        f_bbox = np.load(args.result_path)
        dt = f_bbox["dts"][f_bbox["file_names"] == args.item]
    gt = read_boxes(os.path.join(args.bbox_path, DATA_FOLDER, args.item + "_bbox.npy"))
    gt, dt = visualize.select_boxes(gt, dt, args.end, TOL)
    if args.datatype == "OpticalFlow":
        flow = np.load(os.path.join("optical_flow_buffer", args.item + "_{0}.npy".format(args.end)))
        source, mode = torch.from_numpy(visualize.flow_image(flow)[None]).cuda(), "BGR"
        sensor = tuple(source.shape[1:3])
    else:
        source, mode = torch.from_numpy(load_volume(args, stored)[None]).cuda(), args.datatype
    img = visualize.render(source, mode, sensor, gt=[gt], dt=None if dt is None else [dt], labelmap=labelmap)[0]
    os.makedirs(TARGET_PATH, exist_ok=True)
    path = os.path.join(TARGET_PATH, output_name(args.item, args.end, args.suffix, args.datatype, dt is not None))
    visualize.write_png(path, img)
    print(path)
    return path


if __name__ == "__main__":
    main()
