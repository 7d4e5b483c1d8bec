"""Child process of tests/test_recording_eval_gpu.py: for every entry-point case, ``exp.<recipe>(Setting_test(args)).test()`` once over
the files of the offline command (``--data_path``, with ``--record True``: its summarise.npz is kept as summarise_files.npz) and once
straight from the recordings (``--raw_dir --representation``), in one process group like ``test.py`` sets it up.  The evaluator's
paired lists of both routes go to ``<out>.npz``.

usage: recording_eval_child.py RAW_DIR LABEL_DIR PROCESSED_DIR LOG_ROOT OUT_NPZ
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(raw, lab, processed, log_root, out):
    import recording_eval_data as red
    import test as test_entry
    import train as train_entry
    from frlw_evd_amd.settings import Setting_test
    saved = {}
    for key, case in red.ENTRY_CASES.items():
        log = os.path.join(log_root, key) + "/"
        common = ["--batch_size", "4", "--resume_exp", "R", "--dataset", "gen1", "--exp_type", case["exp_type"], "--event_volume_bins",
                  str(case["bins"]), "--nodes", "1", "--log_path", log, "--bbox_path", lab, "--num_cpu_workers", "2"]
        routes = {"files": ["--data_path", os.path.join(processed, case["representation"]), "--record", "True"],
                  "recordings": ["--raw_dir", raw, "--representation", case["representation"]]}
        for route, extra in routes.items():
            args = test_entry.parse_args(common + extra)
            cls = train_entry.pick_experiment(args.exp_type)
            train_entry.init_distributed(args)
            result = cls(Setting_test(args)).test()
            for name in ("gt_boxes_list", "dt_boxes_list"):
                saved[f"{key}/{route}/{name}/n"] = np.array(len(result[name]))
                for i, rows in enumerate(result[name]):
                    saved[f"{key}/{route}/{name}/{i}"] = np.asarray(rows)
            if route == "files":
                os.replace(os.path.join(log, "R", "summarise.npz"), os.path.join(log, "R", "summarise_files.npz"))
    np.savez(out, **saved)
    import torch
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main(*sys.argv[1:6])
