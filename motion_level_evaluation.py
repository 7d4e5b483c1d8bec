#!/usr/bin/env python3
"""`python motion_level_evaluation.py [-dataset gen1|gen4] -exp_name E` -- the reference's command (motion_level_evaluation.py:13-80, README 5.2): same flags, same directory and file names.
MAP per flow-density bucket from log/E/summarise_stats.npz and statistics_result/gt_<dataset>.npz, scored on the GPU (frlw_evd_amd/motion.py; pinned by tests/golden/motion.npz, written by the reference's own scripts)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from frlw_evd_amd import motion  # noqa: E402

if __name__ == "__main__":
    motion.main("motion_level_evaluation")
