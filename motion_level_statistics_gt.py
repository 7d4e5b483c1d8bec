#!/usr/bin/env python3
"""`python motion_level_statistics_gt.py -raw_dir R -dataset gen1|gen4` -- the reference's command (motion_level_statistics_gt.py:45-140, README 4.2): same flags, same directory and file names.
Every isolated ground-truth box of R/test with the flow density inside it -> statistics_result/gt_<dataset>.npz (frlw_evd_amd/motion.py; pinned by tests/golden/motion.npz, written by the reference's own scripts)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from frlw_evd_amd import motion  # noqa: E402

if __name__ == "__main__":
    motion.main("motion_level_statistics_gt")
