#!/usr/bin/env python3
"""`python generate_opticalflow.py -raw_dir R [-dataset gen1|gen4]` -- the reference's command (generate_opticalflow.py:94-193, README 5.1 step 1): same flags, same directory and file names.
The time-surface pair of every label of R/test on the gfx950 encoder and the TV-L1 flow between the two (cv2.optflow, third-party as in
the reference) -> optical_flow_buffer/<file>_<t>.npy; without cv2.optflow the pairs go to time_surface_buffer/ instead (frlw_evd_amd/motion.py; pinned by tests/golden/motion.npz, written by the reference's own scripts)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from frlw_evd_amd import motion  # noqa: E402

if __name__ == "__main__":
    motion.main("generate_opticalflow")
