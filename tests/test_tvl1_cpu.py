"""The host half of the native Dual TV-L1 solver (frlw_tvl1_plan, frlw_tvl1_workspace_bytes, the exports) and the numpy restatement
the GPU tests are held to (tests/tvl1_restated.py): that it recovers a known motion, and that the default-parameter cases are safe
yardsticks for iteration counts."""
import ctypes as C
import os

import numpy as np
import pytest

import tvl1_data as D
import tvl1_restated as R
from frlw_evd_amd import _lib, motion

LEVELS = {
    (17, 21): [(17, 21)],
    (40, 52): [(40, 52), (32, 42), (26, 34), (21, 27), (17, 22)],
    (240, 304): [(240, 304), (192, 243), (154, 194), (123, 155), (98, 124)],
    (720, 1280): [(720, 1280), (576, 1024), (461, 819), (369, 655), (295, 524)],
}


@pytest.mark.parametrize("shape", sorted(LEVELS))
def test_plan_reproduces_the_level_shapes(shape):
    assert motion.tvl1_plan(shape) == LEVELS[shape]
    assert R.plan(*shape) == LEVELS[shape]


def test_plan_refuses_a_side_below_16_and_cuts_the_pyramid_there():
    assert motion.tvl1_plan((15, 40)) == [] and motion.tvl1_plan((40, 15)) == []
    assert motion.tvl1_plan((20, 200)) == [(20, 200), (16, 160)]          # (13, 128) is dropped
    assert motion.tvl1_plan((240, 304), nscales=2) == LEVELS[(240, 304)][:2]
    assert _lib.load().frlw_tvl1_plan(240, 304, 5, 0.8, None) == 5         # the count alone


def test_workspace_query_is_host_only_monotone_and_64_bit():
    lib = _lib.load()
    prm = _lib.FrlwTvl1Params()
    sizes = [lib.frlw_tvl1_workspace_bytes(n, 720, 1280, C.byref(prm)) for n in range(1, 65)]
    assert all(b > a > 0 for a, b in zip(sizes, sizes[1:]))
    assert sizes[-1] > 2 ** 32 and sizes[-1] >= 64 * 720 * 1280 * 18 * 4      # 18 float planes per pixel and pair, and the pyramids
    assert lib.frlw_tvl1_workspace_bytes(64, 720, 1280, None) == sizes[-1]     # NULL = the defaults
    for n, H, W in ((0, 240, 304), (65, 240, 304), (1, 15, 304), (1, 240, 15), (-1, 240, 304)):
        assert lib.frlw_tvl1_workspace_bytes(n, H, W, C.byref(prm)) == 0
    assert lib.frlw_tvl1_workspace_bytes(1, 240, 304, C.byref(_lib.FrlwTvl1Params(nscales=1))) < lib.frlw_tvl1_workspace_bytes(1, 240, 304, None)
    bad = _lib.FrlwTvl1Params(median=3)
    assert lib.frlw_tvl1_workspace_bytes(1, 240, 304, C.byref(bad)) == 0


def test_exports_are_declared():
    lib = _lib.load()
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "frlw_evd.h")).read()
    for name in ("frlw_tvl1_plan", "frlw_tvl1_workspace_bytes", "frlw_tvl1_flow_batch", "frlw_tvl1_counts"):
        assert name + "(" in text, name
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert "frlw_tvl1_params_t" in text and C.sizeof(_lib.FrlwTvl1Params) == 44


def test_a_bad_call_is_refused_on_the_host():
    """NULL pointers and a frame with a side below 16 are answered before anything touches a device."""
    lib = _lib.load()
    before = motion.tvl1_counts()
    assert lib.frlw_tvl1_flow_batch(None, 1, 240, 304, None, None, None, None, 0, None) == _lib.FRLW_ERR_ARG
    one = C.c_void_p(4096)
    assert lib.frlw_tvl1_flow_batch(one, 1, 15, 304, None, one, None, one, 1 << 40, None) == _lib.FRLW_ERR_ARG
    assert lib.frlw_tvl1_flow_batch(one, 65, 240, 304, None, one, None, one, 1 << 40, None) == _lib.FRLW_ERR_ARG
    assert lib.frlw_tvl1_flow_batch(one, 1, 240, 304, None, one, None, one, 16, None) == _lib.FRLW_ERR_WORKSPACE
    assert motion.tvl1_counts() == before


def test_the_command_knows_its_solver_flag():
    a = motion.PARSERS["generate_opticalflow"]().parse_args(["-raw_dir", "R"])
    assert a.solver is None
    assert motion.PARSERS["generate_opticalflow"]().parse_args(["-raw_dir", "R", "-solver", "native"]).solver == "native"
    with pytest.raises(SystemExit):
        motion.PARSERS["generate_opticalflow"]().parse_args(["-raw_dir", "R", "-solver", "other"])
    if motion._tvl1() is None:
        with pytest.raises(SystemExit, match="-solver"):
            motion.generate_opticalflow("nowhere", "gen1", solver="cv2")


@pytest.fixture(scope="module")
def smooth_runs():
    out = {}
    for name, case in D.SMOOTH.items():
        a, b = D.blob_pair(*case)
        out[name] = (R.tvl1(a, b, np.float64), R.tvl1(a, b, np.float32))
    return out


@pytest.mark.parametrize("name", sorted(D.SMOOTH))
def test_restatement_recovers_a_known_shift(smooth_runs, name):
    """Sums of Gaussian blobs (sigma 2.5 .. 6) shifted analytically, the cases of tvl1_data.SMOOTH (low contrast, see there): the
    median interior endpoint error of the float64 restatement, measured 0.067 px for (1.5, -0.75) at 40 x 52, 0.0036 px for (3, -2)
    and 0.011 px for (6, 4) at 64 x 80 (the float32 restatement: the same to four digits; at full contrast 0.045, 0.005 and 0.005
    px).  At most 0.1 px is asserted, far below the half pixel at which a flow stops telling one-pixel motion from none."""
    shift = D.SMOOTH[name][2]
    for r in smooth_runs[name]:
        epe = R.interior_epe(r["flow"], shift)
        print(name, r["flow"].dtype, "median interior endpoint error", epe)
        assert epe <= 0.1


@pytest.mark.parametrize("name", sorted(D.SMOOTH))
def test_default_cases_are_safe_yardsticks(smooth_runs, name, golden_dir):
    """The golden maker's own check: both restatements run the same iteration counts (the ones tests/golden/tvl1.npz holds), and
    the last error of every (level, warp) lies at least 5 % away from the threshold, so no summation order changes a count.
    Measured: the closest error lies 7.7 % (40 x 52), 5.7 % (64 x 80, (3, -2)) and 5.7 % (64 x 80, (6, 4)) off it, in both dtypes."""
    r64, r32 = smooth_runs[name]
    assert np.array_equal(r64["iters"], r32["iters"])
    assert np.array_equal(r64["iters"], np.load(os.path.join(golden_dir, "tvl1.npz"))[f"smooth_{name}_iters"])
    for r in (r64, r32):
        rel = np.abs(r["errors"] / r["eps"][:, None] - 1.0)
        print(name, r["flow"].dtype, "closest error to the threshold", rel.min())
        assert rel.min() >= 0.05
