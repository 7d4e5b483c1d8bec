"""The native Dual TV-L1 solver on the GPU (frlw_tvl1_flow_batch through ``motion.tvl1_flow``) against the float64 numpy
restatement of tests/tvl1_restated.py.

Bounds: float32 arithmetic is the only licensed difference, so per case the device may differ from the float64 restatement by at
most four times what the float32 restatement differs from it (tests/golden/tvl1.npz, written by tests/golden/make_golden_tvl1.py;
the margin ``density_bound`` has in tests/test_motion_gpu.py).  A wrong stencil shows as 1e-1, not as 1e-3.  Measured
max |float32 - float64| of the restatements: 5.0e-8 (17 x 21), 4.4e-5 (40 x 52), 3.8e-2 (noisy 64 x 80), 1.8e-3 (720 x 1280) for
the short schedules; 4.0e-5, 2.4e-4, 1.1e-4 for the three default-parameter shifts.  On an MI355X the device gave exactly the
float32 restatement's flows in all seven cases (the build contracts no multiply-add and the sums are written in its order)."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import motion_data  # noqa: E402
import tvl1_data as D  # noqa: E402
import tvl1_restated as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def motion():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from frlw_evd_amd import motion
    return motion


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "tvl1.npz")))


def dev(*pairs):
    return torch.from_numpy(np.stack([np.stack(p) for p in pairs])).cuda()


# ---- fixed short schedules: every kernel, pointwise ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["17x21", "40x52", "noisy_64x80", "720x1280"])
def test_short_schedule_equals_the_restatement(motion, golden, name):
    """17 x 21: smaller than one tile in both directions, one level, gradient + warp + median + one iteration.  40 x 52: five
    levels of odd sizes, an upsample at every step.  The noisy pair: sparse edges, impulse cells, large areas of grad = 0 exactly.
    720 x 1280: many tiles, the row stride of a large frame, a last level of 295 x 524."""
    pair, prm = D.short_cases()[name]
    want = R.tvl1(pair[0], pair[1], np.float64, **prm)
    flow, iters = motion.tvl1_flow(dev(pair), params=prm, return_iters=True)
    assert flow.dtype == torch.float32 and tuple(flow.shape) == (1,) + pair[0].shape + (2,)
    assert motion.tvl1_plan(pair[0].shape, prm["nscales"]) == want["levels"]
    assert np.array_equal(iters[0].cpu().numpy(), want["iters"])     # epsilon = 0: warps x outer x inner on every level
    diff = np.abs(flow[0].cpu().numpy().astype(np.float64) - want["flow"]).max()
    bound = 4 * float(golden[f"short_{name}_bound"])
    print(name, "max |device - float64|", diff, "allowed", bound, "largest flow", np.abs(want["flow"]).max())
    assert np.abs(want["flow"]).max() > 0.5 and diff <= bound


# ---- default parameters ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(D.SMOOTH))
def test_default_parameters_on_a_known_shift(motion, golden, name):
    """The iteration counts of the restatement (tests/test_tvl1_cpu.py holds the cases to the condition that makes them
    comparable), the float64 flow within four times the float32 restatement's distance from it, and the true shift within 0.1 px
    (median interior endpoint error)."""
    shift = D.SMOOTH[name][2]
    flow, iters = motion.tvl1_flow(dev(D.blob_pair(*D.SMOOTH[name])), return_iters=True)
    got = flow[0].cpu().numpy()
    diff = np.abs(got.astype(np.float64) - golden[f"smooth_{name}_flow"]).max()
    epe = R.interior_epe(got, shift)
    print(name, "iterations", iters[0].cpu().numpy().tolist(), "max |device - float64|", diff, "allowed", 4 * float(golden[f"smooth_{name}_bound"]),
          "median interior endpoint error", epe)
    assert np.array_equal(iters[0].cpu().numpy(), golden[f"smooth_{name}_iters"])
    assert diff <= 4 * float(golden[f"smooth_{name}_bound"])
    assert epe <= 0.1


def test_default_parameters_on_a_noisy_pair(motion, golden):
    """Single impulse cells differ by pixels between the float32 and the float64 restatement after hundreds of iterations (measured
    4.0 px), the box means by 9e-4 relative at most: what the evaluation reads is the density of a box, so that is what is held
    -- through ``box_flow_sums`` on the tensor ``tvl1_flow`` returned -- within four times the restatements' difference, and no
    box may change its motion-level bucket."""
    from frlw_evd_amd.settings import MOTION_LEVEL_EDGES
    flows = motion.tvl1_flow(dev(D.surface_pair(*D.NOISY)))
    sums = motion.box_flow_sums(flows, D.NOISY_BOXES).cpu().numpy()
    area = (D.NOISY_BOXES[:, 2] - D.NOISY_BOXES[:, 1]) * (D.NOISY_BOXES[:, 4] - D.NOISY_BOXES[:, 3])
    got, d64, d32 = sums / (area + 1e-8), golden["noisy_density64"], golden["noisy_density32"]
    print("densities", got.tolist(), "float64", d64.tolist(), "allowed", (4 * np.abs(d32 - d64)).tolist())
    assert np.all(np.abs(got - d64) <= 4 * np.abs(d32 - d64))
    edges = np.asarray(MOTION_LEVEL_EDGES["gen1"])
    assert np.array_equal(np.searchsorted(edges, got, side="right"), np.searchsorted(edges, d64, side="right"))


# ---- batch independence and determinism -------------------------------------------------------------------------------------------
def test_a_pair_does_not_depend_on_its_batch(motion):
    """A, B, A at 240 x 304 with default parameters: outputs 0 and 2 equal bit for bit, equal A encoded alone, equal a second run."""
    a = D.surface_pair(240, 304, 7410, (2.0, 1.0))
    b = D.surface_pair(240, 304, 7411, (0.5, -1.5))
    batch = dev(a, b, a)
    flows, iters = motion.tvl1_flow(batch, return_iters=True)
    again = motion.tvl1_flow(batch)
    alone, alone_iters = motion.tvl1_flow(dev(a), return_iters=True)
    assert torch.equal(flows[0], flows[2]) and torch.equal(flows, again) and torch.equal(flows[0], alone[0])
    assert torch.equal(iters[0], iters[2]) and torch.equal(iters[0], alone_iters[0])
    assert not torch.equal(flows[0], flows[1]) and float(flows.abs().max()) > 0.5 and bool(torch.isfinite(flows).all())


def test_65_pairs_take_two_calls(motion):
    pairs = np.stack([np.stack(D.blob_pair(17, 21, (0.3 + 0.02 * i, -0.4 + 0.01 * i), seed=7420 + i % 5)) for i in range(65)])
    d = torch.from_numpy(pairs).cuda()
    before = motion.tvl1_counts()[0]
    flows = motion.tvl1_flow(d)
    assert motion.tvl1_counts()[0] - before == 2 and tuple(flows.shape) == (65, 17, 21, 2)
    for i in (0, 1, 31, 63, 64):
        assert torch.equal(flows[i], motion.tvl1_flow(d[i:i + 1])[0]), i


def test_early_and_late_convergence_side_by_side(motion):
    """Two equal images converge in the first iteration of every warp (the error is 0), a shifted pair does not: each pair keeps
    the iteration counts it has alone."""
    a, b = D.blob_pair(40, 52, (1.5, -0.75))
    still, moving = (a, a), (a, b)
    flows, iters = motion.tvl1_flow(dev(still, moving, still), return_iters=True)
    one_still, it_still = motion.tvl1_flow(dev(still), return_iters=True)
    one_moving, it_moving = motion.tvl1_flow(dev(moving), return_iters=True)
    assert torch.equal(iters[0], it_still[0]) and torch.equal(iters[2], it_still[0]) and torch.equal(iters[1], it_moving[0])
    assert torch.equal(flows[0], one_still[0]) and torch.equal(flows[1], one_moving[0])
    assert int(it_still.max()) == 1 and int(it_moving.min()) > 1 and float(one_still.abs().max()) == 0.0


# ---- arguments ------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise_and_enqueue_nothing(motion):
    before = motion.tvl1_counts()
    good = torch.zeros((1, 2, 17, 21), dtype=torch.uint8, device="cuda")
    for bad in (good.cpu(), good.float(), good[0], good[:, :1], torch.zeros((1, 2, 15, 40), dtype=torch.uint8, device="cuda"),
                torch.zeros((1, 2, 40, 15), dtype=torch.uint8, device="cuda")):
        with pytest.raises(ValueError):
            motion.tvl1_flow(bad)
    with pytest.raises(ValueError):
        motion.tvl1_flow(good, params={"median": 3})
    with pytest.raises(TypeError):
        motion.tvl1_flow(good, params={"gamma": 0.1})
    assert motion.tvl1_counts() == before
    assert tuple(motion.tvl1_flow(good[:0]).shape) == (0, 17, 21, 2) and motion.tvl1_counts() == before


# ---- the command ------------------------------------------------------------------------------------------------------------------------
def test_generate_opticalflow_native_feeds_the_statistics(motion, tmp_path):
    """``-solver native`` on the fabricated dataset of tests/motion_data.py: one (240, 304, 2) float32 file per label, nothing on
    the second run, no cv2; ``statistics_gt`` then runs on those files -- the first time this chain runs without OpenCV.  The
    default call still saves the pairs (or OpenCV's flows) as before."""
    import sys
    raw = motion_data.build(str(tmp_path), with_flows=False)
    flow_dir, surface_dir = str(tmp_path / "optical_flow_buffer"), str(tmp_path / "time_surface_buffer")
    n_labels = sum(len(motion_data.label_times(name)) for name in motion_data.FILES)
    had_cv2 = "cv2" in sys.modules
    assert motion.generate_opticalflow(raw, "gen1", flow_dir, surface_dir, solver="native") == n_labels
    assert motion.generate_opticalflow(raw, "gen1", flow_dir, surface_dir, solver="native") == 0
    assert had_cv2 or "cv2" not in sys.modules
    assert not os.path.exists(surface_dir) and len(os.listdir(flow_dir)) == n_labels
    for name in motion_data.FILES:
        for t in motion_data.label_times(name):
            flow = np.load(os.path.join(flow_dir, f"{name}_{t}.npy"))
            assert flow.dtype == np.float32 and flow.shape == (240, 304, 2) and np.isfinite(flow).all()
    out = motion.statistics_gt(raw, "gen1", flow_dir=flow_dir, out_dir=str(tmp_path / "statistics_result"))
    stats = np.load(out)
    assert len(stats["densitys"]) == len(stats["gts"]) > 0 and np.isfinite(stats["densitys"]).all()
    other = str(tmp_path / "default_flows")
    assert motion.generate_opticalflow(raw, "gen1", other, surface_dir) == n_labels
    assert len(os.listdir(surface_dir if motion._tvl1() is None else other)) == n_labels
    with pytest.raises(ValueError):
        motion.generate_opticalflow(raw, "gen1", flow_dir, surface_dir, solver="opencv")
