"""SimOTA and the native loss (csrc/simota.hip: k_candidates, k_rows, k_resolve, k_loss_decode, k_loss_fwd, k_loss_final,
k_loss_bwd) in the regimes of a trained detector: the cases of tests/simota_cases.py -- dynamic k from 1 to 9, dozens of
contested anchors, 0 to 9 candidates, A up to the limit of 9600 (dynamic LDS above the 48 KB default from A = 3073 on), 80
boxes, 1 / 2 / 4 levels, 1 / 20 classes, saturated logits, tied corners.  tests/test_simota_cases_cpu.py shows that every
case reaches its regime and that the reference decides nothing by a near-tie.

The judge is the reference's per-image procedure on CPU tensors (``losses.yolox_losses`` / ``get_assignments`` on ``.cpu()``
inputs, differentiated by autograd; pinned to the reference by tests/test_detector_cpu.py); it shares no code with the
kernels.

Assignment: exact.  Foreground mask, matched box, num_fg and nlabel equal, matched IoU within rtol 1e-12.

Loss tuple and gradients: the hard bound is the project's L3 bound (1e-3, max-abs over max-abs).  The working bound is the
larger of the figures tests/test_detector_gpu.py uses for the native loss (1e-6 relative on the tuple, 2e-6 * max on a
gradient) and 4 times the distance between two executions of the reference itself -- on the CPU and, with ``_FORCE_LOOP``,
in torch on the GPU -- which is the reference's own float32 / libm noise.

Observed on an MI355X, native against the CPU reference (tuple: largest relative error of an element; gradient: largest
max-abs over max-abs of a level, and the same figure for the reference's own GPU execution against its CPU execution):
    crowded-1mpx    tuple 4.3e-08   gradient 2.0e-08   (reference against itself 2.0e-08)
    exact-limit     tuple 3.4e-08   gradient 2.8e-09   (reference against itself 2.8e-09)
    few-candidates  tuple 5.0e-08   gradient 1.0e-08   (reference against itself 2.0e-08)
    levels-1        tuple 2.6e-08   gradient 3.8e-09   (reference against itself 3.8e-09)
    levels-2        tuple 1.8e-08   gradient 2.8e-09   (reference against itself 2.8e-09)
    levels-4        tuple 4.5e-08   gradient 2.0e-09   (reference against itself 2.1e-09)
    nc-1            tuple 9.9e-08   gradient 2.1e-09   (reference against itself 2.1e-09)
    nc-20           tuple 4.4e-08   gradient 1.5e-08   (reference against itself 1.5e-08)
    near-limit      tuple 5.7e-08   gradient 2.8e-08   (reference against itself 2.8e-08)
    saturated       tuple 1.8e-08   gradient 2.4e-09   (reference against itself 9.6e-09)
    small-crowded   tuple 4.6e-08   gradient 1.0e-08   (reference against itself 1.1e-08)
    tied-corners    tuple 7.8e-08   gradient 8.2e-08   (reference against itself 8.2e-08)
    no-candidate    not yet measured (the first GPU run stopped at a mistake in this test's own arithmetic)
Assignment: no anchor differs in any of these cases.  Not yet run on a GPU: the no-candidate, tied-corner-gradient,
run-to-run and anchor-limit tests below.
"""
import ctypes as C
import functools

import pytest

torch = pytest.importorskip("torch")

import simota_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu
L3 = 1e-3
TUPLE_REL, GRAD_REL = 1e-6, 2e-6  # the figures of test_native_loss_equals_autograd_loss
WITH_REFERENCE = sorted(n for n in sc.CASES if n != "no-candidate")


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


def _loss_and_grads(levels, strides, labels, nc, radius, force_loop=False):
    """Tuple values and the gradient of every level for an upstream gradient on four tuple elements at once."""
    from frlw_evd_amd.yolox import losses
    leaves = [t.clone().requires_grad_(True) for t in levels]
    try:
        losses._FORCE_LOOP = force_loop
        tup = losses.yolox_losses(leaves, strides, labels, nc, radius)
    finally:
        losses._FORCE_LOOP = False
    if leaves[0].is_cuda and not force_loop:
        assert isinstance(tup[5], torch.Tensor) and tup[5].is_cuda  # the native result, not the per-image procedure's float
    (tup[0] + 0.5 * tup[1] + 2.0 * tup[2] - 0.25 * tup[3]).backward()
    return [float(v.detach()) if isinstance(v, torch.Tensor) else float(v) for v in tup], [l.grad.detach().cpu() for l in leaves]


@functools.lru_cache(maxsize=None)
def _cpu(name):
    case, _ = sc.cached(name)
    return _loss_and_grads(case.levels, case.strides, case.labels, case.nc, case.radius)


@functools.lru_cache(maxsize=None)
def _native(name):
    case, _ = sc.cached(name)
    dev = torch.device("cuda")
    return _loss_and_grads([t.to(dev) for t in case.levels], case.strides, case.labels.to(dev), case.nc, case.radius)


def _tuple_err(got, want):
    return max(abs(g - w) / abs(w) if w != 0.0 else (0.0 if g == 0.0 else float("inf")) for g, w in zip(got, want))


def _grad_err(got, want):
    return float((got - want).abs().max() / want.abs().max())


def _check_image(a, fg, mgt, miou, nfg, nlab, b):
    """One image of ``simota_assign`` against the reference's Assignment ``a``: no mismatching anchor allowed."""
    assert int(nlab[b]) == a.n
    assert torch.equal(fg[b], a.fg), f"image {b}: {int((fg[b] != a.fg).sum())} anchors differ in the foreground set"
    assert int(nfg[b]) == a.num_fg == int(a.fg.sum())
    assert torch.equal(mgt[b][a.fg].long(), a.matched_gt), f"image {b}: matched boxes differ"
    assert bool((mgt[b][~a.fg] == -1).all())
    assert torch.allclose(miou[b][a.fg], a.matched_iou, rtol=1e-12, atol=0)


def _assign(case, gpu):
    from frlw_evd_amd.yolox import losses
    outputs, xs, ys, ss = sc.decode(case.levels, case.strides)  # on the CPU: both sides get the same bits
    out = losses.simota_assign(outputs.to(gpu), case.labels.to(gpu), xs.to(gpu), ys.to(gpu), ss.to(gpu), case.nc, case.radius)
    return [t.cpu() for t in out]


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_assignment_equals_the_reference(gpu, name):
    case, ref = sc.cached(name)
    fg, mgt, miou, nfg, nlab = _assign(case, gpu)
    for b, a in enumerate(ref):
        if a.n_cand == 0:
            # no candidate: the reference raises (topk with k = 1 on an empty row); k_rows finds no best anchor in either
            # loop, so the image has no foreground -- defined behaviour of the native path
            assert name == "no-candidate" and b == case.meta["empty_image"] and int(nlab[b]) == a.n == 1
            assert not bool(fg[b].any()) and int(nfg[b]) == 0
            assert bool((mgt[b] == -1).all()) and bool((miou[b] == 0.0).all())
            continue
        _check_image(a, fg, mgt, miou, nfg, nlab, b)


@pytest.mark.parametrize("name", WITH_REFERENCE)
def test_loss_and_gradients_equal_the_reference(gpu, name):
    case, _ = sc.cached(name)
    want, gwant = _cpu(name)
    got, ggot = _native(name)
    loop, gloop = _loss_and_grads([t.to(gpu) for t in case.levels], case.strides, case.labels.to(gpu), case.nc,
                                  case.radius, force_loop=True)
    assert want[0] > 0 and want[5] > 0 and want[4] == 0.0 and got[4] == 0.0
    noise = _tuple_err(loop, want)
    err = _tuple_err(got, want)
    print(f"{name}: tuple native-vs-CPU {err:.2e} (reference GPU-vs-CPU {noise:.2e})")
    assert err <= L3
    assert err <= max(TUPLE_REL, 4.0 * noise)
    assert any(float(g[:, :4].abs().max()) > 0 for g in gwant)  # box gradients are exercised
    for l, (a, w, r) in enumerate(zip(ggot, gwant, gloop)):
        assert a.shape == w.shape and bool(torch.isfinite(a).all())
        noise, err = _grad_err(r, w), _grad_err(a, w)
        print(f"{name}: level {l} gradient native-vs-CPU {err:.2e} (reference GPU-vs-CPU {noise:.2e})")
        assert err <= L3
        assert err <= max(GRAD_REL, 4.0 * noise)


def test_no_candidate_image_has_no_foreground_and_a_finite_loss(gpu):
    """An image whose only box has no candidate anchor.  The reference's procedure raises there; the native path gives the
    image no foreground anchor.  The loss and every gradient are finite -- and, since an image without foreground only
    adds its objectness terms, equal to the reference's on the same batch with that box removed; only the last tuple
    element, num_fg / num_gt, still counts the box."""
    case, ref = sc.cached("no-candidate")
    b = case.meta["empty_image"]
    got, ggot = _native("no-candidate")
    assert all(torch.isfinite(torch.tensor(got))) and all(bool(torch.isfinite(g).all()) for g in ggot)
    assert float(ggot[0][b, :4].abs().max()) == 0.0 and float(ggot[0][b, 5:].abs().max()) == 0.0  # background only
    assert float(ggot[0][b, 4].abs().max()) > 0.0
    labels = case.labels.clone()
    labels[b] = 0.0
    want, gwant = _loss_and_grads(case.levels, case.strides, labels, case.nc, case.radius)
    loop, gloop = _loss_and_grads([t.to(gpu) for t in case.levels], case.strides, labels.to(gpu), case.nc, case.radius,
                                  force_loop=True)
    n_gt = ref[1 - b].n
    assert got[5] == pytest.approx(want[5] * n_gt / (n_gt + 1), rel=1e-12)
    noise, err = _tuple_err(loop[:5], want[:5]), _tuple_err(got[:5], want[:5])
    print(f"no-candidate: tuple native-vs-CPU {err:.2e} (reference GPU-vs-CPU {noise:.2e})")
    assert err <= L3 and err <= max(TUPLE_REL, 4.0 * noise)
    for l, (a, w, r) in enumerate(zip(ggot, gwant, gloop)):
        noise, err = _grad_err(r, w), _grad_err(a, w)
        print(f"no-candidate: level {l} gradient native-vs-CPU {err:.2e} (reference GPU-vs-CPU {noise:.2e})")
        assert err <= L3 and err <= max(GRAD_REL, 4.0 * noise)


def test_tied_corner_gradients(gpu):
    """Predictions whose corners equal the box's take the 0.5 branches of k_loss_bwd (torch.max / torch.min split the
    gradient of a tie in halves).  Three foreground anchors: all four corners tied (the prediction is the box, IoU = 1),
    the top-left two, the bottom-right two.

    With all four corners tied the halves cancel: IoU = 1 is the maximum, the gradient of the reference is exactly zero in
    all four box channels, so a non-zero value cannot be demanded of that anchor; the kernel must reproduce the zero
    (taking a tie as 'mine' or as 'the other's' leaves a gradient of the order of the largest one in the level).  The two
    anchors with two tied corners carry the non-zero gradients through the same branches."""
    case, _ = sc.cached("tied-corners")
    want, gwant = _cpu("tied-corners")
    got, ggot = _native("tied-corners")
    loop, gloop = _loss_and_grads([t.to(gpu) for t in case.levels], case.strides, case.labels.to(gpu), case.nc,
                                  case.radius, force_loop=True)
    bound = max(GRAD_REL, 4.0 * _grad_err(gloop[0], gwant[0])) * float(gwant[0].abs().max())
    for n_ties, (lvl, y, x) in zip((4, 2, 2), case.meta["tied"]):
        g, w = ggot[lvl][0, :4, y, x], gwant[lvl][0, :4, y, x]
        print(f"tied-corners: {n_ties} ties: native {g.tolist()} CPU {w.tolist()}")
        if n_ties == 4:
            assert bool((w == 0.0).all())
        else:
            assert bool((w != 0.0).all()) and bool((g != 0.0).all())
        assert float((g - w).abs().max()) <= bound
        assert float(ggot[lvl][0, 4, y, x]) != 0.0 and float(ggot[lvl][0, 5:, y, x].abs().min()) > 0.0  # foreground


def test_crowded_1mpx_twice_gives_the_same_bits(gpu):
    """The sums are ordered (partials per workgroup, added in workgroup order): same results and gradients on every run."""
    case, _ = sc.cached("crowded-1mpx")
    first, gfirst = _native("crowded-1mpx")
    second, gsecond = _loss_and_grads([t.to(gpu) for t in case.levels], case.strides, case.labels.to(gpu), case.nc,
                                      case.radius)
    assert first == second
    assert all(torch.equal(a, b) for a, b in zip(gfirst, gsecond))
    assert all(torch.equal(a, b) for a, b in zip(_assign(case, gpu), _assign(case, gpu)))


def _raw_assign(gpu, preds, labels, xs, ys, st, nc, radius, fill=None):
    """frlw_simota_assign called the way ``losses.simota_assign`` calls it; ``fill`` = sentinels written into the outputs
    first.  Returns (status, fg, matched_gt, matched_iou, num_fg, nlabel)."""
    from frlw_evd_amd import _lib
    lib = _lib.load()
    B, A, _ = preds.shape
    G = labels.shape[1]
    preds, labels = preds.to(gpu).float().contiguous(), labels.to(gpu).double().contiguous()
    xs, ys, st = (t.to(gpu).reshape(-1).float().contiguous() for t in (xs, ys, st))
    fg = torch.empty((B, A), dtype=torch.uint8, device=gpu)
    mgt = torch.empty((B, A), dtype=torch.int32, device=gpu)
    miou = torch.empty((B, A), dtype=torch.float64, device=gpu)
    nfg = torch.empty((B,), dtype=torch.int32, device=gpu)
    nlab = torch.empty((B,), dtype=torch.int32, device=gpu)
    if fill is not None:
        fg.fill_(fill[0]); mgt.fill_(fill[1]); miou.fill_(fill[2]); nfg.fill_(fill[1]); nlab.fill_(fill[1])
    need = lib.frlw_simota_workspace_bytes(B, A, G)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    rc = lib.frlw_simota_assign(preds.data_ptr(), labels.data_ptr(), xs.data_ptr(), ys.data_ptr(), st.data_ptr(), B, A, G, nc,
                                C.c_float(radius), fg.data_ptr(), mgt.data_ptr(), miou.data_ptr(), nfg.data_ptr(),
                                nlab.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream(gpu).cuda_stream)
    torch.cuda.synchronize()
    return rc, fg.cpu(), mgt.cpu(), miou.cpu(), nfg.cpu(), nlab.cpu()


def test_anchor_limit_of_frlw_simota_assign(gpu):
    """A = 9600 (two float64 rows = 150 KB of dynamic LDS) is served and right; A = 9601 is refused before any kernel that
    writes the outputs has run.  ``losses.NATIVE_MAX_ANCHORS`` is this limit."""
    from frlw_evd_amd import _lib
    from frlw_evd_amd.yolox import losses
    assert losses.NATIVE_MAX_ANCHORS == 9600
    case, ref = sc.cached("exact-limit")
    outputs, xs, ys, ss = sc.decode(case.levels, case.strides)
    assert outputs.shape[1] == losses.NATIVE_MAX_ANCHORS
    rc, fg, mgt, miou, nfg, nlab = _raw_assign(gpu, outputs, case.labels, xs, ys, ss, case.nc, case.radius)
    assert rc == _lib.FRLW_OK
    _check_image(ref[0], fg.bool(), mgt, miou, nfg, nlab, 0)
    # one level of 9601 x 1 cells
    A = losses.NATIVE_MAX_ANCHORS + 1
    gen = torch.Generator().manual_seed(5)
    level = torch.randn((1, 5 + case.nc, A, 1), generator=gen) * 0.5
    outputs, xs, ys, ss = sc.decode([level], [8])
    assert outputs.shape[1] == A
    labels = torch.zeros((1, 80, 5), dtype=torch.float64)
    labels[0, 0] = torch.tensor([1.0, 4.0, 400.0, 30.0, 60.0])
    rc, fg, mgt, miou, nfg, nlab = _raw_assign(gpu, outputs, labels, xs, ys, ss, case.nc, case.radius, fill=(0xAB, -77, -7.5))
    assert rc == _lib.FRLW_ERR_UNSUPPORTED
    assert bool((fg == 0xAB).all()) and bool((mgt == -77).all()) and bool((miou == -7.5).all())
    with pytest.raises(ValueError):
        losses.simota_assign(outputs.to(gpu), labels.to(gpu), xs.to(gpu), ys.to(gpu), ss.to(gpu), case.nc, case.radius)
