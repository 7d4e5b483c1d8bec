"""The operand cache protocol of the native train step (yolox/operand_cache.py, yolox/train_ops.py): when may a BaseConv forward
skip its weight layout (``w == NULL``), when may its backward reuse the forward's operands (``w_cache != NULL``), and is what
they then compute right.  Two oracles, neither reads private state: the same computation on a ``copy.deepcopy`` of the module
(new parameters, nothing cached: must be EQUAL, the layout kernels write the same operand whoever launches them) and torch
autograd in float64 (TOL as in test_train_ops_gpu.py; the weight states under test differ by their own magnitude, so a stale
operand misses TOL by orders of magnitude).  Launch decisions are observed at the ABI (the ``spy`` fixture)."""
import copy
import gc

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
TOL = 1e-3
PRECISIONS = ["f32", "bf16x3"]


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.fixture
def spy(monkeypatch):
    """Every frlw_baseconv_train_fwd / _bwd / frlw_conv_weight_layouts_batch call as (entry point, w is NULL, w_cache is NULL,
    fuse.split, Cout) -- for the batched layout (.., None, None, 0, number of table entries) -- then the call itself."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from frlw_evd_amd import _lib
    lib = _lib.load()
    calls = []
    fwd, bwd, batch = lib.frlw_baseconv_train_fwd, lib.frlw_baseconv_train_bwd, lib.frlw_conv_weight_layouts_batch

    def split(fuse):
        return 0 if fuse is None else int(fuse._obj.split)

    def spy_fwd(*a):
        calls.append(("fwd", a[1] is None, None, split(a[25]), a[9]))
        return fwd(*a)

    def spy_bwd(*a):
        calls.append(("bwd", None, a[21] is None, split(a[25]), a[13]))
        return bwd(*a)

    def spy_batch(*a):
        calls.append(("batch", None, None, 0, a[1]))
        return batch(*a)
    monkeypatch.setattr(lib, "frlw_baseconv_train_fwd", spy_fwd)
    monkeypatch.setattr(lib, "frlw_baseconv_train_bwd", spy_bwd)
    monkeypatch.setattr(lib, "frlw_conv_weight_layouts_batch", spy_batch)
    return calls


def _block(cin, cout, k, stride, seed):
    from frlw_evd_amd.yolox.network_blocks import BaseConv
    torch.manual_seed(seed)
    m = BaseConv(cin, cout, k, stride, act="silu").cuda().train()
    with torch.no_grad():
        m.conv.weight.normal_()
        m.bn.weight.uniform_(0.5, 1.5)
        m.bn.bias.normal_(0, 0.2)
    return m


def _params(m):
    return [p for blk in (m if isinstance(m, (list, tuple, torch.nn.Sequential)) else [m]) for p in (blk.conv.weight, blk.bn.weight, blk.bn.bias)]


def _fwd(m, x):
    from frlw_evd_amd.yolox import train_ops
    xl = x.clone().requires_grad_(True)
    assert train_ops.eligible(xl, m.conv, m.bn, m.act)
    return xl, train_ops.base_conv_train(xl, m.conv, m.bn)


def _bwd(m, xl, y, gy):
    """[y, dx, dw, dgamma, dbeta] of one block."""
    return [y.detach(), *torch.autograd.grad(y, [xl] + _params(m), gy)]


def _f64(blocks, x, gy):
    """[y, dx, (dw, dgamma, dbeta) per block] of the blocks in sequence: torch autograd in float64 on copies."""
    ref = [copy.deepcopy(b).double() for b in blocks]
    xr = x.detach().double().requires_grad_(True)
    y = xr
    for b in ref:
        y = b.act(b.bn(b.conv(y)))
    return [y.detach(), *torch.autograd.grad(y, [xr] + _params(ref), gy.double())]


def _assert_equal(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), (what, i, rel(a.double(), b.double()))


def _assert_close(got, want, what, tol=TOL):
    assert len(got) == len(want)
    errs = [rel(a.double(), b.double()) for a, b in zip(got, want)]
    assert max(errs) <= tol, (what, errs)


def _out_shape(m, x):
    k, s = m.conv.kernel_size[0], m.conv.stride[0]
    pad = (k - 1) // 2
    return (x.shape[0], m.conv.out_channels, (x.shape[2] + 2 * pad - k) // s + 1, (x.shape[3] + 2 * pad - k) // s + 1)


# ---- 1: one layer at two parity classes before any backward ---------------------------------------------------------------

@pytest.mark.parametrize("order", ["even_first", "odd_first"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_two_parity_classes_before_any_backward(precision, order, spy, monkeypatch):
    """A stride-2 3x3 layer on an even-sized input (data-gradient operand grouped by parity class), then on an odd-sized one
    (transposed gather), then both backwards in either order: the second forward has overwritten the data-gradient half of the
    cache, so the first one's backward must lay out again (w_cache == NULL), the second one's must not."""
    monkeypatch.setenv("FRLW_CONV_PRECISION", precision)
    m = _block(8, 16, 3, 2, seed=1)
    xs = [torch.randn(1, 8, 8, 8, device="cuda"), torch.randn(1, 8, 7, 9, device="cuda")]
    gys = [torch.randn(_out_shape(m, x), device="cuda") for x in xs]
    want = []
    for x, gy in zip(xs, gys):  # each on a fresh copy of its own, and in float64
        f = copy.deepcopy(m)
        want.append((_bwd(f, *_fwd(f, x), gy), _f64([m], x, gy)))
    mark = len(spy)
    runs = [_fwd(m, x) for x in xs]
    got = [None, None]
    for i in ((0, 1) if order == "even_first" else (1, 0)):
        got[i] = _bwd(m, *runs[i], gys[i])
    for i in (0, 1):
        _assert_equal(got[i], want[i][0], ("fresh copy", i))
        _assert_close(got[i], want[i][1], ("float64", i))
    seen = spy[mark:]
    assert [c[0] for c in seen] == ["fwd", "fwd", "bwd", "bwd"] and [c[1] for c in seen[:2]] == [False, False]
    null_by_input = dict(zip((0, 1) if order == "even_first" else (1, 0), [c[2] for c in seen[2:]]))
    assert null_by_input == {0: True, 1: False}


# ---- 2: a stacked pair, its first block alone, the pair again ---------------------------------------------------------------

def _pair_sequence(ca, cb, x, sequence):
    from frlw_evd_amd.yolox import train_ops
    leaves, outs = [], []
    for what in sequence:
        xl = x.clone().requires_grad_(True)
        leaves.append(xl)
        outs += list(train_ops.pair_train(xl, ca, cb)) if what == "pair" else [train_ops.base_conv_train(xl, ca.conv, ca.bn)]
    return leaves, outs


@pytest.mark.parametrize("cout,sequence,stack,retired", [
    (8, ("pair", "alone", "pair"), "1", 0),    # the first forward sizes the cache for the stacked operand: nothing to replace
    (8, ("pair", "alone", "pair"), "0", 0),
    (8, ("alone", "pair", "alone"), "1", 0),   # 8 and 8 + 8 channels pad to the same 32 operand columns / 16 rows: the cache is large enough
    (24, ("alone", "pair", "alone"), "1", 1),  # 24 -> 48 channels: 32 -> 64 columns, the stacked operand outgrows the cache: replaced once
    (24, ("alone", "pair", "alone"), "0", 0),  # (FRLW_TRAIN_STACK=0: two blocks, each with the cache of its own weight)
])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_pair_then_alone_then_pair(precision, cout, sequence, stack, retired, spy, monkeypatch):
    """Two 1x1 blocks reading one input as a stacked pair, the first block on its own, the pair again (and the other way round);
    ONE backward through everything.  While a HIP graph is live (_pins.pin()) a replaced cache is retired, not freed."""
    from frlw_evd_amd import _pins
    monkeypatch.setenv("FRLW_CONV_PRECISION", precision)
    monkeypatch.setenv("FRLW_TRAIN_STACK", stack)
    ca, cb = _block(8, cout, 1, 1, seed=2), _block(8, cout, 1, 1, seed=3)
    x = torch.randn(2, 8, 4, 4, device="cuda")
    gys = [torch.randn(2, cout, 4, 4, device="cuda") for what in sequence for _ in range(2 if what == "pair" else 1)]
    # fresh copies: every element of the sequence on a pair of its own (these runs also grow the shared scratch to its size)
    fresh_y, fresh_dx, fresh_dp, lo = [], [], None, 0
    for what in sequence:
        fa, fb = copy.deepcopy(ca), copy.deepcopy(cb)
        leaves, outs = _pair_sequence(fa, fb, x, (what,))
        g = torch.autograd.grad(outs, leaves + _params([fa, fb]), gys[lo:lo + len(outs)], allow_unused=True)
        lo += len(outs)
        fresh_y += [o.detach() for o in outs]
        fresh_dx.append(g[0])
        dp = [torch.zeros_like(p) if t is None else t for t, p in zip(g[1:], _params([fa, fb]))]
        fresh_dp = dp if fresh_dp is None else [a + b for a, b in zip(fresh_dp, dp)]
    # float64: the whole sequence, one backward
    ra, rb = copy.deepcopy(ca).double(), copy.deepcopy(cb).double()
    l64, o64 = [], []
    for what in sequence:
        xr = x.double().requires_grad_(True)
        l64.append(xr)
        o64 += [b.act(b.bn(b.conv(xr))) for b in ((ra, rb) if what == "pair" else (ra,))]
    g64 = torch.autograd.grad(o64, l64 + _params([ra, rb]), [g.double() for g in gys])
    gc.collect()
    before = _pins.live()
    _pins.pin()
    try:
        leaves, outs = _pair_sequence(ca, cb, x, sequence)
        node = "_PairStackTrainBackward" if stack == "1" else "_PairTrainBackward"
        assert type(outs[sequence.index("pair")].grad_fn).__name__ == node
        got = torch.autograd.grad(outs, leaves + _params([ca, cb]), gys)
        assert _pins.live()[1] - before[1] == retired
    finally:
        _pins.unpin()
    assert _pins.live()[0] == before[0] and (before[0] > 0 or _pins.live() == (0, 0))
    n = len(sequence)
    _assert_equal([o.detach() for o in outs], fresh_y, "fresh copy: outputs")
    _assert_equal(got[:n], fresh_dx, "fresh copy: input gradients")
    # parameter gradients are accumulated over the elements of the sequence by autograd, here by the test: three float32
    # terms summed in another order differ by at most 2 ulp of the largest partial sum (2^-22 relative to the largest entry)
    _assert_close(got[n:], fresh_dp, "fresh copy: parameter gradients", tol=1e-6)
    _assert_close([o.detach() for o in outs] + list(got), [o.detach() for o in o64] + list(g64), "float64")


# ---- 3: the precision switched on a live module -----------------------------------------------------------------------------

@pytest.mark.parametrize("first,second", [("f32", "bf16x3"), ("bf16x3", "f32")])
def test_precision_switch_on_a_live_module(first, second, spy, monkeypatch):
    m = _block(16, 16, 3, 2, seed=4)
    x = torch.randn(1, 16, 8, 8, device="cuda")
    gy = torch.randn(_out_shape(m, x), device="cuda")
    monkeypatch.setenv("FRLW_CONV_PRECISION", first)
    _bwd(m, *_fwd(m, x), gy)
    monkeypatch.setenv("FRLW_CONV_PRECISION", second)
    got = _bwd(m, *_fwd(m, x), gy)
    f = copy.deepcopy(m)
    _assert_equal(got, _bwd(f, *_fwd(f, x), gy), "fresh copy")
    _assert_close(got, _f64([m], x, gy), "float64")


# ---- 4, 5: the batched layout and what invalidates it ------------------------------------------------------------------------

def _three_layers(seed):
    return torch.nn.Sequential(_block(8, 8, 3, 1, seed), _block(8, 16, 3, 2, seed + 1), _block(16, 8, 1, 1, seed + 2))


def _step(model, x, gy):
    xl = x.clone().requires_grad_(True)
    y = model(xl)
    return [y.detach(), *torch.autograd.grad(y, [xl] + _params(model), gy)]


@pytest.mark.parametrize("edited", [0, 1, 2])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_batched_layout_then_an_edit(precision, edited, spy, monkeypatch):
    """layout_all_weights, then ONE weight is overwritten in place: that layer lays out its own operands (w != NULL), the other two
    take the batched ones (w == NULL)."""
    from frlw_evd_amd.yolox import train_ops
    monkeypatch.setenv("FRLW_CONV_PRECISION", precision)
    model = _three_layers(seed=10)
    x, gy = torch.randn(2, 8, 8, 8, device="cuda"), torch.randn(2, 8, 4, 4, device="cuda")
    _step(model, x, gy)
    assert train_ops.layout_all_weights(model) is True
    with torch.no_grad():
        model[edited].conv.weight.normal_()
    mark = len(spy)
    got = _step(model, x, gy)
    seen = spy[mark:]
    assert [c[0] for c in seen] == ["fwd"] * 3 + ["bwd"] * 3
    assert [c[1] for c in seen[:3]] == [i != edited for i in range(3)]
    assert [c[2] for c in seen[3:]] == [False] * 3
    _assert_equal(got, _step(copy.deepcopy(model), x, gy), "fresh copy")
    _assert_close(got, _f64(list(model), x, gy), "float64")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_batched_layout_storage_replaced(precision, spy, monkeypatch):
    """Weights whose storage is replaced (``.data = ...``: new address, same version counter) between two layout_all_weights calls:
    the second call lays the NEW storage out, every forward after it passes w == NULL."""
    from frlw_evd_amd.yolox import train_ops
    monkeypatch.setenv("FRLW_CONV_PRECISION", precision)
    model = _three_layers(seed=20)
    x, gy = torch.randn(2, 8, 8, 8, device="cuda"), torch.randn(2, 8, 4, 4, device="cuda")
    _step(model, x, gy)
    assert train_ops.layout_all_weights(model) is True
    model[1].conv.weight.data = model[1].conv.weight.data.clone()
    model[2].conv.weight.data = torch.randn_like(model[2].conv.weight.data)  # (and one with other values: its old operands would be wrong)
    assert train_ops.layout_all_weights(model) is True
    mark = len(spy)
    got = _step(model, x, gy)
    assert [c[1] for c in spy[mark:mark + 3]] == [True] * 3
    _assert_equal(got, _step(copy.deepcopy(model), x, gy), "fresh copy")
    _assert_close(got, _f64(list(model), x, gy), "float64")


@pytest.mark.parametrize("first,second", [("f32", "bf16x3"), ("bf16x3", "f32")])
def test_batched_layout_follows_a_precision_switch(first, second, spy, monkeypatch):
    """The model moves to the other arithmetic between two layout_all_weights calls: the plan is rebuilt for it (every forward
    after the second call passes w == NULL, which it only does for operands of its own precision)."""
    from frlw_evd_amd.yolox import train_ops
    monkeypatch.setenv("FRLW_CONV_PRECISION", first)
    model = _three_layers(seed=30)
    x, gy = torch.randn(2, 8, 8, 8, device="cuda"), torch.randn(2, 8, 4, 4, device="cuda")
    _step(model, x, gy)
    assert train_ops.layout_all_weights(model) is True
    monkeypatch.setenv("FRLW_CONV_PRECISION", second)
    _step(model, x, gy)
    assert train_ops.layout_all_weights(model) is True
    mark = len(spy)
    got = _step(model, x, gy)
    assert [c[1] for c in spy[mark:mark + 3]] == [True] * 3
    _assert_equal(got, _step(copy.deepcopy(model), x, gy), "fresh copy")
    _assert_close(got, _f64(list(model), x, gy), "float64")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_batched_layout_then_another_parity_and_back(precision, spy, monkeypatch):
    """layout_all_weights for the parity class of an even-sized input, a forward there (w == NULL), one on an odd-sized input (the
    layer lays its data-gradient operand out for the transposed gather), then the even-sized input again: the batched operands
    are gone, so this forward lays out again, and its backward is right."""
    from frlw_evd_amd.yolox import train_ops
    monkeypatch.setenv("FRLW_CONV_PRECISION", precision)
    model = torch.nn.Sequential(_block(8, 16, 3, 2, seed=50))
    m = model[0]
    xe, xo = torch.randn(1, 8, 8, 8, device="cuda"), torch.randn(1, 8, 7, 9, device="cuda")
    gy = torch.randn(_out_shape(m, xe), device="cuda")
    _bwd(m, *_fwd(m, xe), gy)
    assert train_ops.layout_all_weights(model) is True
    mark = len(spy)
    _fwd(m, xe)
    _fwd(m, xo)
    got = _bwd(m, *_fwd(m, xe), gy)
    f = copy.deepcopy(m)
    want = _bwd(f, *_fwd(f, xe), gy)
    assert [c[1] for c in spy[mark:mark + 3]] == [True, False, False]
    _assert_equal(got, want, "fresh copy")
    _assert_close(got, _f64([m], xe, gy), "float64")


# ---- 6: nothing outlives its weight -----------------------------------------------------------------------------------------

def test_nothing_outlives_its_weight(spy):
    """A dropped model leaves no record behind, and a fresh parameter -- wherever the allocators put it and its cache -- is never
    told that its operands are ready."""
    from frlw_evd_amd.yolox import operand_cache, train_ops
    x, gy = torch.randn(2, 8, 8, 8, device="cuda"), torch.randn(2, 8, 8, 8, device="cuda")

    def life(seed):
        """One single-layer model from its first forward to a step on the batched layout: (id of its weight, spy entries)."""
        mark = len(spy)
        model = torch.nn.Sequential(_block(8, 8, 3, 1, seed))
        _step(model, x, gy)
        assert train_ops.layout_all_weights(model) is True
        _step(model, x, gy)
        return id(model[0].conv.weight), spy[mark:]

    gc.collect()
    before = len(operand_cache._RECORDS)
    wid, _ = life(40)
    gc.collect()
    assert wid not in operand_cache._RECORDS and len(operand_cache._RECORDS) <= before
    for i in range(32):
        _, seen = life(40)  # the same seed: the same shapes, values and version counts as the model before it
        gc.collect()
        assert [c[:2] for c in seen if c[0] != "bwd"] == [("fwd", False), ("batch", None), ("fwd", True)], i
    assert len(operand_cache._RECORDS) <= before


# ---- 7: the steady state of the real models ---------------------------------------------------------------------------------

def _inputs(B, H, W, seed):
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.integers(0, 256, size=(B, 16, H, W, 1, 1)).astype(np.float32) / np.float32(255))
    lab = torch.zeros(B, 80, 5, dtype=torch.float64)
    lab[:, 0] = torch.tensor([0, (60.0 + seed) * W / 160, 50.0 * H / 128, 40.0 * W / 160, 30.0 * H / 128])
    lab[:, 1] = torch.tensor([1, 100.0 * W / 160, (90.0 - seed) * H / 128, 30.0 * W / 160, 50.0 * H / 128])
    return x.cuda(), lab.cuda()


@pytest.mark.parametrize("net,H,W", [("yolox", 128, 160),   # trainer and inputs of test_train_graph_gpu.py
                                     ("aed", 64, 96)])      # Darknet-21 recipe; 64 x 96: two map rows at stride 32 (the smoke run's size)
def test_steady_state_of_a_real_model(net, H, W, spy):
    """Three eager steps: in the first every forward lays out its own operands; from the second on ONE batched layout launch per step,
    every forward takes its operands (w == NULL), every backward reuses them (w_cache != NULL), the same calls in the same order."""
    from frlw_evd_amd.trainer import Trainer
    from frlw_evd_amd.yolox import build_yolox
    from frlw_evd_amd.yolox.model import build_aed, recipe_state_dict
    m = build_yolox(16, 2) if net == "yolox" else build_aed(16, 2)
    m.load_state_dict(recipe_state_dict(m, seed=31))
    tr = Trainer(m.cuda(), global_batch=4, nodes=1, iters_per_epoch=4, max_epoch=10, warmup_epochs=1, graph=False)
    steps = []
    for i in range(3):
        mark = len(spy)
        tr.train_step(*_inputs(4, H, W, i), i)
        steps.append(spy[mark:])
    assert len(steps[0]) > 40 and all(c[0] != "batch" for c in steps[0])
    assert all(c[1] is False for c in steps[0] if c[0] == "fwd")
    for s in steps[1:]:
        assert [c[0] for c in s].count("batch") == 1 and s[0][0] == "batch"
        assert all(c[1] is True for c in s if c[0] == "fwd"), [c for c in s if c[0] == "fwd" and not c[1]]
        assert all(c[2] is False for c in s if c[0] == "bwd"), [c for c in s if c[0] == "bwd" and c[2]]
    assert steps[1] == steps[2]
    assert [c for c in steps[0] if c[0] == "bwd"] == [c for c in steps[1] if c[0] == "bwd"]
    assert [c[3:] for c in steps[0] if c[0] == "fwd"] == [c[3:] for c in steps[1] if c[0] == "fwd"]
