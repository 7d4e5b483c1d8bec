"""Every form of the convolution family (conv_mfma.h launch_conv, wgrad_mfma.h launch_wgrad_tiles, the split-K reductions, the
parity classes of a stride-2 data gradient, the half-batch split, the detector epilogues) against float64 torch, through the
C ABI so that the raw convolution output is visible.

One table of cases; each names the forms it must reach, and each test asserts that the set of frlw_conv_path_counts counters
its call moved is exactly that set -- a retune of a threshold that moves a shape to another form fails here instead of
silently dropping coverage.  test_every_form_has_a_case checks that the table reaches every counter.

Two judgements per case and arithmetic:
  (a) integer data: x, w, dz in {-3..3}, integer bias.  Every partial sum stays far below 2^24 and every value is exact in
      bf16, so float32 AND bf16x3 must equal the float64 reference bit for bit whatever the summation order: a dropped,
      doubled or misplaced tap, split, padding element or parity class is an integer-sized error.  Outputs are NaN before
      every call (a tile nobody wrote fails too).  With an activation the epilogue's hardware exp / reciprocal round: those
      cases use sparse weights (pre-activations of a few units) and 4e-6 relative against the float64 activation.
  (b) randn + 0.5 data: |y - ref| <= tol * (|x| (*) |w|) element by element, the right side the same operation on absolute
      values in float64; tol = 1e-5 (float32), 1e-4 (bf16x3).  Worst ratio observed on an MI355X: 0.16 (float32),
      0.088 (bf16x3).  The train forward's BatchNorm mean and variance are held to the same bound per channel.
A negative control on the reference side (one tap zeroed, one 16-wide k-tile dropped) shows that the bound in (b) rejects
such errors.  The train-path backward cases are judged by (b) only: their dz comes out of the BatchNorm backward."""
import ctypes as C
import zlib

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL = {0: 1e-5, 1: 1e-4}
PREC = {"f32": 0, "bf16x3": 1}
ACT_NONE, ACT_SILU, ACT_SIGMOID = 0, 1, 2
SCRATCH = 8 * 1024 * 1024
WORST = {}  # (precision) -> worst |err| / bound of the (b) judgements


def _lib():
    from frlw_evd_amd import _lib as L
    return L, L.load()


def counts():
    L, lib = _lib()
    n = len(L.CONV_PATHS)
    c = (C.c_uint64 * n)()
    assert lib.frlw_conv_path_counts(c, n) == n
    return list(c)


def forms_moved(before):
    L, _ = _lib()
    return {L.CONV_PATHS[i] for i, (a, b) in enumerate(zip(before, counts())) if b != a}


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def check_rc(rc, what):
    L, _ = _lib()
    assert rc == L.FRLW_OK, f"{what} -> {rc}"


# ---- data and references ---------------------------------------------------------------------------------------------

def gen(shape, mode, g, sparse_k=0):
    """mode 'int': {-3..3}; 'randn': randn + 0.5.  sparse_k > 0 (weights of a case with an activation, integer mode): {-1, 0, 1}
    with about three non-zero taps per output, so pre-activations stay a few units and the activation does not saturate."""
    if mode == "int":
        if sparse_k:
            v = torch.randint(-1, 2, shape, generator=g, device="cuda").float()
            return v * (torch.rand(shape, generator=g, device="cuda") < 3.0 / sparse_k).float()
        return torch.randint(-3, 4, shape, generator=g, device="cuda").float()
    return torch.randn(shape, generator=g, device="cuda") + 0.5


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


def conv_ref(x, w, stride):
    """NHWC float64 forward convolution, padding (k - 1) / 2."""
    k = w.shape[-1]
    return nhwc(torch.nn.functional.conv2d(nchw(x.double()), w.double(), stride=stride, padding=(k - 1) // 2))


def dgrad_ref(dz, w, stride, H, W):
    B, Cin, k = dz.shape[0], w.shape[1], w.shape[-1]
    return nhwc(torch.nn.grad.conv2d_input((B, Cin, H, W), w.double(), nchw(dz.double()), stride=stride, padding=(k - 1) // 2))


def wgrad_ref(x, dz, wshape, stride):
    k = wshape[-1]
    return torch.nn.grad.conv2d_weight(nchw(x.double()), wshape, nchw(dz.double()), stride=stride, padding=(k - 1) // 2)


def act_ref(v, act, sig_from=0):
    if act == ACT_SILU:
        return v * torch.sigmoid(v)
    if act == ACT_SIGMOID:
        out = v.clone()
        out[..., sig_from:] = torch.sigmoid(v[..., sig_from:])
        return out
    return v


def judge(got, ref, absref, mode, prec, what, act=ACT_NONE, res=None, sig_from=0):
    """(a) / (b) above.  ref = act(conv + bias) before any residual; absref = |x| (*) |w| + |bias|; res: added after the activation
    (with an activation the bound also carries its largest slope and the 4e-6 of the hardware exp / reciprocal)."""
    assert torch.isfinite(got).all(), f"{what}: {int((~torch.isfinite(got)).sum())} outputs not written or not finite"
    want = ref + (res.double() if res is not None else 0)
    err = (got.double() - want).abs()
    if mode == "int" and act == ACT_NONE:
        bad = err != 0
        assert not bad.any(), f"{what}: {int(bad.sum())} of {err.numel()} differ from the exact integer result, max {float(err.max())}"
        return
    resabs = res.double().abs() if res is not None else 0
    if mode == "int":
        bound = 4e-6 * (ref.abs() + resabs) + 1e-6
    else:
        slope = torch.ones(ref.shape[-1], dtype=torch.float64, device=ref.device)  # largest |activation'| per channel
        if act == ACT_SILU:
            slope *= 1.1
        elif act == ACT_SIGMOID:
            slope[sig_from:] = 0.25
        bound = slope * TOL[prec] * absref + (4e-6 * ref.abs() if act != ACT_NONE else 0) + 2.0 ** -23 * (ref.abs() + resabs)
    ratio = float((err / bound.clamp_min(1e-300)).max())
    if mode == "randn":
        WORST[prec] = max(WORST.get(prec, 0.0), ratio)
    assert ratio <= 1.0, f"{what}: worst |err| / bound = {ratio:.3g}"


def bound_rejects(got, wrong_ref, absref, prec):
    return bool(((got.double() - wrong_ref).abs() > TOL[prec] * absref).any())


# ---- the library calls -------------------------------------------------------------------------------------------------

def operands(w, prec, H=0, W=0, stride=1):
    """forward and data-gradient operands of a torch (Cout, Cin, k, k) weight."""
    _, lib = _lib()
    Cout, Cin, k = w.shape[0], w.shape[1], w.shape[-1]
    par = lib.frlw_conv2d_dgrad_parity(k, stride, H, W) if H else 0
    wf = torch.full((lib.frlw_conv_operand_floats(k * k * Cin, Cout, prec),), float("nan"), device="cuda")
    wd = torch.full((lib.frlw_conv_operand_floats(k * k * Cout, Cin, prec),), float("nan"), device="cuda")
    check_rc(lib.frlw_conv_weight_layouts(ptr(w), Cout, Cin, k, par, ptr(wf), ptr(wd), prec, None), "frlw_conv_weight_layouts")
    return wf, wd


def plain(name, shape, pitch):
    """The allocator of run_fwd / run_dgrad / run_wgrad: a NaN-filled float32 tensor at exactly its size.  test_conv_edges_gpu.py
    hands over one that puts every buffer between guard bands (name: for its messages; pitch: floats per row of the buffer)."""
    return torch.full(shape, float("nan"), device="cuda")


def run_fwd(x, w, stride, prec, scratch=True, alloc=plain):
    _, lib = _lib()
    B, H, W_, Cin = x.shape
    Cout, k = w.shape[0], w.shape[-1]
    pad = (k - 1) // 2
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W_ + 2 * pad - k) // stride + 1
    wf, _ = operands(w, prec)
    z = alloc("z", (B, Ho, Wo, Cout), Cout)
    sc = alloc("split-K scratch", (SCRATCH,), (Cout + 31) // 32 * 32) if scratch else None
    torch.cuda.synchronize()
    before = counts()
    check_rc(lib.frlw_conv2d_fwd(ptr(x), B, H, W_, Cin, ptr(wf), Cout, k, stride, ptr(z), ptr(sc), SCRATCH if scratch else 0,
                                 prec, None), "frlw_conv2d_fwd")
    torch.cuda.synchronize()
    return z, forms_moved(before)


def run_dgrad(dz, w, stride, H, W, prec, alloc=plain):
    _, lib = _lib()
    B, Ho, Wo, Cout = dz.shape
    Cin, k = w.shape[1], w.shape[-1]
    _, wd = operands(w, prec, H, W, stride)
    dx = alloc("dx", (B, H, W, Cin), Cin)
    sc = alloc("split-K scratch", (SCRATCH,), (Cin + 31) // 32 * 32)
    torch.cuda.synchronize()
    before = counts()
    check_rc(lib.frlw_conv2d_dgrad(ptr(dz), B, Ho, Wo, Cout, ptr(wd), Cin, k, stride, H, W, ptr(dx), ptr(sc), SCRATCH, prec, None),
             "frlw_conv2d_dgrad")
    torch.cuda.synchronize()
    return dx, forms_moved(before)


def run_wgrad(x, dz, k, stride, prec, scratch_part=1.0, alloc=plain):
    _, lib = _lib()
    B, H, W, Cin = x.shape
    _, Ho, Wo, Cout = dz.shape
    want = lib.frlw_conv2d_wgrad_scratch_floats(B, Ho, Wo, Cin, Cout, k)
    n = int(want * scratch_part)
    sc = alloc("wgrad scratch", (n,), Cout)
    dw = alloc("dw", (Cout, Cin, k, k), Cin * k * k)
    torch.cuda.synchronize()
    before = counts()
    check_rc(lib.frlw_conv2d_wgrad(ptr(x), B, H, W, Cin, ptr(dz), Ho, Wo, Cout, k, stride, ptr(dw), ptr(sc), n, prec, None),
             "frlw_conv2d_wgrad")
    torch.cuda.synchronize()
    return dw, forms_moved(before)


# ---- the table -----------------------------------------------------------------------------------------------------------
# (name, (B, Cin, H, W, Cout, k, stride), {precision: forms}); worked out from the thresholds of launch_conv /
# launch_wgrad_tiles -- the counters are the judge.

FWD = [  # frlw_conv2d_fwd with split-K scratch (no arrival counters: the two-launch reduction)
    ("128x32", (2, 64, 32, 40, 32, 3, 1), {"f32": {"128x32"}, "bf16x3": {"128x32"}}),
    ("128x32 gathered", (2, 20, 32, 40, 32, 3, 1), {"f32": {"128x32", "gathered"}, "bf16x3": {"128x32", "gathered"}}),
    ("128x128 2x2", (2, 64, 256, 320, 128, 1, 1), {"f32": {"128x128_2x2"}, "bf16x3": {"128x128_2x2"}}),  # bf16x3 too: K < 512
    ("128x128 2x2 gathered", (2, 36, 256, 320, 128, 1, 1), {"f32": {"128x128_2x2", "gathered"}, "bf16x3": {"128x128_2x2", "gathered"}}),
    ("64x128 / 4x1", (2, 64, 128, 160, 256, 3, 1), {"f32": {"64x128"}, "bf16x3": {"128x128_4x1"}}),
    ("64x128 / 4x1 gathered", (2, 60, 128, 160, 256, 3, 1), {"f32": {"64x128", "gathered"}, "bf16x3": {"128x128_4x1", "gathered"}}),
    ("64x64 whole", (2, 64, 32, 40, 64, 3, 1), {"f32": {"64x64"}, "bf16x3": {"64x64"}}),
    ("64x64 gathered", (2, 20, 32, 40, 64, 3, 1), {"f32": {"64x64", "gathered"}, "bf16x3": {"64x64", "gathered"}}),
    ("64x64 stride 2", (2, 64, 32, 40, 64, 3, 2), {"f32": {"64x64"}, "bf16x3": {"64x64"}}),
    ("split 8 + vector reduce", (2, 256, 8, 10, 256, 3, 1), {"f32": {"split_vec"}, "bf16x3": {"split_vec"}}),
    ("split 8 gathered", (2, 116, 8, 10, 256, 3, 1), {"f32": {"split_vec", "gathered"}, "bf16x3": {"split_vec", "gathered"}}),
    # 32 k-tiles: too short to split without the in-kernel reduction (min_nk 64 for the two-launch form)
    ("1x1 512 unsplit", (2, 512, 8, 10, 256, 1, 1), {"f32": {"64x64"}, "bf16x3": {"64x64"}}),
]

DGRAD = [  # frlw_conv2d_dgrad with split-K scratch
    # parity classes of 1 / 2 / 2 / 4 taps: K = 512 stays whole, the other three split 8 ways
    ("parity, split", (2, 256, 16, 20, 512, 3, 2), {"f32": {"parity", "64x64", "split_vec"}, "bf16x3": {"parity", "64x64", "split_vec"}}),
    ("parity 128x32", (2, 32, 32, 40, 64, 3, 2), {"f32": {"parity", "128x32"}, "bf16x3": {"parity", "128x32"}}),
    ("parity gathered", (2, 32, 32, 40, 20, 3, 2), {"f32": {"parity", "128x32", "gathered"}}),  # bf16x3 needs Cout % 16 == 0
    ("transposed gather, odd", (2, 24, 15, 13, 28, 3, 2), {"f32": {"128x32", "gathered"}, "bf16x3": {"128x32", "gathered"}}),
    ("stride 1, split", (2, 256, 8, 10, 256, 3, 1), {"f32": {"split_vec"}, "bf16x3": {"split_vec"}}),
]

WGRAD = [  # frlw_conv2d_wgrad: (..., scratch fraction)
    ("wgrad 128x128", (2, 256, 16, 20, 256, 3, 1), 1.0, {"wgrad_128x128"}),
    ("wgrad 128x128, a third of the scratch", (2, 256, 16, 20, 256, 3, 1), 0.34, {"wgrad_128x128", "wgrad_scratch_limited"}),
    ("wgrad 128x32", (2, 64, 32, 40, 32, 3, 1), 1.0, {"wgrad_128x32"}),
    ("wgrad 128x64", (2, 64, 32, 40, 64, 3, 1), 1.0, {"wgrad_128x64"}),
    ("wgrad 128x64 stride 2", (2, 32, 32, 40, 64, 3, 2), 1.0, {"wgrad_128x64"}),
    ("wgrad 64x64 + group sums", (2, 64, 64, 80, 64, 1, 1), 1.0, {"wgrad_64x64", "wgrad_group_sum"}),
    ("wgrad 64x64, a third of the scratch", (2, 64, 64, 80, 64, 1, 1), 0.34, {"wgrad_64x64", "wgrad_scratch_limited"}),
]

TRAIN = [  # frlw_baseconv_train_fwd / _bwd with the arrival counters: (forward forms, backward forms) per precision
    ("train, in-kernel split-K 2", (2, 256, 64, 80, 256, 3, 1),
     {"f32": ({"split_inkernel_stats"}, {"split_inkernel", "wgrad_128x128"}),
      "bf16x3": ({"split_vec"}, {"split_vec", "wgrad_128x128"})}),
    ("train, in-kernel split-K 4", (2, 512, 8, 10, 256, 1, 1),
     {"f32": ({"split_inkernel_stats"}, {"64x64", "wgrad_128x64"}), "bf16x3": ({"split_vec"}, {"64x64", "wgrad_128x64"})}),
    # the parity classes split 4 / 8 / 8 / 8 ways and reduce inside the kernel (row-pitched stores of the last arriver)
    ("train, parity split-K", (2, 256, 16, 20, 512, 3, 2),
     {"f32": ({"split_inkernel_stats"}, {"parity", "split_inkernel", "wgrad_128x128"}),
      "bf16x3": ({"split_vec"}, {"parity", "split_vec", "wgrad_128x128"})}),
    ("train, 128x32 with statistics", (2, 64, 32, 40, 32, 3, 1),
     {"f32": ({"128x32"}, {"64x64", "wgrad_128x32"}), "bf16x3": ({"128x32"}, {"64x64", "wgrad_128x32"})}),
    ("train, gathered", (2, 20, 32, 40, 64, 3, 1),
     {"f32": ({"64x64", "gathered"}, {"128x32", "wgrad_128x64"}), "bf16x3": ({"64x64", "gathered"}, {"128x32", "wgrad_128x64"})}),
]

# detector plans: one convolution (+ a fused upsample); `opt` names the epilogue features
DET = [
    ("det bias + SiLU + residual, in-kernel split-K", (2, 256, 8, 10, 256, 3, 1), dict(act=ACT_SILU, bias=True, res=True, scratch=True),
     {"f32": {"split_inkernel"}, "bf16x3": {"split_vec"}}),
    # Cout 126 (Npad 128): no vector rows -- the scalar k_splitk_reduce, the only way to reach it
    ("det odd Cout, sigmoid from 5, scalar reduce", (2, 256, 8, 10, 126, 3, 1), dict(act=ACT_SIGMOID, sig_from=5, bias=True, scratch=True),
     {"f32": {"split_scalar"}, "bf16x3": {"split_scalar"}}),
    ("det offsets + residual", (2, 64, 16, 20, 64, 3, 1),
     dict(act=ACT_SILU, bias=True, res=True, src_cs=80, src_co=16, dst_cs=96, dst_co=8, dst_gap=64, res_cs=72, res_co=4),
     {"f32": {"64x64"}, "bf16x3": {"64x64"}}),
    ("det offsets, 128x128 2x2 / 4x1", (2, 64, 256, 320, 128, 3, 1), dict(act=ACT_SILU, bias=True, src_cs=72, src_co=8, dst_cs=160, dst_co=16),
     {"f32": {"128x128_2x2"}, "bf16x3": {"128x128_4x1"}}),
    ("det group_n 128", (2, 64, 16, 20, 256, 3, 1), dict(act=ACT_SILU, bias=True, group_n=128),
     {"f32": {"64x64"}, "bf16x3": {"64x64"}}),
    ("det fused upsample", (2, 64, 16, 20, 64, 1, 1), dict(act=ACT_SILU, bias=True, upsample=True),
     {"f32": {"64x64"}, "bf16x3": {"64x64"}}),
    ("det 128x32 sigmoid", (2, 36, 32, 40, 24, 3, 2), dict(act=ACT_SIGMOID, sig_from=4, bias=True),
     {"f32": {"128x32", "gathered"}, "bf16x3": {"128x32", "gathered"}}),
]

HALF = ("half batch", (4, 4096, 256, 256, 32, 1, 1), {"f32": {"half_batch", "128x32"}, "bf16x3": {"half_batch", "128x32"}})


def seed(*key):
    return zlib.crc32(repr(key).encode())


def _ids(table):
    return [c[0] for c in table]


# ---- forward / data gradient / weight gradient ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["int", "randn"])
@pytest.mark.parametrize("case", FWD, ids=_ids(FWD))
def test_conv2d_fwd_forms(case, mode):
    name, (B, Cin, H, W, Cout, k, s), forms = case
    g = torch.Generator(device="cuda").manual_seed(seed(name, mode))
    x, w = gen((B, H, W, Cin), mode, g), gen((Cout, Cin, k, k), mode, g)
    ref, absref = conv_ref(x, w, s), conv_ref(x.abs(), w.abs(), s)
    for pname, fs in forms.items():
        z, moved = run_fwd(x, w, s, PREC[pname], scratch=True)
        assert moved == fs, (pname, moved)
        judge(z, ref, absref, mode, PREC[pname], f"{name} {pname}")


def test_bound_rejects_a_dropped_tap_and_k_tile():
    """Negative control on the reference side: the (b) bound of a correct kernel output against a reference with one tap zeroed,
    or with one 16-wide k-tile (16 input channels of one tap) dropped, fails -- in both arithmetics."""
    g = torch.Generator(device="cuda").manual_seed(5)
    x, w = gen((2, 32, 40, 64), "randn", g), gen((256, 64, 3, 3), "randn", g)
    absref = conv_ref(x.abs(), w.abs(), 1)
    w_tap, w_kt = w.clone(), w.clone()
    w_tap[:, :, 1, 2] = 0
    w_kt[:, 16:32, 0, 0] = 0
    for prec in (0, 1):
        z, _ = run_fwd(x, w, 1, prec)
        judge(z, conv_ref(x, w, 1), absref, "randn", prec, "control")
        assert bound_rejects(z, conv_ref(x, w_tap, 1), absref, prec)
        assert bound_rejects(z, conv_ref(x, w_kt, 1), absref, prec)


@pytest.mark.parametrize("mode", ["int", "randn"])
@pytest.mark.parametrize("case", DGRAD, ids=_ids(DGRAD))
def test_conv2d_dgrad_forms(case, mode):
    name, (B, Cin, H, W, Cout, k, s), forms = case
    pad = (k - 1) // 2
    Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    g = torch.Generator(device="cuda").manual_seed(seed(name, mode))
    dz, w = gen((B, Ho, Wo, Cout), mode, g), gen((Cout, Cin, k, k), mode, g)
    ref, absref = dgrad_ref(dz, w, s, H, W), dgrad_ref(dz.abs(), w.abs(), s, H, W)
    for pname, fs in forms.items():
        dx, moved = run_dgrad(dz, w, s, H, W, PREC[pname])
        assert moved == fs, (pname, moved)
        judge(dx, ref, absref, mode, PREC[pname], f"{name} {pname}")


@pytest.mark.parametrize("mode", ["int", "randn"])
@pytest.mark.parametrize("case", WGRAD, ids=_ids(WGRAD))
def test_conv2d_wgrad_forms(case, mode):
    name, (B, Cin, H, W, Cout, k, s), part, fs = case
    pad = (k - 1) // 2
    Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    g = torch.Generator(device="cuda").manual_seed(seed(name, mode))
    x, dz = gen((B, H, W, Cin), mode, g), gen((B, Ho, Wo, Cout), mode, g)
    shape = (Cout, Cin, k, k)
    ref, absref = wgrad_ref(x, dz, shape, s), wgrad_ref(x.abs(), dz.abs(), shape, s)
    for pname, prec in PREC.items():
        dw, moved = run_wgrad(x, dz, k, s, prec, part)
        assert moved == fs, (pname, moved)
        judge(dw, ref, absref, mode, prec, f"{name} {pname}")


# ---- train-mode BaseConv (the only caller besides the detector that hands over arrival counters) ---------------------------

@pytest.mark.parametrize("mode", ["int", "randn"])
@pytest.mark.parametrize("case", TRAIN, ids=_ids(TRAIN))
def test_baseconv_train_forms(case, mode):
    L, lib = _lib()
    name, (B, Cin, H, W, Cout, k, s), forms = case
    pad = (k - 1) // 2
    Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    g = torch.Generator(device="cuda").manual_seed(seed(name, mode))
    x, w = gen((B, H, W, Cin), mode, g), gen((Cout, Cin, k, k), mode, g)
    gamma = torch.rand(Cout, generator=g, device="cuda") + 0.5
    beta = torch.randn(Cout, generator=g, device="cuda") * 0.2
    dy = torch.randn(B, Ho, Wo, Cout, generator=g, device="cuda")
    ref, absref = conv_ref(x, w, s), conv_ref(x.abs(), w.abs(), s)
    # per channel: mean and biased variance of z, and their bounds (|d mean| <= tol E A; |d var| <= 2 tol (E A^2 + (E A)^2))
    mean_ref, var_ref = ref.mean((0, 1, 2)), ref.var((0, 1, 2), unbiased=False)
    a1, a2 = absref.mean((0, 1, 2)), (absref * absref).mean((0, 1, 2))
    nbytes = lib.frlw_baseconv_train_scratch_bytes(B, H, W, Cin, Cout, k, s)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(1024, dtype=torch.int32, device="cuda")
    for pname, (ffs, bfs) in forms.items():
        prec = PREC[pname]
        nan = lambda *sh: torch.full(sh, float("nan"), device="cuda")
        z, y = nan(B, Ho, Wo, Cout), nan(B, Ho, Wo, Cout)
        mean, var, invstd = nan(Cout), nan(Cout), nan(Cout)
        torch.cuda.synchronize()
        before = counts()
        check_rc(lib.frlw_baseconv_train_fwd(ptr(x), ptr(w), ptr(gamma), ptr(beta), C.c_float(1e-5), B, H, W, Cin, Cout, k, s,
                                             ptr(z), ptr(y), ptr(mean), ptr(var), ptr(invstd), None, None, C.c_float(0.1), None,
                                             None, ptr(scratch), nbytes, ptr(cnt), None, prec, None), "train_fwd")
        torch.cuda.synchronize()
        assert forms_moved(before) == ffs, (pname, "forward", forms_moved(before))
        assert int(cnt.abs().sum()) == 0, "arrival counters not reset"
        judge(z, ref, absref, mode, prec, f"{name} {pname} z")
        tol = TOL[prec]
        assert ((mean.double() - mean_ref).abs() <= tol * a1 + 2.0 ** -23 * mean_ref.abs()).all(), f"{name} {pname} mean"
        assert ((var.double() - var_ref).abs() <= 2 * tol * (a2 + a1 * a1) + 2.0 ** -23 * var_ref).all(), f"{name} {pname} var"
        dz, dx, dw = nan(B, Ho, Wo, Cout), nan(B, H, W, Cin), nan(Cout, Cin, k, k)
        dgamma, dbeta = nan(Cout), nan(Cout)
        before = counts()
        check_rc(lib.frlw_baseconv_train_bwd(ptr(dy), 0, ptr(x), ptr(z), ptr(w), ptr(gamma), ptr(beta), ptr(mean), ptr(invstd),
                                             B, H, W, Cin, Cout, k, s, ptr(dz), ptr(dx), ptr(dw), ptr(dgamma), ptr(dbeta), None,
                                             ptr(scratch), nbytes, ptr(cnt), None, prec, None), "train_bwd")
        torch.cuda.synchronize()
        assert forms_moved(before) == bfs, (pname, "backward", forms_moved(before))
        assert int(cnt.abs().sum()) == 0, "arrival counters not reset"
        assert torch.isfinite(dz).all()
        # BatchNorm + SiLU per channel against float64 on the z the forward returned: statistics (var relative to itself), y, and
        # the backward's dz, dgamma, dbeta (bounds: test_bn_silu_forms_gpu.py)
        import test_bn_silu_forms_gpu as bnf
        bn_ref = bnf.reference(z.reshape(-1, Cout), gamma, beta, dy.reshape(-1, Cout))
        bnf.assert_ok(bnf.judge(bn_ref, dict(mean=mean, var=var, invstd=invstd, y=y.reshape(-1, Cout), dz=dz.reshape(-1, Cout), dgamma=dgamma,
                                         dbeta=dbeta)), f"{name} {pname} BatchNorm + SiLU")
        # the data and weight gradients of the dz the BatchNorm backward produced: (b) in both data modes
        judge(dx, dgrad_ref(dz, w, s, H, W), dgrad_ref(dz.abs(), w.abs(), s, H, W), "randn", prec, f"{name} {pname} dx")
        judge(dw, wgrad_ref(x, dz, w.shape, s), wgrad_ref(x.abs(), dz.abs(), w.shape, s), "randn", prec, f"{name} {pname} dw")


PAIR = [  # (name, H, W, stride, precisions); the parity-grouped operand in the bf16x3 arithmetic needs Cout % 16 == 0
    ("stride 1", 8, 8, 1, ("f32", "bf16x3")),
    ("stride 2, transposed gather", 9, 9, 2, ("f32", "bf16x3")),
    ("stride 2, parity classes", 8, 8, 2, ("f32",)),
]


@pytest.mark.parametrize("case", PAIR, ids=_ids(PAIR))
def test_baseconv_train_stacked_pair_without_operand_cache(case):
    """Two blocks stacked along the output channels (frlw_baseconv_fuse_t::split) with no w_cache in either direction: the forward
    lays the stacked forward operand out in its scratch, the backward the stacked data-gradient operand (k_weight_layouts reading
    two weights, parity-grouped in the third case).  z, dx and dw by (b) against float64 on the concatenated weight, BatchNorm +
    SiLU per channel on the concatenated rows."""
    import test_bn_silu_forms_gpu as bnf
    L, lib = _lib()
    name, H, W, s, precs = case
    B, Cin, c1, Cout, k = 2, 8, 16, 36, 3
    Ho, Wo = (H + 2 - k) // s + 1, (W + 2 - k) // s + 1
    g = torch.Generator(device="cuda").manual_seed(seed(name, "pair"))
    x, w = gen((B, H, W, Cin), "randn", g), gen((Cout, Cin, k, k), "randn", g)
    gamma = torch.rand(Cout, generator=g, device="cuda") + 0.5
    beta = torch.randn(Cout, generator=g, device="cuda") * 0.2
    dy = torch.randn(B, Ho, Wo, Cout, generator=g, device="cuda")
    first = [t[:c1].contiguous() for t in (w, gamma, beta)]
    second = [t[c1:].contiguous() for t in (w, gamma, beta)]
    dy1, dy2 = dy[..., :c1].contiguous(), dy[..., c1:].contiguous()
    ref, absref = conv_ref(x, w, s), conv_ref(x.abs(), w.abs(), s)
    nbytes = lib.frlw_baseconv_train_scratch_bytes(B, H, W, Cin, Cout, k, s)
    cnt = torch.zeros(1024, dtype=torch.int32, device="cuda")
    for pname in precs:
        prec = PREC[pname]
        nan = lambda *sh: torch.full(sh, float("nan"), device="cuda")
        scratch = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")  # NaN wherever a float is read unwritten
        z, y1, y2 = nan(B, Ho, Wo, Cout), nan(B, Ho, Wo, c1), nan(B, Ho, Wo, Cout - c1)
        mean, var, invstd = nan(Cout), nan(Cout), nan(Cout)
        fuse = L.FrlwBaseconvFuse(split=c1, w2=second[0].data_ptr(), gamma2=second[1].data_ptr(), beta2=second[2].data_ptr(),
                                  y2=y2.data_ptr(), dy2=dy2.data_ptr())
        check_rc(lib.frlw_baseconv_train_fwd(ptr(x), ptr(first[0]), ptr(first[1]), ptr(first[2]), C.c_float(1e-5), B, H, W, Cin, Cout, k, s,
                                             ptr(z), ptr(y1), ptr(mean), ptr(var), ptr(invstd), None, None, C.c_float(0.1), None,
                                             None, ptr(scratch), nbytes, ptr(cnt), C.byref(fuse), prec, None), "train_fwd")
        judge(z, ref, absref, "randn", prec, f"{name} {pname} z")
        dz, dx, dw = nan(B, Ho, Wo, Cout), nan(B, H, W, Cin), nan(Cout, Cin, k, k)
        dgamma, dbeta = nan(Cout), nan(Cout)
        check_rc(lib.frlw_baseconv_train_bwd(ptr(dy1), 0, ptr(x), ptr(z), ptr(first[0]), ptr(first[1]), ptr(first[2]), ptr(mean), ptr(invstd),
                                             B, H, W, Cin, Cout, k, s, ptr(dz), ptr(dx), ptr(dw), ptr(dgamma), ptr(dbeta), None,
                                             ptr(scratch), nbytes, ptr(cnt), C.byref(fuse), prec, None), "train_bwd")
        torch.cuda.synchronize()
        assert int(cnt.abs().sum()) == 0, "arrival counters not reset"
        bn_ref = bnf.reference(z.reshape(-1, Cout), gamma, beta, dy.reshape(-1, Cout))
        bnf.assert_ok(bnf.judge(bn_ref, dict(mean=mean, var=var, invstd=invstd, y=torch.cat([y1, y2], -1).reshape(-1, Cout),
                                             dz=dz.reshape(-1, Cout), dgamma=dgamma, dbeta=dbeta)), f"{name} {pname} BatchNorm + SiLU")
        judge(dx, dgrad_ref(dz, w, s, H, W), dgrad_ref(dz.abs(), w.abs(), s, H, W), "randn", prec, f"{name} {pname} dx")
        judge(dw, wgrad_ref(x, dz, w.shape, s), wgrad_ref(x.abs(), dz.abs(), w.shape, s), "randn", prec, f"{name} {pname} dw")


# ---- detector plans --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["int", "randn"])
@pytest.mark.parametrize("case", DET, ids=_ids(DET))
def test_detector_conv_epilogues(case, mode):
    L, lib = _lib()
    name, (B, Cin, H, W, Cout, k, s), opt, forms = case
    act, sig_from, gn = opt.get("act", ACT_NONE), opt.get("sig_from", 0), opt.get("group_n", 0)
    groups = 2 if gn else 1
    src_cs, src_co = opt.get("src_cs", Cin * groups), opt.get("src_co", 0)
    Npad = (Cout + 31) // 32 * 32
    pad = (k - 1) // 2
    Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    dst_cs, dst_co = opt.get("dst_cs", Cout), opt.get("dst_co", 0)
    dst_bs = Ho * Wo * dst_cs + opt.get("dst_gap", 0)
    g = torch.Generator(device="cuda").manual_seed(seed(name, mode))
    K = k * k * Cin
    xb = gen((B, H, W, src_cs), mode, g)
    w = gen((Cout, Cin, k, k), mode, g, sparse_k=K if act != ACT_NONE else 0)
    bias = (torch.randint(-2, 3, (Cout,), generator=g, device="cuda").float() if mode == "int"
            else torch.randn(Cout, generator=g, device="cuda")) if opt.get("bias") else None
    res_cs, res_co = opt.get("res_cs", Cout), opt.get("res_co", 0)
    resb = gen((B, Ho, Wo, res_cs), mode, g) if opt.get("res") else None
    # float64 reference: per group, the Cin input channels at src_co + g Cin and the output columns [g gn, (g + 1) gn)
    pre, apre = [], []
    for gi in range(groups):
        xs = xb[..., src_co + gi * Cin: src_co + (gi + 1) * Cin]
        ws = w[gi * gn:(gi + 1) * gn] if gn else w
        pre.append(conv_ref(xs, ws, s))
        apre.append(conv_ref(xs.abs(), ws.abs(), s))
    pre, apre = torch.cat(pre, -1), torch.cat(apre, -1)
    if bias is not None:
        pre, apre = pre + bias.double(), apre + bias.double().abs()
    ref = act_ref(pre, act, sig_from)
    res = resb[..., res_co:res_co + Cout] if resb is not None else None
    # GEMM operand (K, Npad): row (ky k + kx) Cin + ci
    wop = torch.zeros(K, Npad, device="cuda")
    wop[:, :Cout] = w.permute(2, 3, 1, 0).reshape(K, Cout)
    for pname, fs in forms.items():
        prec = PREC[pname]
        if prec == 1:
            wdev = torch.empty(lib.frlw_conv_split_operand_bytes(K, Npad) // 4, device="cuda")
            check_rc(lib.frlw_conv_split_operand(ptr(wop), K, Npad, ptr(wdev), None), "frlw_conv_split_operand")
        else:
            wdev = wop
        yb = torch.full((B * dst_bs,), float("nan"), device="cuda")
        bufs = [xb, yb]
        res_idx = -1
        if resb is not None:
            res_idx = len(bufs)
            bufs.append(resb)
        up_idx = sc_idx = -1
        if opt.get("upsample"):
            up_idx = len(bufs)
            bufs.append(torch.full((B, 2 * Ho, 2 * Wo, Cout + 32), float("nan"), device="cuda"))
        if opt.get("scratch"):
            sc_idx = len(bufs)
            bufs.append(torch.zeros(SCRATCH + 1024, device="cuda"))
        d = lib.frlw_det_create()
        try:
            check_rc(lib.frlw_det_set_precision(d, prec), "set_precision")
            if sc_idx >= 0:
                check_rc(lib.frlw_det_set_scratch(d, sc_idx, SCRATCH + 1024), "set_scratch")
            check_rc(lib.frlw_det_add_conv(d, 0, src_cs, src_co, Cin, H, W, ptr(wdev), ptr(bias), Cout, Npad, k, s, 1, dst_cs, dst_co,
                                           dst_bs, res_idx, res_cs, res_co, act, sig_from, gn), "add_conv")
            if up_idx >= 0:
                check_rc(lib.frlw_det_add_upsample(d, 1, dst_cs, dst_co, Cout, Ho, Wo, up_idx, Cout + 32, 32), "add_upsample")
                assert lib.frlw_det_num_ops(d) == 1  # fused into the convolution's epilogue
            arr = (C.c_void_p * len(bufs))(*[t.data_ptr() for t in bufs])
            torch.cuda.synchronize()
            before = counts()
            check_rc(lib.frlw_det_run(d, B, arr, len(bufs), 0, -1, None), "frlw_det_run")
            torch.cuda.synchronize()
        finally:
            lib.frlw_det_destroy(d)
        assert forms_moved(before) == fs, (pname, forms_moved(before))
        if sc_idx >= 0:
            assert int(bufs[sc_idx][SCRATCH:].abs().sum()) == 0, "arrival counters not reset"
        img = yb.view(B, dst_bs)
        y = img[:, :Ho * Wo * dst_cs].view(B, Ho, Wo, dst_cs)
        judge(y[..., dst_co:dst_co + Cout], ref, apre, mode, prec, f"{name} {pname}", act, res, sig_from)
        outside = torch.ones_like(img, dtype=torch.bool)
        outside[:, :Ho * Wo * dst_cs].view(B, Ho, Wo, dst_cs)[..., dst_co:dst_co + Cout] = False
        assert torch.isnan(img[outside]).all(), f"{name} {pname}: stores outside the destination slice"
        if up_idx >= 0:
            up = bufs[up_idx]
            want = y[..., dst_co:dst_co + Cout].repeat_interleave(2, 1).repeat_interleave(2, 2)
            assert torch.equal(up[..., 32:], want)
            assert torch.isnan(up[..., :32]).all()


# ---- the half-batch split of launch_conv (views beyond the 32-bit buffer offsets) -----------------------------------------

def _rows_ref(x2d, w2d, rows):
    ref, absref = [], []
    for i in range(0, rows.numel(), 16384):
        r = x2d[rows[i:i + 16384]].double()
        ref.append(r @ w2d.double())
        absref.append(r.abs() @ w2d.double().abs())
    return torch.cat(ref), torch.cat(absref)


def test_half_batch_split():
    """4 x 4.3 GB / 4 of input: launch_conv runs the batch as two halves of two images.  The images on both sides of the cut
    (b = 1, 2) in full and a random sample of rows of all four against float64; one image of 4.3 GB is FRLW_ERR_UNSUPPORTED."""
    L, lib = _lib()
    name, (B, Cin, H, W, Cout, k, s), forms = HALF
    g = torch.Generator(device="cuda").manual_seed(11)
    try:
        x = torch.empty(B, H, W, Cin, device="cuda")
        x2d = x.view(-1, Cin)
        hw = H * W
        pick = torch.cat([torch.arange(hw, 3 * hw, device="cuda"),
                          torch.randint(0, B * hw, (8192,), generator=g, device="cuda")])
        for mode in ("int", "randn"):
            for b in range(B):  # (image by image: no temporary of the whole input)
                x[b] = gen((H, W, Cin), mode, g)
            w = gen((Cout, Cin, 1, 1), mode, g)
            ref, absref = _rows_ref(x2d, w.view(Cout, Cin).t(), pick)
            for pname, fs in forms.items():
                z, moved = run_fwd(x, w, 1, PREC[pname], scratch=False)
                assert moved == fs, (pname, moved)
                judge(z.view(-1, Cout)[pick], ref, absref, mode, PREC[pname], f"{name} {mode} {pname}")
                del z
        del x, x2d
        torch.cuda.empty_cache()
        # one image beyond the 32-bit offsets: nothing to split, nothing launched
        x1 = torch.zeros(1, 512, 512, 4096, device="cuda")
        w1 = torch.zeros(32, 4096, 1, 1, device="cuda")
        wf, _ = operands(w1, 0)
        z1 = torch.full((1, 512, 512, 32), float("nan"), device="cuda")
        torch.cuda.synchronize()
        before = counts()
        assert lib.frlw_conv2d_fwd(ptr(x1), 1, 512, 512, 4096, ptr(wf), 32, 1, 1, ptr(z1), None, 0, 0, None) == L.FRLW_ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert forms_moved(before) == set()
        assert torch.isnan(z1).all()
    finally:
        x = x2d = x1 = None
        torch.cuda.empty_cache()


# ---- coverage of the table -------------------------------------------------------------------------------------------------

def test_every_form_has_a_case():
    """Every FRLW_CONV_PATH_* counter is the expected result of at least one case above: a form added without a case fails."""
    L, _ = _lib()
    reached = set()
    for table in (FWD, DGRAD, DET):
        for c in table:
            for fs in c[-1].values():
                reached |= fs
    for c in WGRAD:
        reached |= c[-1]
    for c in TRAIN:
        for f, b in c[-1].values():
            reached |= f | b
    for fs in HALF[-1].values():
        reached |= fs
    assert reached <= set(L.CONV_PATHS), reached - set(L.CONV_PATHS)
    assert set(L.CONV_PATHS) <= reached, set(L.CONV_PATHS) - reached
    if WORST:
        print("worst |err| / bound:", {p: round(v, 4) for p, v in WORST.items()})
