"""Every non-convolution op of the detector plan on its own, driven through the C ABI on plans of one or a few ops so that the
raw output is visible: OP_UPSAMPLE as its own launch (the recipes always fuse it into the convolution before it), k_focus,
k_spp_pool, k_bfm_stem<2|4|8> and k_pred_infer<1|2> with the merging of prediction levels.  Every destination is filled with a
sentinel or NaN first (with guard words around it); every element the op owes must be written, every other one must keep its fill.

k_focus and k_spp_pool move or compare numbers, so they must equal torch bit for bit.  The shapes are chosen by what launch_focus /
launch_spp_pool make of them (restated below as focus_launch / spp_lds and asserted, so a retune that moves a shape off its branch
fails here): the halving of Wp, an odd W / 2, the clamped tail of the eight-deep load loop, the refusal above 150 KB; pools on maps
smaller than the window, a partial 32-channel group, a pixel stride above 4 C, the 512-pixel limit with 135 168 bytes of LDS.  The
SPP input is negative everywhere, so zero padding in place of -inf padding fails along the whole border.

k_bfm_stem and k_pred_infer are judged twice against float64 restatements written here:
  (a) integer data, where every float32 sum is exact: bit for bit (the sigmoid rows of the predictions: 4e-6, the hardware exp and
      reciprocal, as in test_conv_forms_gpu.py).  A mis-indexed weight, group, carried channel, quadrant, lane or level is an
      integer-sized error.
  (b) real data.  BFM: the Temporal_Active_Focus_connect module with randn weight_g / weight_v / biases, packed as
      DetectorEngine._bfm_front packs it; the restatement equals module.double().mix(x) to 1e-12, and the kernel may be off by at
      most BFM_TOL = min(8 e32, 1e-5) of max |float64|, e32 being the error of the float32 torch forward of the same module on the
      device.  Measured on an MI355X: e32 = 1.58e-7 (C = 4, 8, 16: 1.58e-7, 1.15e-7, 8.9e-8), so BFM_TOL = 8 e32 = 1.26e-6; the
      kernel: 1.0e-7, 2.6e-7, 1.4e-7.
      Predictions: judge() of test_conv_forms_gpu.py, |got - ref| <= 1e-5 (|x| . |w| + |b|) element by element, plus 4e-6 for the
      sigmoid rows.  Worst |err| / bound observed on an MI355X: 0.017.
Negative controls, on the reference side only: two quadrants of the BFM reference swapped, the SPP reference padded with 0, one
float4 chunk of the prediction's dot product dropped, BL and TR of the Focus reference swapped -- each is rejected by the same
comparison that the kernel passes."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from frlw_evd_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


def _run(lib, det, B, tensors, first, last):
    ptrs = (C.c_void_p * len(tensors))(*[C.c_void_p(t.data_ptr()) for t in tensors])
    _lib.check(lib.frlw_det_run(det, B, ptrs, len(tensors), first, last, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "run")
    torch.cuda.synchronize()


def test_upsample_as_its_own_launch(gpu):
    """k_upsample2x: C = 6 is no multiple of 4, so the op can never fuse.  Slice to slice, bit for bit against
    torch.nn.functional.interpolate(nearest); every other channel of the destination keeps its sentinel."""
    lib = _lib.load()
    B, H, W, Cc, cs_src, co_src, cs_dst, co_dst = 2, 3, 5, 6, 12, 4, 10, 2
    src = torch.randn(B, H, W, cs_src, device=gpu)
    dst = torch.full((B, 2 * H, 2 * W, cs_dst), 12345.0, device=gpu)
    det = lib.frlw_det_create()
    try:
        assert lib.frlw_det_add_upsample(det, 0, cs_src, co_src, Cc, H, W, 1, cs_dst, co_dst) == _lib.FRLW_OK
        assert lib.frlw_det_num_ops(det) == 1
        _run(lib, det, B, [src, dst], 0, -1)
    finally:
        lib.frlw_det_destroy(det)
    want = torch.nn.functional.interpolate(src[..., co_src:co_src + Cc].permute(0, 3, 1, 2), scale_factor=2, mode="nearest").permute(0, 2, 3, 1)
    assert torch.equal(dst[..., co_dst:co_dst + Cc], want)
    rest = torch.cat([dst[..., :co_dst], dst[..., co_dst + Cc:]], dim=-1)
    assert bool((rest == 12345.0).all())


@pytest.mark.parametrize("F", [7, 12])  # k_pred_infer<1> (F <= 8) and k_pred_infer<2>
def test_prediction_levels_across_a_range_cut(gpu, F):
    """Three frlw_det_add_pred ops on one lane (C = 4, hw = 6, 2, 1, B = 2): frlw_det_run merges consecutive levels into one
    launch, but only inside the range it is given.  [0, 3) in one call and [0, 1) + [1, 3) in two give the same bits, and both
    equal a float64 restatement within 1e-5: four-term float32 dot products and the hardware sigmoid (2 ulp)."""
    lib = _lib.load()
    B, Cc, cs, co, hws = 2, 4, 12, 4, (6, 2, 1)
    A = sum(hws)
    rng = np.random.default_rng(1000 + F)
    feats = [torch.from_numpy(rng.standard_normal((B, hw, cs)).astype(np.float32)).to(gpu) for hw in hws]
    ws = [torch.from_numpy(rng.standard_normal((F, Cc)).astype(np.float32)).to(gpu) for _ in hws]
    bs = [torch.from_numpy(rng.standard_normal(F).astype(np.float32)).to(gpu) for _ in hws]
    det = lib.frlw_det_create()
    try:
        off = 0
        for i, hw in enumerate(hws):
            assert lib.frlw_det_add_pred(det, i, cs, co, Cc, hw, C.c_void_p(ws[i].data_ptr()), C.c_void_p(bs[i].data_ptr()), F, 3, off,
                                         A * F) == _lib.FRLW_OK
            off += hw
        assert lib.frlw_det_num_ops(det) == 3
        whole = torch.full((B, A, F), 12345.0, device=gpu)
        cut = torch.full((B, A, F), 12345.0, device=gpu)
        _run(lib, det, B, feats + [whole], 0, 3)
        _run(lib, det, B, feats + [cut], 0, 1)
        _run(lib, det, B, feats + [cut], 1, 3)
    finally:
        lib.frlw_det_destroy(det)
    assert torch.equal(whole, cut)
    want = []
    for f, w, b in zip(feats, ws, bs):
        f, w, b = f.double().cpu(), w.double().cpu(), b.double().cpu()
        reg = f[..., co:co + Cc] @ w[:5].T + b[:5]              # rows 0-4 (reg, obj) read reg_feat
        cls = f[..., co + Cc:co + 2 * Cc] @ w[5:].T + b[5:]     # rows 5.. (cls) read cls_feat
        t = torch.cat([reg, cls], dim=-1)
        t[..., 4:] = torch.sigmoid(t[..., 4:])
        want.append(t)
    want = torch.cat(want, dim=1)
    err = float((whole.double().cpu() - want).abs().max())
    print(f"F = {F}: max abs error against float64 {err:.3e}")
    assert err <= 1e-5


# ---- helpers of the single-op tests ------------------------------------------------------------------------------------------

SENT, GUARD = 12345.0, 64


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _guarded(shape, fill, dev):
    """A destination of `shape` filled with `fill`, with GUARD words of the same fill in front of it and behind it."""
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * GUARD,), fill, device=dev)
    return flat, flat[GUARD:GUARD + n].view(shape)


def _kept(t, fill):
    return bool(torch.isnan(t).all()) if fill != fill else bool((t == fill).all())


def _guards_kept(flat, fill):
    return _kept(flat[:GUARD], fill) and _kept(flat[-GUARD:], fill)


def _plan_run(lib, B, tensors, add, first=0, last=-1):
    """A plan of the ops `add(det)` adds (asserted FRLW_OK there), run once over `tensors`."""
    det = lib.frlw_det_create()
    try:
        n = add(det)
        assert lib.frlw_det_num_ops(det) == n
        _run(lib, det, B, tensors, first, last)
    finally:
        lib.frlw_det_destroy(det)


# ---- k_focus -------------------------------------------------------------------------------------------------------------------

def focus_launch(Cc, W):
    """launch_focus of csrc/det_focus.h: (pixels per workgroup, bytes of LDS)."""
    Wp = W // 2
    while Wp % 2 == 0 and Wp * (4 * Cc + 1) * 4 > 20 * 1024:
        Wp //= 2
    return Wp, Wp * (4 * Cc + 1) * 4


FOCUS = [  # (C, H, W), (Wp, LDS bytes), the branch
    ((1, 2, 2), (1, 20), "smallest shape"),
    ((10, 6, 10), (5, 820), "W / 2 = 5 odd, one part"),
    ((16, 4, 640), (40, 10400), "Wp halves 320 -> 40, eight parts per row"),
    ((3, 4, 2052), (513, 26676), "W / 2 = 1026 -> Wp = 513, n2 = 3078: the second pass of the load loop ends in the clamped tail"),
]
FOCUS_TOO_WIDE = ((64, 2, 302), (151, 155228))  # W / 2 = 151 is odd, so Wp cannot halve: above the 150 KB limit


def _focus_ref(x, swap_bl_tr=False):
    from frlw_evd_amd.yolox.network_blocks import Focus
    want = Focus.space_to_depth(x).permute(0, 2, 3, 1).contiguous()
    if swap_bl_tr:
        Cc = x.shape[1]
        want = torch.cat([want[..., :Cc], want[..., 2 * Cc:3 * Cc], want[..., Cc:2 * Cc], want[..., 3 * Cc:]], dim=-1)
    return want


@pytest.mark.parametrize("shape,launch,why", FOCUS, ids=[str(c[0]) for c in FOCUS])
def test_focus_bit_exact(gpu, shape, launch, why):
    lib = _lib.load()
    Cc, H, W = shape
    assert focus_launch(Cc, W) == launch, why
    Wp, n2 = launch[0], 2 * Cc * launch[0]
    assert (W // 2) % Wp == 0 and launch[1] <= 150 * 1024
    if shape == (3, 4, 2052):
        assert n2 > 2048 and n2 % 2048 != 0
    B = 2
    x = torch.randn(B, Cc, H, W, generator=torch.Generator().manual_seed(Cc * 1000 + W)).to(gpu)
    flat, y = _guarded((B, H // 2, W // 2, 4 * Cc), float("nan"), gpu)
    assert lib.frlw_focus_nhwc(_ptr(x), B, Cc, H, W, _ptr(y), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == _lib.FRLW_OK
    torch.cuda.synchronize()
    assert torch.equal(y, _focus_ref(x))
    assert not torch.equal(y, _focus_ref(x, swap_bl_tr=True))  # negative control
    assert _guards_kept(flat, float("nan"))


def test_focus_as_a_plan_op(gpu):
    lib = _lib.load()
    B, Cc, H, W = 2, 10, 6, 10
    x = torch.randn(B, Cc, H, W, generator=torch.Generator().manual_seed(77)).to(gpu)
    flat, y = _guarded((B, H // 2, W // 2, 4 * Cc), float("nan"), gpu)

    def add(det):
        assert lib.frlw_det_add_focus(det, 0, Cc, H, W, 1) == _lib.FRLW_OK
        return 1
    _plan_run(lib, B, [x, y], add)
    assert torch.equal(y, _focus_ref(x))
    assert _guards_kept(flat, float("nan"))


def test_focus_refuses_a_row_above_150_kb(gpu):
    lib = _lib.load()
    (Cc, H, W), launch = FOCUS_TOO_WIDE
    assert focus_launch(Cc, W) == launch and launch[1] > 150 * 1024
    B = 2
    x = torch.randn(B, Cc, H, W, device=gpu)
    flat, y = _guarded((B, H // 2, W // 2, 4 * Cc), SENT, gpu)
    rc = lib.frlw_focus_nhwc(_ptr(x), B, Cc, H, W, _ptr(y), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == _lib.FRLW_ERR_UNSUPPORTED
    assert _kept(flat, SENT)


# ---- k_spp_pool ----------------------------------------------------------------------------------------------------------------

def spp_lds(H, W):
    """launch_spp_pool of csrc/det_glue.h: two H x W x (32 + 1) float tiles."""
    return 2 * H * W * 33 * 4


SPP = [  # (H, W, C, cs), bytes of LDS, the branch
    ((1, 1, 4, 16), 264, "smallest map: every window is padding but its centre"),
    ((3, 4, 40, 160), 3168, "H and W below 5; the second channel group holds 8 of 32 channels"),
    ((5, 7, 32, 136), 9240, "pixel stride above 4 C: channels [128, 136) are not the op's"),
    ((16, 32, 8, 32), 135168, "512 pixels = kSppMaxPix: the dynamic LDS request above 64 KB"),
]


def _spp_ref(x_nhwc, k, zero_pad=False):
    x = x_nhwc.cpu().permute(0, 3, 1, 2)
    if zero_pad:
        y = torch.nn.functional.max_pool2d(torch.nn.functional.pad(x, (k // 2,) * 4, value=0.0), k, 1, 0)
    else:
        y = torch.nn.MaxPool2d(k, 1, k // 2)(x)
    return y.permute(0, 2, 3, 1)


@pytest.mark.parametrize("shape,lds,why", SPP, ids=[str(c[0]) for c in SPP])
def test_spp_pools_bit_exact(gpu, shape, lds, why):
    lib = _lib.load()
    H, W, Cc, cs = shape
    assert spp_lds(H, W) == lds and H * W <= 512, why
    B = 2
    x = torch.randn(B, H, W, Cc, generator=torch.Generator().manual_seed(H * 100 + W)) - 10.0  # negative everywhere
    x[..., ::4] = (x[..., ::4] * 2).round() / 2  # a quarter of the channels in halves: ties
    assert float(x.max()) < 0
    flat, buf = _guarded((B, H, W, cs), SENT, gpu)
    buf[..., :Cc] = x.to(gpu)

    def add(det):
        assert lib.frlw_det_add_spp_pool(det, 0, cs, Cc, H, W) == _lib.FRLW_OK
        return 1
    _plan_run(lib, B, [buf], add)
    got = buf.cpu()
    assert torch.equal(got[..., :Cc], x)
    for r, k in enumerate((5, 9, 13), start=1):
        assert torch.equal(got[..., r * Cc:(r + 1) * Cc], _spp_ref(x, k)), f"pool {k}"
        assert not torch.equal(got[..., r * Cc:(r + 1) * Cc], _spp_ref(x, k, zero_pad=True)), f"pool {k}: negative control"
    assert _kept(got[..., 4 * Cc:], SENT)
    assert _guards_kept(flat, SENT)


def test_spp_refuses_more_than_512_pixels():
    lib = _lib.load()
    det = lib.frlw_det_create()
    try:
        assert lib.frlw_det_add_spp_pool(det, 0, 32, 8, 17, 31) == _lib.FRLW_ERR_UNSUPPORTED
        assert lib.frlw_det_num_ops(det) == 0
    finally:
        lib.frlw_det_destroy(det)


# ---- k_bfm_stem ----------------------------------------------------------------------------------------------------------------

BFM_TOL = 1.26e-6  # min(8 e32, 1e-5) with the measured e32 = 1.576e-7: see the module docstring
BFM_SHAPES = [(4, 2, 6, 10), (8, 2, 6, 10), (16, 2, 6, 10), (8, 1, 2, 2)]  # (C, B, H, W)


def _bfm_split(packed, Cc):
    """The packed weights det_bfm.h documents -> [(W (n_out, in_g), b) per stage], (W up (4 ER, ER), b), (W down (ER, 4 ER), b)."""
    TC = Cc // 2
    R = TC.bit_length() - 1
    ER, off, stages = 4 * R, 0, []

    def take(*shape):
        nonlocal off
        n = int(np.prod(shape))
        t = packed[off:off + n].reshape(shape)
        off += n
        return t
    for i in range(R):
        n_out, in_g = 2 * (TC >> i), 4 if i == 0 else 8
        stages.append((take(n_out, in_g), take(n_out)))
    up = (take(4 * ER, ER), take(4 * ER))
    down = (take(ER, 4 * ER), take(ER))
    assert off == packed.numel()
    return stages, up, down


def _bfm_mix64(x, packed, Cc):
    """Float64 restatement of the per-pixel part: (B, C, H, W) -> (B, ER, H, W)."""
    F = torch.nn.functional
    stages, up, down = _bfm_split(packed.double(), Cc)
    v, cat = x.double(), []
    for w, b in stages:
        v = F.relu(F.conv2d(v, w[:, :, None, None], b, groups=w.shape[0] // 4))  # four outputs per time-group pair
        cat.append(v[:, :4])
    cat = torch.cat(cat, dim=1)
    h = F.conv2d(cat, up[0][:, :, None, None], up[1])
    h = h * torch.sigmoid(h)
    return cat + F.conv2d(h, down[0][:, :, None, None], down[1])


def _bfm_pack(stem):
    """DetectorEngine._bfm_front's packing, in the module's own dtype."""
    parts = []
    for conv in stem.convs:
        w = torch._weight_norm(conv.weight_v.detach(), conv.weight_g.detach(), 0)
        parts += [w.reshape(w.shape[0], -1).flatten(), conv.bias.detach().flatten()]
    for lin in (stem.trans_up, stem.trans_down):
        parts += [lin.weight.detach().reshape(lin.weight.shape[0], -1).flatten(), lin.bias.detach().flatten()]
    return torch.cat([p.cpu() for p in parts]).contiguous()


def _bfm_run(gpu, x, packed):
    """k_bfm_stem as a plan of one op -> (B, H / 2, W / 2, 4 ER) on the host."""
    lib = _lib.load()
    B, Cc, H, W = x.shape
    ER = 4 * ((Cc // 2).bit_length() - 1)
    assert lib.frlw_det_bfm_weight_count(Cc) == packed.numel()
    xd, wd = x.float().to(gpu), packed.float().to(gpu)
    flat, y = _guarded((B, H // 2, W // 2, 4 * ER), float("nan"), gpu)

    def add(det):
        assert lib.frlw_det_add_bfm_stem(det, 0, Cc, H, W, _ptr(wd), wd.numel(), 1) == _lib.FRLW_OK
        return 1
    _plan_run(lib, B, [xd, y], add)
    assert _guards_kept(flat, float("nan"))
    return y.cpu()


def _focus_layout(t, swap=None):
    """(B, ER, H, W) -> the kernel's output layout (B, H / 2, W / 2, [TL | BL | TR | BR]); swap: two quadrants exchanged."""
    q = [t[..., ::2, ::2], t[..., 1::2, ::2], t[..., ::2, 1::2], t[..., 1::2, 1::2]]
    if swap:
        q[swap[0]], q[swap[1]] = q[swap[1]], q[swap[0]]
    return torch.cat(q, dim=1).permute(0, 2, 3, 1)


@pytest.mark.parametrize("Cc,B,H,W", BFM_SHAPES)
def test_bfm_stem_integer_data_bit_exact(gpu, Cc, B, H, W):
    """(a): x, stage weights and biases in {-2..2}, trans_down all zero: the output is `cat`, at most 8 * 2 * 290 + 2 in size."""
    g = torch.Generator().manual_seed(4000 + Cc + H)
    n = _lib.load().frlw_det_bfm_weight_count(Cc)
    packed = torch.randint(-2, 3, (n,), generator=g).float()
    ER = 4 * ((Cc // 2).bit_length() - 1)
    packed[n - (4 * ER * ER + ER):] = 0.0  # trans_down W and b
    x = torch.randint(-2, 3, (B, Cc, H, W), generator=g).float()
    ref = _bfm_mix64(x, packed, Cc)
    assert float(ref.abs().max()) > 0 and bool((ref == ref.round()).all())
    got = _bfm_run(gpu, x, packed).double()
    assert torch.equal(got, _focus_layout(ref))
    for swap in ((0, 1), (1, 2), (0, 3)):  # negative control: BL for TL, TR for BL, BR for TL
        assert not torch.equal(got, _focus_layout(ref, swap)), swap


def _bfm_module(Cc):
    from frlw_evd_amd.yolox.bfm import Temporal_Active_Focus_connect
    torch.manual_seed(5000 + Cc)
    m = Temporal_Active_Focus_connect(Cc, 32, ksize=3, act="silu").eval()
    with torch.no_grad():
        for conv in m.convs:
            conv.weight_g.normal_()
            conv.weight_v.normal_()
            conv.bias.normal_()
        m.trans_up.bias.normal_()
        m.trans_down.bias.normal_()
    return m


@pytest.fixture(scope="module")
def bfm_real(gpu):
    """Per C: the module's data, the float64 restatement, the float32 torch forward on the device and its error e32."""
    out = {}
    for Cc in (4, 8, 16):
        m, m64 = _bfm_module(Cc), _bfm_module(Cc).double()  # (the same seed: the same parameters)
        x = torch.randn(2, Cc, 6, 10, generator=torch.Generator().manual_seed(6000 + Cc))
        with torch.no_grad():
            ref = _bfm_mix64(x, _bfm_pack(m64), Cc)
            mix64 = m64.mix(x.double())
            mix32 = _bfm_module(Cc).to(gpu).mix(x.to(gpu)).cpu()
            v = x.double()
            for conv in m64.convs:  # outputs on both sides of every ReLU
                pre = conv(v)
                assert float(pre.min()) < 0 < float(pre.max())
                v = torch.relu(pre)
        out[Cc] = dict(m=m, x=x, ref=ref, mix64=mix64, e32=float((mix32.double() - ref).abs().max() / ref.abs().max()))
    return out


@pytest.mark.parametrize("Cc", [4, 8, 16])
def test_bfm_stem_real_data(gpu, bfm_real, Cc):
    """(b): the restatement is the module (1e-12); the kernel is within BFM_TOL of the restatement, relative to max |float64|."""
    d = bfm_real[Cc]
    assert float((d["ref"] - d["mix64"]).abs().max()) <= 1e-12 * max(1.0, float(d["mix64"].abs().max()))
    got = _bfm_run(gpu, d["x"], _bfm_pack(d["m"])).double()
    err = float((got - _focus_layout(d["ref"])).abs().max() / d["ref"].abs().max())
    e32 = max(r["e32"] for r in bfm_real.values())
    print(f"C = {Cc}: kernel {err:.3e}, float32 torch {d['e32']:.3e} of max |float64|; e32 = {e32:.3e}, 8 e32 = {8 * e32:.3e}")
    assert err <= BFM_TOL


# ---- k_pred_infer --------------------------------------------------------------------------------------------------------------

def _pred_gen(shape, mode, g):
    if mode == "int":
        return torch.randint(-3, 4, shape, generator=g).float()
    return torch.randn(shape, generator=g) + 0.5


def _pred_ref(f, w, b, co, Cc, drop_chunk=None):
    """Float64 restatement of one level (that of test_prediction_levels_across_a_range_cut) -> pre-activations, |x| . |w| + |b|.
    drop_chunk: the float4 chunk of both dot products that the negative control leaves out."""
    f, w, b = f.double(), w.double(), b.double()
    if drop_chunk is not None:
        w = w.clone()
        w[:, 4 * drop_chunk:4 * drop_chunk + 4] = 0.0
    reg, cls = f[..., co:co + Cc], f[..., co + Cc:co + 2 * Cc]
    pre = torch.cat([reg @ w[:5].T + b[:5], cls @ w[5:].T + b[5:]], dim=-1)
    absref = torch.cat([reg.abs() @ w[:5].abs().T + b[:5].abs(), cls.abs() @ w[5:].abs().T + b[5:].abs()], dim=-1)
    return pre, absref


def _sig_rows(pre):
    t = pre.clone()
    t[..., 4:] = torch.sigmoid(t[..., 4:])
    return t


PRED_WORST = {}


def _pred_judge(got, pre, absref, mode, what, record=True):
    """(a) / (b) of the module docstring for one level's rows."""
    import test_conv_forms_gpu as forms
    got, ref = got.double(), _sig_rows(pre)
    assert bool(torch.isfinite(got).all()) and not bool((got == SENT).any()), f"{what}: rows not written"
    if mode == "int":
        assert torch.equal(got[..., :4], ref[..., :4]), f"{what}: rows 0-3 differ from the exact integer result"
        err = float((got[..., 4:] - ref[..., 4:]).abs().max())
        assert err <= 4e-6, f"{what}: sigmoid rows off by {err:.3e}"
        return
    saved = dict(forms.WORST)
    forms.WORST.clear()
    try:
        forms.judge(got[..., :4], ref[..., :4], absref[..., :4], "randn", 0, what + " rows 0-3")
        forms.judge(got[..., 4:], ref[..., 4:], absref[..., 4:], "randn", 0, what + " rows 4..", act=forms.ACT_SIGMOID)
        if record:
            PRED_WORST[mode] = max(PRED_WORST.get(mode, 0.0), forms.WORST[0])
    finally:
        forms.WORST.clear()
        forms.WORST.update(saved)


def _pred_rejects(got, wrong_pre, absref, mode):
    """The comparison of _pred_judge refuses a wrong reference."""
    try:
        _pred_judge(got, wrong_pre, absref, mode, "negative control", record=False)
    except AssertionError:
        return True
    return False


class PredPlan:
    """Levels (C, F, hw, cs, co) as consecutive frlw_det_add_pred ops.  Levels of one F share a (B, 1 + A_F + 2, F) head tensor whose
    first anchor and last two belong to nobody; buffers: the levels' features, then one head tensor per distinct F."""

    def __init__(self, gpu, B, levels, mode, seed):
        self.lib, self.gpu, self.B, self.levels, self.mode = _lib.load(), gpu, B, levels, mode
        g = torch.Generator().manual_seed(seed)
        self.f = [_pred_gen((B, hw, cs), mode, g) for (_, _, hw, cs, _) in levels]
        self.w = [_pred_gen((F, Cc), mode, g) for (Cc, F, _, _, _) in levels]
        self.b = [_pred_gen((F,), mode, g) for (_, F, _, _, _) in levels]
        self.dev = [[t.to(gpu) for t in ts] for ts in (self.f, self.w, self.b)]
        self.Fs = sorted({lv[1] for lv in levels})
        self.A = {F: 1 + sum(lv[2] for lv in levels if lv[1] == F) + 2 for F in self.Fs}
        self.first, nxt = [], {F: 1 for F in self.Fs}
        for (_, F, hw, _, _) in levels:
            self.first.append(nxt[F])
            nxt[F] += hw
        self.det = self.lib.frlw_det_create()
        for i, (Cc, F, hw, cs, co) in enumerate(levels):
            rc = self.lib.frlw_det_add_pred(self.det, i, cs, co, Cc, hw, _ptr(self.dev[1][i]), _ptr(self.dev[2][i]), F,
                                            len(levels) + self.Fs.index(F), self.first[i], self.A[F] * F)
            assert rc == _lib.FRLW_OK
        assert self.lib.frlw_det_num_ops(self.det) == len(levels)

    def close(self):
        self.lib.frlw_det_destroy(self.det)

    def run(self, ranges):
        """Fresh sentinel-filled head tensors, the op ranges run in order -> {F: (flat with guards, (B, A_F, F))}."""
        outs = {F: _guarded((self.B, self.A[F], F), SENT, self.gpu) for F in self.Fs}
        for first, last in ranges:
            _run(self.lib, self.det, self.B, self.dev[0] + [outs[F][1] for F in self.Fs], first, last)
        return outs

    def check(self, outs, negative_control=True):
        for F in self.Fs:
            flat, out = outs[F]
            assert _guards_kept(flat, SENT)
            assert _kept(out[:, 0], SENT) and _kept(out[:, -2:], SENT), f"F = {F}: rows outside the levels' anchors written"
        for i, (Cc, F, hw, cs, co) in enumerate(self.levels):
            got = outs[F][1][:, self.first[i]:self.first[i] + hw].cpu()
            pre, absref = _pred_ref(self.f[i], self.w[i], self.b[i], co, Cc)
            _pred_judge(got, pre, absref, self.mode, f"level {i} (C = {Cc}, F = {F}, hw = {hw})")
            if negative_control:  # without the last lane's chunk
                wrong, _ = _pred_ref(self.f[i], self.w[i], self.b[i], co, Cc, drop_chunk=Cc // 4 - 1)
                assert _pred_rejects(got, wrong, absref, self.mode), f"level {i}: a dropped chunk passes"


def _pred_single(gpu, mode, B, Cc, F, hw, cs, co, seed):
    p = PredPlan(gpu, B, [(Cc, F, hw, cs, co)], mode, seed)
    try:
        p.check(p.run([(0, -1)]))
    finally:
        p.close()


@pytest.mark.parametrize("mode", ["int", "randn"])
@pytest.mark.parametrize("Cc,F", [(96, 7), (252, 9), (256, 16)])  # 24 lanes (no power of two), 63, 64; NG = 1, 2, 2 (all 16 rows)
def test_pred_lanes(gpu, Cc, F, mode):
    _pred_single(gpu, mode, 2, Cc, F, 5, 2 * Cc + 8, 4, 7000 + Cc + F)


@pytest.mark.parametrize("mode", ["int", "randn"])
@pytest.mark.parametrize("F", [6, 8, 9, 16])  # the smallest F; NG = 1 full; the first row of the second group; NG = 2 full
def test_pred_row_count_edges(gpu, F, mode):
    _pred_single(gpu, mode, 2, 8, F, 5, 24, 4, 7100 + F)


@pytest.mark.parametrize("mode", ["int", "randn"])
def test_pred_more_rows_than_the_grid_takes(gpu, mode):
    """65 573 rows > 2048 workgroups x 4 wavefronts x 8 rows: the grid is capped at 8192 wavefronts, which stride over eight or nine rows each."""
    hw = 65536 + 37
    assert (hw + 31) // 32 > 2048
    _pred_single(gpu, mode, 1, 4, 6, hw, 16, 4, 7200)


@pytest.mark.parametrize("mode", ["int", "randn"])
@pytest.mark.parametrize("F", [7, 12])
def test_pred_five_levels_and_every_range_cut(gpu, F, mode):
    """Five consecutive levels of one F run as 4 + 1; the run cut at every op boundary gives the same bits as the whole range."""
    hws = (6, 2, 1, 3, 5)
    p = PredPlan(gpu, 2, [(8, F, hw, 24, 4) for hw in hws], mode, 7300 + F)
    try:
        whole = p.run([(0, 5)])
        p.check(whole)
        for k in range(1, 5):
            cut = p.run([(0, k), (k, 5)])
            assert torch.equal(cut[F][0], whole[F][0]), f"cut at {k}"
        single = p.run([(i, i + 1) for i in range(5)])
        assert torch.equal(single[F][0], whole[F][0])
    finally:
        p.close()


@pytest.mark.parametrize("mode", ["int", "randn"])
@pytest.mark.parametrize("F,F2", [(7, 12), (12, 7)])
def test_pred_levels_of_another_row_count_do_not_merge(gpu, F, F2, mode):
    """Levels F, F, F', F: the third must not ride in the launch of the first two (its NG and row stride would be theirs)."""
    p = PredPlan(gpu, 2, [(8, F, 6, 24, 4), (8, F, 2, 24, 4), (8, F2, 3, 24, 4), (8, F, 5, 24, 4)], mode, 7400 + F)
    try:
        p.check(p.run([(0, -1)]))
    finally:
        p.close()


def test_pred_worst_ratio_report():
    if PRED_WORST:
        print("prediction rows, worst |err| / bound:", {k: round(v, 4) for k, v in PRED_WORST.items()})
