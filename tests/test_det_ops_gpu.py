"""Plan ops that the recipes never run on their own, driven through the C ABI: OP_UPSAMPLE as its own launch (the recipes always
fuse it into the convolution before it) and the merged prediction levels across a cut of the op range."""
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
