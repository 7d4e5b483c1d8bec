"""The stand-alone kernels of csrc/elementwise.hip at the values and sizes production never sends them.

    frlw_quantize_u8          against u8_rule (tests/leaky_cases.py), equal bytes, clip255 0 and 1
    frlw_leaky_transform      float32 only, uint8 only and both: equal to one another, the uint8 = u8_rule of the float32
    frlw_resize_nearest_*     against CPU torch.nn.functional.interpolate(mode="nearest"), bit for bit

Sizes: n = 2 * 524 288 + 3 elements is past the 2 048 blocks x 256 threads grid_for caps the grid at, so the grid-stride loop
takes two full rounds and a partial third; the resize has one case past the cap too.  Every output is prefilled with 0xAA and
has a guard band behind it that must survive.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import leaky_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu

N_BIG = 2 * 524288 + 3
GUARD = 64  # bytes


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from frlw_evd_amd import _lib
    return _lib.load()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class Guarded:
    """A device buffer of ``n`` elements filled with 0xAA bytes, ``GUARD`` more bytes of the same behind it."""

    def __init__(self, n, dtype):
        self.n, self.item = n, torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full((n * self.item + GUARD,), 0xAA, dtype=torch.uint8, device="cuda")
        self.t = self.raw[:n * self.item].view(dtype)

    def result(self):
        """The payload on the host; the guard must be as it was."""
        torch.cuda.synchronize()
        assert bool((self.raw[self.n * self.item:] == 0xAA).all()), "write behind the output"
        return self.t.cpu().numpy()

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.raw == 0xAA).all())


def the_list():
    """B, C, D of tests/leaky_cases.py (they do not depend on anyone's thresholds), their float64 levels as floats, and the
    edges of the uint8 and int32 ranges."""
    v = lc.flat(lc.values(None), "BCD")
    with np.errstate(invalid="ignore", divide="ignore"):  # (C holds positive v: log1p of -1 and below)
        levels = lc.level64(-v.astype(np.float64)).astype(np.float32)
    two31 = np.float32(2147483648.0)
    extra = np.array([-1.5, -0.999, 255.0, np.nextafter(np.float32(256), np.float32(0)), 256.0, 300.7, 1e9,
                      two31, np.nextafter(two31, np.float32(0)), np.nextafter(two31, np.float32(np.inf)),
                      -two31, np.nextafter(-two31, np.float32(0)), np.nextafter(-two31, np.float32(-np.inf)),
                      np.inf, -np.inf, np.nan], dtype=np.float32)
    return np.concatenate([v, levels, extra])


LIST_LEN = len(the_list())


@pytest.fixture(scope="module")
def big():
    """The list tiled to N_BIG elements, on the host and on the device."""
    v = np.resize(the_list(), N_BIG)
    return v, torch.from_numpy(v).cuda()


# ---- frlw_quantize_u8 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip255", [0, 1])
def test_quantize_u8_is_the_documented_conversion(lib, big, clip255):
    from frlw_evd_amd import _lib
    v, d = big
    out = Guarded(N_BIG, torch.uint8)
    _lib.check(lib.frlw_quantize_u8(ptr(d), N_BIG, clip255, ptr(out.t), stream()), "frlw_quantize_u8")
    with np.errstate(invalid="ignore"):
        want = lc.u8_rule(np.where(v > np.float32(255), np.float32(255), v) if clip255 else v)
    got = out.result()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:5], v[bad[:5]], got[bad[:5]], want[bad[:5]])


def test_quantize_u8_refusals(lib, big):
    from frlw_evd_amd import _lib
    _, d = big
    out = Guarded(16, torch.uint8)
    assert lib.frlw_quantize_u8(None, 16, 0, ptr(out.t), stream()) == _lib.FRLW_ERR_ARG
    assert lib.frlw_quantize_u8(ptr(d), 16, 0, None, stream()) == _lib.FRLW_ERR_ARG
    assert lib.frlw_quantize_u8(ptr(d), -1, 0, ptr(out.t), stream()) == _lib.FRLW_ERR_ARG
    assert lib.frlw_quantize_u8(ptr(d), 0, 0, ptr(out.t), stream()) == _lib.FRLW_OK
    assert out.untouched()


# ---- frlw_leaky_transform ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, N_BIG])
def test_leaky_transform_outputs_agree(lib, big, n):
    from frlw_evd_amd import _lib
    v, d = big
    src = d[LIST_LEN - n:LIST_LEN] if n < N_BIG else d  # (the short runs: the end of the list's first copy, NaN last)
    runs = {}
    for what, (wf, wu) in {"f32": (True, False), "u8": (False, True), "both": (True, True)}.items():
        f, u = Guarded(n, torch.float32), Guarded(n, torch.uint8)
        _lib.check(lib.frlw_leaky_transform(ptr(src), n, ptr(f.t) if wf else None, ptr(u.t) if wu else None, stream()), what)
        if not wf:
            assert f.untouched(), "the float32 output was not asked for"
        if not wu:
            assert u.untouched(), "the uint8 output was not asked for"
        runs[what] = (f.result().view(np.uint32) if wf else None, u.result() if wu else None)
    assert np.array_equal(runs["f32"][0], runs["both"][0])  # as bits: NaN included
    assert np.array_equal(runs["u8"][1], runs["both"][1])
    assert np.array_equal(runs["both"][1], lc.u8_rule(runs["both"][0].view(np.float32)))
    # not a constant: the tail of the list holds v = 0 (255) as well as v > 1 (NaN: 0)
    if n > 1:
        assert runs["u8"][1].min() == 0 and runs["u8"][1].max() == 255


def test_leaky_transform_refusals(lib, big):
    from frlw_evd_amd import _lib
    _, d = big
    f, u = Guarded(16, torch.float32), Guarded(16, torch.uint8)
    assert lib.frlw_leaky_transform(None, 16, ptr(f.t), ptr(u.t), stream()) == _lib.FRLW_ERR_ARG
    assert lib.frlw_leaky_transform(ptr(d), 16, None, None, stream()) == _lib.FRLW_ERR_ARG
    assert lib.frlw_leaky_transform(ptr(d), -1, ptr(f.t), ptr(u.t), stream()) == _lib.FRLW_ERR_ARG
    assert lib.frlw_leaky_transform(ptr(d), 0, ptr(f.t), ptr(u.t), stream()) == _lib.FRLW_OK
    assert f.untouched() and u.untouched()


# ---- frlw_resize_nearest_f32 / _u8 ------------------------------------------------------------------------------------------
PAIRS = [(1, 1, 5, 7), (5, 7, 1, 1), (3, 7, 7, 3), (29, 87, 87, 29), (100, 33, 33, 100), (5, 5, 7, 7), (7, 7, 5, 5), (13, 1, 2, 9),
         (255, 257, 256, 256), (49, 58, 7, 29), (6, 6, 6, 6), (240, 304, 256, 320)]
CASES = [(c,) + p for p in PAIRS for c in (1, 3)] + [(3, 23, 58, 512, 400)]  # the last: 614 400 outputs, past the grid cap


def resize_input(Cn, H, W, dtype):
    rng = np.random.default_rng(Cn * 1000003 + H * 1009 + W)
    if dtype == np.uint8:
        return rng.integers(0, 256, size=(Cn, H, W), dtype=np.uint8)
    a = rng.standard_normal((Cn, H, W)).astype(np.float32)
    flat = a.reshape(-1)
    flat[::7] = np.float32(-0.0)
    flat[::11] = lc.bits_f32(np.array([0x7FC12345], np.uint32))[0]  # a NaN with a payload
    flat[0] = lc.bits_f32(np.array([0xFFC54321], np.uint32))[0]
    return a


@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
@pytest.mark.parametrize("Cn,H,W,Ho,Wo", CASES)
def test_resize_nearest_equals_cpu_torch(lib, Cn, H, W, Ho, Wo, dtype):
    from frlw_evd_amd import _lib
    a = resize_input(Cn, H, W, dtype)
    want = torch.nn.functional.interpolate(torch.from_numpy(a)[None], size=(Ho, Wo), mode="nearest")[0].numpy()
    out = Guarded(Cn * Ho * Wo, torch.float32 if dtype == np.float32 else torch.uint8)
    fn = lib.frlw_resize_nearest_f32 if dtype == np.float32 else lib.frlw_resize_nearest_u8
    _lib.check(fn(ptr(torch.from_numpy(a).cuda()), Cn, H, W, Ho, Wo, ptr(out.t), stream()), "resize_nearest")
    got = out.result().reshape(Cn, Ho, Wo)
    view = np.uint32 if dtype == np.float32 else np.uint8
    bad = np.argwhere(got.view(view) != np.ascontiguousarray(want).view(view))
    assert bad.size == 0, (len(bad), bad[:5])
    if dtype == np.float32 and a.size >= 12 and Ho >= H and Wo >= W:  # (an up-scale samples every source pixel)
        assert np.isnan(got).any() and (got.view(np.uint32) == 0x80000000).any()


def test_resize_nearest_refusals(lib):
    from frlw_evd_amd import _lib
    a = torch.zeros((1, 4, 4), device="cuda")
    out = Guarded(16, torch.float32)
    assert lib.frlw_resize_nearest_f32(None, 1, 4, 4, 4, 4, ptr(out.t), stream()) == _lib.FRLW_ERR_ARG
    assert lib.frlw_resize_nearest_f32(ptr(a), 1, 4, 4, 4, 4, None, stream()) == _lib.FRLW_ERR_ARG
    for bad in [(0, 4, 4, 4, 4), (1, 0, 4, 4, 4), (1, 4, 0, 4, 4), (1, 4, 4, 0, 4), (1, 4, 4, 4, 0)]:
        assert lib.frlw_resize_nearest_f32(ptr(a), *bad, ptr(out.t), stream()) == _lib.FRLW_ERR_ARG
        assert lib.frlw_resize_nearest_u8(ptr(a), *bad, ptr(out.t), stream()) == _lib.FRLW_ERR_ARG
    assert out.untouched()
