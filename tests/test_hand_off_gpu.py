"""frlw_volume_hand_off_u8 / transforms.hand_off: a detector batch from uint8 planes that lie in different tensors, in one launch,
byte-equal to the numpy restatement (tests/hand_off_restated.py) and to the multi-step route it replaces
(``er.resize_nearest`` + ``transforms.transform_images`` with default parameters).

Shapes: resize up with ``W % 4 == 0`` (16-byte stores, byte gathers), equal shapes (one 32-bit word per four outputs), odd sizes
(the scalar path), and equal shapes with samples sliced at an odd plane offset of a buffer that starts one byte behind a 4-byte
boundary (90 * 160 is a multiple of 4, so the misalignment comes from the buffer: the byte loads of the equal-shape path).  In
every case the samples of a batch alternate between two source tensors and start at plane 1 of a sample's planes, so with
odd ``h * w`` the plane addresses are unaligned as well.  ``out`` lies inside a guard band that must keep its sentinel.
"""
import ctypes as C

import numpy as np
import pytest

import hand_off_restated as restated

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD = 4096          # floats on either side of out
SENTINEL = -77.25
BATCHES = (1, 5, 64)
CHANNELS = (2, 8, 10, 16)


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


def make_sources(B, Cn, h, w, seed, device, misalign=0):
    """Two uint8 buffers, each ``misalign`` bytes + (B, Cn + 1, h, w); sample b is planes [1, Cn + 1) of entry b of buffer b % 2.
    Returns (list of B tensor views, list of B numpy arrays of the same bytes)."""
    rng = np.random.default_rng(seed)
    n = B * (Cn + 1) * h * w
    host = [rng.integers(0, 256, misalign + n, dtype=np.uint8) for _ in range(2)]
    host[0][misalign:misalign + 512] = np.arange(512) % 256   # every byte value, 0 and 255 included
    dev = [torch.from_numpy(a).to(device) for a in host]
    views, arrays = [], []
    for b in range(B):
        lo = misalign + (b * (Cn + 1) + 1) * h * w
        views.append(dev[b % 2][lo:lo + Cn * h * w])
        arrays.append(host[b % 2][lo:lo + Cn * h * w])
    return views, arrays


def guarded(n, device):
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=device)
    return buf, buf[GUARD:GUARD + n]


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("shapes", restated.SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}to{s[1][0]}x{s[1][1]}")
def test_hand_off_equals_restatement_and_multi_step_route(cuda, shapes, B):
    from frlw_evd_amd import event_representation as er
    from frlw_evd_amd import transforms
    (h, w), (H, W) = shapes
    misalign = 1 if (h, w) == (90, 160) else 0
    for Cn in CHANNELS:
        views, arrays = make_sources(B, Cn, h, w, 100 * B + Cn, cuda, misalign)
        if misalign or (h * w) % 4:
            assert any(v.data_ptr() % 4 for v in views)   # the case is about unaligned plane addresses
        buf, out = guarded(B * Cn * H * W, cuda)
        got = transforms.hand_off(views, Cn, (h, w), (H, W), out=out)
        assert got.data_ptr() == out.data_ptr()
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert (host[:GUARD] == np.float32(SENTINEL)).all() and (host[-GUARD:] == np.float32(SENTINEL)).all(), (shapes, B, Cn)
        got = host[GUARD:-GUARD].reshape(B, Cn, H, W)
        want = restated.hand_off(arrays, Cn, (h, w), (H, W))
        assert got.tobytes() == want.tobytes(), (shapes, B, Cn, int((got != want).sum()))
        # the route it replaces: stack the samples, resize, transform with default parameters
        vol = torch.stack([v.reshape(Cn, h, w) for v in views])
        if (h, w) != (H, W):
            vol = er.resize_nearest(vol.reshape(B * Cn, h, w), (H, W))
        steps = transforms.transform_images(vol.reshape(B, Cn, H, W), [transforms.SampleParams()] * B)
        assert steps.shape == (B, Cn, H, W, 1, 1)
        assert steps.cpu().numpy().tobytes() == want.tobytes(), (shapes, B, Cn)


def test_fresh_output_has_the_loader_shape(cuda):
    from frlw_evd_amd import transforms
    views, arrays = make_sources(3, 2, 57, 73, 7, cuda)
    got = transforms.hand_off(views, 2, (57, 73), (61, 97))
    assert got.shape == (3, 2, 61, 97, 1, 1) and got.dtype == torch.float32
    assert got.cpu().numpy().tobytes() == restated.hand_off(arrays, 2, (57, 73), (61, 97)).tobytes()


def test_bad_arguments_write_nothing(cuda):
    from frlw_evd_amd import _lib, transforms
    lib = _lib.load()
    h, w, H, W, Cn = 8, 12, 8, 12, 2
    views, _ = make_sources(2, Cn, h, w, 3, cuda)
    buf, out = guarded(65 * Cn * H * W, cuda)
    stream = torch.cuda.current_stream().cuda_stream
    table = (C.c_void_p * 65)(*[views[b % 2].data_ptr() for b in range(65)])
    for bad_B in (0, -1, 65):
        assert lib.frlw_volume_hand_off_u8(table, bad_B, Cn, h, w, H, W, out.data_ptr(), stream) == _lib.FRLW_ERR_ARG
    for sizes in ((0, h, w, H, W), (Cn, 0, w, H, W), (Cn, h, -3, H, W), (Cn, h, w, 0, W), (Cn, h, w, H, 0)):
        assert lib.frlw_volume_hand_off_u8(table, 2, *sizes, out.data_ptr(), stream) == _lib.FRLW_ERR_ARG
    assert lib.frlw_volume_hand_off_u8(None, 2, Cn, h, w, H, W, out.data_ptr(), stream) == _lib.FRLW_ERR_ARG
    assert lib.frlw_volume_hand_off_u8(table, 2, Cn, h, w, H, W, None, stream) == _lib.FRLW_ERR_ARG
    hole = (C.c_void_p * 2)(views[0].data_ptr(), None)
    assert lib.frlw_volume_hand_off_u8(hole, 2, Cn, h, w, H, W, out.data_ptr(), stream) == _lib.FRLW_ERR_ARG
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())
    with pytest.raises(ValueError):
        transforms.hand_off([views[0]] * 65, Cn, (h, w), (H, W))
    with pytest.raises(ValueError):
        transforms.hand_off([], Cn, (h, w), (H, W))
    with pytest.raises(ValueError):
        transforms.hand_off([views[0][:Cn * h * w - 1]], Cn, (h, w), (H, W))     # fewer bytes than C planes
    with pytest.raises(ValueError):
        transforms.hand_off([views[0].cpu()], Cn, (h, w), (H, W))
    assert bool((buf == SENTINEL).all())
