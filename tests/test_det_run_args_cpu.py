"""frlw_det_run's buffer binding and the size checks of the frlw_det_add_* calls, on a machine without a GPU.

Every op kind that reads or writes a buffer answers FRLW_ERR_ARG when one of its buffers resolves to NULL -- an index past the
table, or a NULL entry -- and it answers before it launches anything, so no device is needed: the weight pointers and the table's
entries are fake addresses that nothing dereferences.  (Optional buffers are left out of the plans: a convolution without a
residual, a decode without the decoded boxes.)"""
import ctypes as C

import pytest

from frlw_evd_amd import _lib

W_, B_ = C.c_void_p(0x1000), C.c_void_p(0x2000)  # weights and bias: never dereferenced, adding an op launches nothing
ONE = (C.c_int * 1)(1)


def _add_conv(lib, d):
    return lib.frlw_det_add_conv(d, 0, 4, 0, 4, 2, 2, W_, B_, 4, 32, 1, 1, 1, 4, 0, 0, -1, 0, 0, 0, 0, 0)


def _add_focus(lib, d):
    return lib.frlw_det_add_focus(d, 0, 3, 4, 4, 1)


def _add_upsample(lib, d):
    return lib.frlw_det_add_upsample(d, 0, 4, 0, 4, 2, 2, 1, 4, 0)


def _add_spp(lib, d):
    return lib.frlw_det_add_spp_pool(d, 1, 16, 4, 2, 2)


def _add_decode(lib, d):
    return lib.frlw_det_add_decode_nms(d, 0, 4, 1, 1, ONE, ONE, ONE, 0.5, 0.5, -1, 1, 2, 3)


def _add_bfm(lib, d):
    return lib.frlw_det_add_bfm_stem(d, 0, 4, 2, 2, W_, lib.frlw_det_bfm_weight_count(4), 1)


def _add_pred(lib, d):
    return lib.frlw_det_add_pred(d, 0, 8, 0, 4, 4, W_, B_, 6, 1, 0, 24)


def _add_focus_stem(lib, d):
    return lib.frlw_det_add_focus_stem(d, 0, 4, 4, 4, W_, B_, 32, 1, 32, 0)


# kind -> (the one op, the buffer indices it must find bound)
KINDS = {
    "conv": (_add_conv, (0, 1)),
    "focus": (_add_focus, (0, 1)),
    "upsample": (_add_upsample, (0, 1)),
    "spp": (_add_spp, (1,)),
    "decode": (_add_decode, (0, 1, 2, 3)),
    "bfm": (_add_bfm, (0, 1)),
    "pred": (_add_pred, (0, 1)),
    "focus_stem": (_add_focus_stem, (0, 1)),
}


def _table(n, null_at=None):
    return (C.c_void_p * max(n, 1))(*[C.c_void_p(None if i == null_at else 0x10000 * (i + 1)) for i in range(max(n, 1))])


@pytest.mark.parametrize("kind", list(KINDS))
def test_unbound_buffer_is_an_argument_error(kind):
    """A table one short of the highest index, then a NULL at every index the op uses (the highest included)."""
    lib = _lib.load()
    add, used = KINDS[kind]
    top = max(used)
    d = lib.frlw_det_create()
    try:
        assert add(lib, d) == _lib.FRLW_OK
        assert lib.frlw_det_num_ops(d) == 1
        assert lib.frlw_det_run(d, 1, _table(top), top, 0, -1, None) == _lib.FRLW_ERR_ARG, "table too short"
        for i in sorted(used, reverse=True):
            assert lib.frlw_det_run(d, 1, _table(top + 1, null_at=i), top + 1, 0, -1, None) == _lib.FRLW_ERR_ARG, f"NULL at {i}"
    finally:
        lib.frlw_det_destroy(d)


@pytest.mark.parametrize("bad", [(0, 4, 4), (-1, 4, 4), (4, 0, 4), (4, 4, 0), (4, -2, 4), (4, 4, -2)])
def test_sizes_below_one_are_argument_errors(bad):
    """C, H or W below 1: FRLW_ERR_ARG from the four calls that used to build an empty grid or an empty LDS request from them,
    and no op is added."""
    lib = _lib.load()
    Cc, H, W = bad
    n_w = lib.frlw_det_bfm_weight_count(4)
    calls = {
        "focus": lambda d: lib.frlw_det_add_focus(d, 0, Cc, H, W, 1),
        "bfm": lambda d: lib.frlw_det_add_bfm_stem(d, 0, Cc, H, W, W_, n_w, 1),
        "upsample": lambda d: lib.frlw_det_add_upsample(d, 0, 4, 0, Cc, H, W, 1, 4, 0),
        "spp": lambda d: lib.frlw_det_add_spp_pool(d, 0, 16, Cc, H, W),
    }
    for name, call in calls.items():
        d = lib.frlw_det_create()
        try:
            assert _add_focus(lib, d) == _lib.FRLW_OK  # (no convolution in front: an upsample must not fuse into it)
            assert call(d) == _lib.FRLW_ERR_ARG, name
            assert lib.frlw_det_num_ops(d) == 1, name
        finally:
            lib.frlw_det_destroy(d)


def test_upsample_of_no_size_does_not_fuse_into_a_convolution():
    """The fused form (the convolution before it stores the upsampled copy) is refused like the launch of its own."""
    lib = _lib.load()
    d = lib.frlw_det_create()
    try:
        assert lib.frlw_det_add_conv(d, 0, 4, 0, 4, 0, 0, W_, B_, 4, 32, 1, 1, 1, 4, 0, 0, -1, 0, 0, 0, 0, 0) == _lib.FRLW_OK
        assert lib.frlw_det_add_upsample(d, 1, 4, 0, 4, 0, 0, 2, 4, 0) == _lib.FRLW_ERR_ARG
        assert lib.frlw_det_num_ops(d) == 1
    finally:
        lib.frlw_det_destroy(d)
