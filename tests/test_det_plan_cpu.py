"""The detector plan through the C ABI on a machine without a GPU: which Focus + stem shapes frlw_det_add_focus_stem takes.

The table is what the library answered BEFORE the stem's kernel, LDS and grid were resolved in one place (focus_stem_plan of
csrc/det_focus.h): FRLW_ERR_UNSUPPORTED exactly for C outside {4, 8, 10, 16}, for Cout > 64, and for C = 16 with Cout > 32 in the
bf16x3 arithmetic (measured slower than Focus + convolution); every other shape is one op."""
import ctypes as C

import pytest

from frlw_evd_amd import _lib

OK, NO = (_lib.FRLW_OK, 1), (_lib.FRLW_ERR_UNSUPPORTED, 0)  # (status, frlw_det_num_ops afterwards)
COUTS = (16, 32, 48, 64, 96)
# {precision: {C: the answers for Cout = 16, 32, 48, 64, 96}}, recorded from the library
TABLE = {
    0: {4: (OK, OK, OK, OK, NO), 6: (NO,) * 5, 8: (OK, OK, OK, OK, NO), 10: (OK, OK, OK, OK, NO), 12: (NO,) * 5, 16: (OK, OK, OK, OK, NO)},
    1: {4: (OK, OK, OK, OK, NO), 6: (NO,) * 5, 8: (OK, OK, OK, OK, NO), 10: (OK, OK, OK, OK, NO), 12: (NO,) * 5, 16: (OK, OK, NO, NO, NO)},
}


@pytest.mark.parametrize("precision", [0, 1])
def test_focus_stem_shapes_accepted(precision):
    lib = _lib.load()
    w, bias = C.c_void_p(0x1000), C.c_void_p(0x2000)  # never dereferenced: adding an op launches nothing
    for Cin, row in TABLE[precision].items():
        for Cout, want in zip(COUTS, row):
            d = lib.frlw_det_create()
            try:
                assert lib.frlw_det_set_precision(d, precision) == _lib.FRLW_OK
                rc = lib.frlw_det_add_focus_stem(d, 0, Cin, 64, 96, w, bias, Cout, 1, Cout, 0)
                assert (rc, lib.frlw_det_num_ops(d)) == want, (Cin, Cout, precision)
            finally:
                lib.frlw_det_destroy(d)
