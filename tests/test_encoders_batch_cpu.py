"""Batched Event Count Image / Surface of Active Events (csrc/encoders_batch.hip): what can be checked without a GPU -- the six
symbols, the host-only size queries and counters, and the argument validation of the Python layer, which raises before any
device call."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from frlw_evd_amd import _lib

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("frlw_eci_batch_workspace_bytes", "frlw_eci_encode_batch", "frlw_sae_batch_workspace_bytes", "frlw_sae_encode_batch",
       "frlw_encoder_batch_counts")


def test_symbols_resolve_and_are_declared():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "frlw_evd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SYMBOLS, name
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} is not declared in include/frlw_evd.h"
    from frlw_evd_amd import event_representation as er
    assert callable(er.encode_eci_batch) and callable(er.encode_sae_batch)


def test_workspace_queries_are_host_only():
    lib = _lib.load()
    for query, cell in ((lib.frlw_eci_batch_workspace_bytes, 4), (lib.frlw_sae_batch_workspace_bytes, 8)):
        assert query(1_000, 65, 240, 304) == 0          # more than FRLW_MAX_SEQUENCES windows
        assert query(1_000, 0, 240, 304) == 0
        assert query(1_000, 1, 0, 304) == 0
        one = query(100_000, 1, 240, 304)
        assert one >= 2 * 240 * 304 * cell              # one integer per cell of the window's plane, behind the header
        assert query(100_000, 64, 240, 304) >= 64 * 2 * 240 * 304 * cell > one
        assert query(0, 1, 53, 91) > 0                  # the record count does not size the planes


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    p = C.c_void_p(0x1000)  # never dereferenced: the answers come from host-side argument checks
    ev = _lib.FrlwEvents(0x2000, 100, _lib.LAYOUT_DAT8, 0, None, None, 0, 0, None)
    lo, hi = (C.c_int64 * 65)(*([0] * 65)), (C.c_int64 * 65)(*([10] * 65))
    assert lib.frlw_eci_encode_batch(C.byref(ev), lo, hi, 65, 8, 12, p, None, p, 1 << 20, None) == _lib.FRLW_ERR_ARG
    assert lib.frlw_eci_encode_batch(C.byref(ev), lo, hi, 0, 8, 12, p, None, p, 1 << 20, None) == _lib.FRLW_ERR_ARG
    assert lib.frlw_eci_encode_batch(C.byref(ev), lo, hi, 2, 8, 12, None, None, p, 1 << 20, None) == _lib.FRLW_ERR_ARG  # no output
    assert lib.frlw_eci_encode_batch(C.byref(ev), lo, hi, 2, 8, 12, p, None, p, 1024, None) == _lib.FRLW_ERR_WORKSPACE
    assert lib.frlw_eci_encode_batch(C.byref(ev), hi, lo, 2, 8, 12, p, None, p, 1 << 20, None) == _lib.FRLW_ERR_ARG    # hi < lo
    far = (C.c_int64 * 2)(0, 101)
    assert lib.frlw_eci_encode_batch(C.byref(ev), lo, far, 2, 8, 12, p, None, p, 1 << 20, None) == _lib.FRLW_ERR_ARG   # behind the array
    f64 = _lib.FrlwEvents(0x2000, 100, _lib.LAYOUT_XYTP_F64, 4, None, None, 0, 0, None)
    assert lib.frlw_eci_encode_batch(C.byref(f64), lo, hi, 2, 8, 12, p, None, p, 1 << 20, None) == _lib.FRLW_ERR_UNSUPPORTED
    offs, now = (C.c_int64 * 66)(*range(66)), (C.c_int64 * 65)(*([5] * 65))
    lam = (C.c_double * 3)(1e-5, 2.5e-6, 1e-6)
    assert lib.frlw_sae_encode_batch(C.byref(ev), offs, now, 65, 8, 12, lam, 3, None, p, 0, p, None, p, 1 << 20, None) == _lib.FRLW_ERR_ARG
    assert lib.frlw_sae_encode_batch(C.byref(ev), offs, now, 2, 8, 12, lam, 3, None, None, 0, p, None, p, 1 << 20, None) == _lib.FRLW_ERR_ARG
    assert lib.frlw_sae_encode_batch(C.byref(ev), offs, now, 2, 8, 12, lam, 9, None, p, 0, p, None, p, 1 << 20, None) == _lib.FRLW_ERR_ARG
    assert lib.frlw_sae_encode_batch(C.byref(ev), offs, now, 2, 8, 12, lam, 3, None, p, 0, p, None, p, 1024, None) == _lib.FRLW_ERR_WORKSPACE
    back = (C.c_int64 * 3)(0, 50, 20)
    assert lib.frlw_sae_encode_batch(C.byref(ev), back, now, 2, 8, 12, lam, 3, None, p, 0, p, None, p, 1 << 20, None) == _lib.FRLW_ERR_ARG
    assert lib.frlw_encoder_batch_counts(None) == _lib.FRLW_ERR_ARG


def test_batch_counters_start_at_zero():
    code = ("import ctypes as C, sys; sys.path.insert(0, sys.argv[1]); from frlw_evd_amd import _lib; lib = _lib.load(); "
            "c = (C.c_uint64 * 2)(7, 7); r = lib.frlw_encoder_batch_counts(c); print(r, list(c))")
    p = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert p.stdout.split("\n")[-2] == "0 [0, 0]"


def test_python_layer_validates_before_any_device_call():
    """CPU tensors: everything below must raise ValueError from the argument checks -- reaching the device layer with them
    would raise RuntimeError ("dat must be a CUDA tensor") instead."""
    from frlw_evd_amd import event_representation as er
    dat = torch.zeros((100, 8), dtype=torch.uint8)
    with pytest.raises(ValueError):
        er.encode_eci_batch(dat, [(0, 10)] * 65, (8, 12))
    with pytest.raises(ValueError):
        er.encode_eci_batch(dat, [], (8, 12))
    with pytest.raises(ValueError):
        er.encode_eci_batch(dat, [(0, 10), (30, 20)], (8, 12))      # hi < lo
    with pytest.raises(ValueError):
        er.encode_eci_batch(dat, [(0, 101)], (8, 12))               # behind the array
    with pytest.raises(ValueError):
        er.encode_eci_batch(dat, [(0, 10)], (8, 12), want_f32=False, want_u8=False)
    lam = [1e-5, 2.5e-6, 1e-6]
    with pytest.raises(ValueError):
        er.encode_sae_batch(dat, list(range(66)), (8, 12), lam, None, 5, 0)
    with pytest.raises(ValueError):
        er.encode_sae_batch(dat, [0], (8, 12), lam, None, 5, 0)
    with pytest.raises(ValueError):
        er.encode_sae_batch(dat, [0, 50, 20], (8, 12), lam, None, 5, 0)
    with pytest.raises(ValueError):
        er.encode_sae_batch(dat, [0, 50, 100], (8, 12), lam, None, [5, 6, 7], 0)   # one `now` per sequence
    with pytest.raises(ValueError):
        er.encode_sae_batch(dat, [0, 50, 100], (8, 12), lam, torch.zeros((3, 2, 8, 12)), 5, 0)
    with pytest.raises(ValueError):
        er.encode_sae_batch(dat, [0, 50, 100], (8, 12), [1e-6] * 9, None, 5, 0)


def test_per_sequence_arguments_are_length_checked_before_any_device_call():
    """CPU tensors again.  ctypes zero-fills a short initialiser -- ``(c_int64 * 3)(*[5])`` is ``[5, 0, 0]`` -- so a ``t_start`` /
    ``t_end`` list one entry short would encode the last sequence from t = 0 without a word, and one entry too long raises ctypes'
    IndexError, which in this layer means "event coordinate out of range".  Both are ValueError from the argument checks, like a
    sequence list that descends, leaves ``dat`` or holds 0 or 65 sequences; an int applies to all and passes them (the device
    check behind them then turns the CPU tensor down with RuntimeError)."""
    from frlw_evd_amd import event_representation as er
    H, W, K = 8, 12, 8
    dat = torch.zeros((100, 8), dtype=torch.uint8)
    two = [0, 50, 100]

    def taf(offs, t_start):
        B = len(offs) - 1
        return er.encode_taf_batch(dat, offs, (H, W), torch.zeros((B, H, W, 2, K)), t_start, 10_000, 8, K)

    def stripe(offs, t_start):
        return er.encode_taf_stripe(dat, offs, (H, W), (0, 4), torch.zeros((len(offs) - 1, 4, W, 2, K)), t_start)

    def ev(offs, t_end):
        return er.encode_ev_batch(dat, offs, (H, W), t_end, 10_000)

    for call, items in ((taf, [0]), (taf, [0, 0, 0]), (stripe, [0]), (ev, [7]), (ev, [7, 7, 7])):
        with pytest.raises(ValueError):
            call(two, items)
    for call in (taf, ev):
        for offs in ([0, 50, 20], [0, 50, 101], [0], list(range(66))):
            with pytest.raises(ValueError):
                call(offs, 0)
    for call in (taf, stripe, ev):
        with pytest.raises(RuntimeError):
            call(two, 0)
