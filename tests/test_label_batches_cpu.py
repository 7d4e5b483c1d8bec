"""A file's labels per call (frlw_sae_encode_chain, frlw_ev_encode_ranges) -- what can be checked without a GPU: the symbols, the
host-only size queries and counter, the argument checks that answer before any device call, and the pure functions of
frlw_evd_amd/generate.py that turn a file's label slices into the steps / jobs of the two offline commands."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import harness_data
from frlw_evd_amd import _lib, dat_io

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("frlw_sae_chain_workspace_bytes", "frlw_sae_encode_chain", "frlw_ev_ranges_workspace_bytes", "frlw_ev_encode_ranges",
       "frlw_encoder_chain_counts")
DENSE_LABELS = np.arange(100_000, 7_150_000, 70_000, dtype=np.int64)   # 101 labels on test/seqA: more than one part


def test_symbols_resolve_and_are_declared():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "frlw_evd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SYMBOLS, name
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} is not declared in include/frlw_evd.h"
    from frlw_evd_amd import event_representation as er
    assert callable(er.encode_sae_chain) and callable(er.encode_ev_ranges)


def test_workspace_queries_are_host_only():
    lib = _lib.load()
    chain, batch = lib.frlw_sae_chain_workspace_bytes, lib.frlw_sae_batch_workspace_bytes
    for k in (0, 65):
        assert chain(1_000, k, 240, 304) == 0
        assert lib.frlw_ev_ranges_workspace_bytes(1_000, k, 240, 304, 250_000) == 0
    assert chain(1_000, 1, 0, 304) == 0 and chain(1_000, 1, 240, -3) == 0
    assert lib.frlw_ev_ranges_workspace_bytes(1_000, 1, 0, 304, 250_000) == 0
    assert lib.frlw_ev_ranges_workspace_bytes(1_000, 1, 240, -3, 250_000) == 0
    assert lib.frlw_ev_ranges_workspace_bytes(1_000, 1, 240, 304, 1 << 20) == 0     # the window does not fit the 4-byte record
    for n, k, H, W in ((0, 1, 8, 12), (100_000, 1, 240, 304), (100_000, 64, 240, 304), (5, 7, 53, 91)):
        assert chain(n, k, H, W) == batch(n, k, H, W) > 0                           # the same key planes
    for n, k, H, W, win in ((0, 1, 53, 91, 50_000), (1, 5, 240, 304, 250_000), (123_457, 5, 240, 304, 250_000),
                            (3_000_000, 64, 240, 304, 1_000_000), (600_000, 3, 512, 640, 80_000)):
        inner = lib.frlw_ev_batch_workspace_bytes(n, k, H, W, win)
        assert inner > 0
        assert lib.frlw_ev_ranges_workspace_bytes(n, k, H, W, win) >= 8 * n + inner, (n, k, H, W, win)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    p = C.c_void_p(0x1000)  # never dereferenced: the answers come from host-side argument checks
    ev = _lib.FrlwEvents(0x2000, 100, _lib.LAYOUT_DAT8, 0, None, None, 0, 0, None)
    i64 = lambda *v: (C.c_int64 * len(v))(*v)  # noqa: E731
    lo, hi, now, win = i64(*([0] * 65)), i64(*([10] * 65)), i64(*([50] * 65)), i64(*([7] * 65))
    emit = (C.c_uint8 * 65)(*([1] * 65))
    lam = (C.c_double * 3)(1e-5, 2.5e-6, 1e-6)
    big = 1 << 20

    def chain(lo=lo, hi=hi, now=now, win=win, emit=emit, n=2, H=8, W=12, lam=lam, nl=3, mem_out=p, f32=p, ws=p, ws_bytes=big, ev=ev):
        return lib.frlw_sae_encode_chain(C.byref(ev), lo, hi, now, win, emit, n, H, W, lam, nl, None, mem_out, f32, None, ws, ws_bytes, None)

    assert chain(n=0) == _lib.FRLW_ERR_ARG and chain(n=65) == _lib.FRLW_ERR_ARG
    assert chain(lo=hi, hi=lo) == _lib.FRLW_ERR_ARG                                   # runs backwards
    assert chain(hi=i64(10, 101)) == _lib.FRLW_ERR_ARG                                # leaves the array
    assert chain(lo=i64(-1, 0)) == _lib.FRLW_ERR_ARG
    assert chain(mem_out=None) == _lib.FRLW_ERR_ARG and chain(ws=None) == _lib.FRLW_ERR_ARG
    assert chain(lo=None) == _lib.FRLW_ERR_ARG and chain(now=None) == _lib.FRLW_ERR_ARG and chain(emit=None) == _lib.FRLW_ERR_ARG
    assert chain(f32=None) == _lib.FRLW_ERR_ARG                                       # a step emits, nowhere to write
    assert chain(nl=9) == _lib.FRLW_ERR_ARG
    assert chain(H=0) == _lib.FRLW_ERR_ARG
    assert chain(ws_bytes=1024) == _lib.FRLW_ERR_WORKSPACE
    f64 = _lib.FrlwEvents(0x2000, 100, _lib.LAYOUT_XYTP_F64, 4, None, None, 0, 0, None)
    assert chain(ev=f64) == _lib.FRLW_ERR_UNSUPPORTED

    def ranges(lo=lo, hi=hi, te=now, n=2, H=8, W=12, bins=5, win=1000, f32=p, ws=p, ws_bytes=big, ev=ev):
        return lib.frlw_ev_encode_ranges(C.byref(ev), lo, hi, te, n, H, W, bins, win, f32, None, ws, ws_bytes, None)

    assert ranges(n=0) == _lib.FRLW_ERR_ARG and ranges(n=65) == _lib.FRLW_ERR_ARG
    assert ranges(lo=hi, hi=lo) == _lib.FRLW_ERR_ARG
    assert ranges(hi=i64(10, 101)) == _lib.FRLW_ERR_ARG
    assert ranges(lo=i64(-1, 0)) == _lib.FRLW_ERR_ARG
    assert ranges(f32=None) == _lib.FRLW_ERR_ARG and ranges(ws=None) == _lib.FRLW_ERR_ARG and ranges(te=None) == _lib.FRLW_ERR_ARG
    assert ranges(bins=0) == _lib.FRLW_ERR_ARG and ranges(win=0) == _lib.FRLW_ERR_ARG
    assert ranges(H=0) == _lib.FRLW_ERR_ARG
    assert ranges(ws_bytes=1024) == _lib.FRLW_ERR_WORKSPACE
    need = lib.frlw_ev_ranges_workspace_bytes(20, 2, 8, 12, 1000)
    assert ranges(ws_bytes=need - 1) == _lib.FRLW_ERR_WORKSPACE                       # the copy counts
    assert ranges(win=1 << 20) == _lib.FRLW_ERR_UNSUPPORTED
    assert ranges(ev=f64) == _lib.FRLW_ERR_UNSUPPORTED
    assert lib.frlw_encoder_chain_counts(None) == _lib.FRLW_ERR_ARG


def test_chain_counters_start_at_zero():
    code = ("import ctypes as C, sys; sys.path.insert(0, sys.argv[1]); from frlw_evd_amd import _lib; lib = _lib.load(); "
            "c = (C.c_uint64 * 2)(7, 7); r = lib.frlw_encoder_chain_counts(c); print(r, list(c))")
    p = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert p.stdout.split("\n")[-2] == "0 [0, 0]"


def test_python_layer_validates_before_any_device_call():
    """CPU tensors: everything below must raise ValueError from the argument checks -- reaching the device layer with them
    would raise RuntimeError ("dat must be a CUDA tensor") instead."""
    from frlw_evd_amd import event_representation as er
    dat = torch.zeros((100, 8), dtype=torch.uint8)
    lam = [1e-5, 2.5e-6, 1e-6]
    step = (0, 10, 50, 7, True)
    for steps in ([], [step] * 65, [(0, 10, 50, 7)], [(0, 10, 50, 7, True, 1)], [(30, 20, 50, 7, True)], [(0, 101, 50, 7, True)],
                  [(-1, 5, 50, 7, False)]):
        with pytest.raises(ValueError):
            er.encode_sae_chain(dat, steps, (8, 12), lam, None)
    with pytest.raises(ValueError):
        er.encode_sae_chain(dat, [step], (8, 12), [1e-6] * 9, None)
    with pytest.raises(ValueError):
        er.encode_sae_chain(dat, [step], (8, 12), lam, torch.zeros((1, 2, 8, 12)))
    with pytest.raises(ValueError):
        er.encode_sae_chain(dat, [step], (8, 12), lam, None, want_f32=False, want_u8=False)
    for rng in ([], [(0, 10)] * 65, [(0, 10), (30, 20)], [(0, 101)], [(-1, 5)]):
        with pytest.raises(ValueError):
            er.encode_ev_ranges(dat, rng, (8, 12), 50, 1000)
    with pytest.raises(ValueError):
        er.encode_ev_ranges(dat, [(0, 10), (5, 20)], (8, 12), [50], 1000)            # one t_end per window
    with pytest.raises(ValueError):
        er.encode_ev_ranges(dat, [(0, 10)], (8, 12), 50, 1000, want_f32=False, want_u8=False)


# ---- the job lists of the two commands -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return harness_data.build(str(tmp_path_factory.mktemp("label_batches")))


def files(dataset):
    """(mode, event file, label times): the two sequences with their own labels, and test/seqA and train/seqB with 101 labels."""
    raw, _ = dataset
    out = []
    for (mode, name) in harness_data.SEQUENCES:
        path = os.path.join(raw, mode, name + "_td.dat")
        out.append((mode, path, harness_data.label_times(mode, name)))
        out.append((mode, path, DENSE_LABELS))
    return out


def test_sae_step_list(dataset):
    from frlw_evd_amd import generate
    windows = generate.SAE_TIME_WINDOWS
    assert windows == [554126, 2216505, 5541263]
    most = 0
    for mode, path, labels in files(dataset):
        slices = list(dat_io.sae_label_slices(dat_io.DatFile(path), labels))
        steps = generate.sae_steps(dat_io.sae_label_slices(dat_io.DatFile(path), labels), mode)
        per = windows if mode == "test" else [max(windows)]
        assert len(slices) > 0 and len(steps) == len(slices) * len(per)
        want = [(sl["start_count"], sl["end_count"], sl["label_time"], tw, tw == per[-1]) for sl in slices for tw in per]
        assert [tuple(s) for s in steps] == want                       # every slice once per window, in order; now = label time
        assert all(len(s) == 5 for s in steps)
        if mode == "test":
            assert [bool(s[4]) for s in steps] == [False, False, True] * len(slices)
            assert [s[3] for s in steps[:3]] == windows
        else:
            assert all(s[4] for s in steps) and {s[3] for s in steps} == {max(windows)}
        parts = generate.sae_parts(steps)
        assert [s for part in parts for s in part] == steps
        assert all(1 <= len(part) <= _lib.MAX_SEQUENCES for part in parts)
        assert len(parts) == -(-len(steps) // _lib.MAX_SEQUENCES)
        most = max(most, len(parts))
    assert most >= 5   # 101 labels x 3 windows: parts that end between the three steps of one label (64 is no multiple of 3)


def test_ev_job_list(dataset):
    from frlw_evd_amd import generate
    windows = generate.EV_TIME_WINDOWS
    assert windows == [250000, 500000, 1000000]
    narrowed = split_by_budget = 0
    for mode, path, labels in files(dataset):
        f = dat_io.DatFile(path)
        t = np.asarray(f.records["t"]).astype(np.int64)
        slices = list(dat_io.ev_label_slices(f, labels, windows))
        assert len(slices) > 0
        for tw in windows:
            plain = generate.ev_jobs(slices, tw, "out/seq")
            jobs = generate.ev_jobs(slices, tw, "out/seq", f._t)
            assert len(jobs) == len(plain) == len(slices)
            for sl, raw_job, job in zip(slices, plain, jobs):           # every slice once, in order
                assert raw_job == (sl["start_count"], sl["end_count"], sl["end_time"], f"out/seq_{sl['label_time']}.npy")
                lo, hi, end, out_path = job
                assert (hi, end, out_path) == raw_job[1:] and sl["start_count"] <= lo <= hi
                # the narrowed lo drops only records the encoder drops anyway: none with t > end_time - tw
                assert not (t[sl["start_count"]:lo] > end - tw).any(), (mode, tw, sl["label_time"])
                assert lo == hi or t[lo] > end - tw
                narrowed += lo > sl["start_count"]
            for budget in (generate.EV_RECORD_BUDGET, 300_000):
                parts = generate.ev_parts(jobs, _lib.MAX_SEQUENCES, budget)
                assert [j for part in parts for j in part] == jobs
                for part in parts:
                    assert 1 <= len(part) <= _lib.MAX_SEQUENCES
                    assert len(part) == 1 or sum(hi - lo for lo, hi, _, _ in part) <= budget
                split_by_budget += len(parts) > -(-len(jobs) // _lib.MAX_SEQUENCES)
            assert all(len(part) <= 7 for part in generate.ev_parts(jobs, 7))
    assert narrowed > 0 and split_by_budget > 0
