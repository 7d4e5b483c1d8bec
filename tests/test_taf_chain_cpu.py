"""The host side of the TAF chain (no GPU needed): the planner that groups a file's labels into chains (generate.taf_chains),
the argument checks of frlw_taf_encode_chain, and the compiler's resource report of the tile kernels -- k_taf_tile_snap keeps
its FIFO in registers like k_taf_tile, and k_taf_tile itself is the kernel it was before the snapshots were added."""
import ctypes as C
import os
import subprocess

import pytest

from frlw_evd_amd import _build, _lib, generate
from test_kernel_resources_cpu import _hipcc, parse_resource_remarks

WIN = 10_000


def label(start_time, bins, start_count, end_count, fresh=False, end_time=None, label_time=None):
    end_time = start_time + bins * WIN if end_time is None else end_time
    return {"label_time": end_time if label_time is None else label_time, "start_count": start_count, "end_count": end_count,
            "start_time": start_time, "end_time": end_time, "bins": bins, "fresh": fresh}


def run_of(n, t0=100_000, bins=2, per=50, fresh_first=True):
    """n contiguous labels of `bins` windows and `per` records each, the first one fresh."""
    return [label(t0 + i * bins * WIN, bins, i * per, (i + 1) * per, fresh=fresh_first and i == 0) for i in range(n)]


def early(sl):
    """Every label's last record lies one microsecond in front of its end."""
    return sl["end_time"] - 1 if sl["end_count"] > sl["start_count"] else None


def ids(chains):
    return [[sl["label_time"] for sl in c] for c in chains]


def test_five_contiguous_labels_are_one_chain():
    sl = run_of(5)
    chains = generate.taf_chains(sl, early)
    assert ids(chains) == [[s["label_time"] for s in sl]]
    assert chains[0][0] is sl[0]   # the planner hands the slices through


def test_a_fresh_label_starts_a_chain():
    sl = run_of(5)
    sl[3]["fresh"] = True
    assert [len(c) for c in generate.taf_chains(sl, early)] == [3, 2]


def test_a_label_without_windows_stays_alone():
    """bins <= 0: the double-transform branch needs the state at that point -- the chain in front of it is closed, and the label
    behind it starts a new one."""
    sl = run_of(2)
    t = sl[-1]["end_time"]
    sl.append(label(t, 0, 100, 100, label_time=t + 3))
    sl.append(label(t, 0, 100, 100, label_time=t + 4))
    sl += [label(t, 2, 100, 150), label(t + 2 * WIN, 2, 150, 200)]
    assert [len(c) for c in generate.taf_chains(sl, early)] == [2, 1, 1, 2]


def test_a_label_behind_a_clipped_one_is_off_the_grid():
    """The predecessor's end was clipped to total_time(): bins = ceil(...) windows, but the next label starts at the clipped time."""
    sl = run_of(2)
    t = sl[-1]["end_time"]
    sl.append(label(t, 2, 100, 150, end_time=t + 2 * WIN - 4_000))
    sl.append(label(t + 2 * WIN - 4_000, 1, 150, 200))
    assert [len(c) for c in generate.taf_chains(sl, early)] == [3, 1]


def test_equal_timestamps_at_a_label_end_break_the_chain():
    """seek_time landed inside a run of records at exactly the label's end: the per-label call clamps them into its last window."""
    sl = run_of(4)
    on_the_end = lambda s: s["end_time"] if s is sl[1] else early(s)  # noqa: E731
    assert [len(c) for c in generate.taf_chains(sl, on_the_end)] == [2, 2]
    assert [len(c) for c in generate.taf_chains(sl, lambda s: s["end_time"])] == [1, 1, 1, 1]
    empty = run_of(3, per=0)   # labels without records have no last record
    assert [len(c) for c in generate.taf_chains(empty, early)] == [3]


def test_at_most_64_snapshots_per_chain():
    sl = run_of(150, bins=1)
    chains = generate.taf_chains(sl, early)
    assert [len(c) for c in chains] == [64, 64, 22]
    assert [s["label_time"] for c in chains for s in c] == [s["label_time"] for s in sl]   # every label once, in order
    # the chain behind a full one starts on its own grid
    assert chains[1][0]["start_time"] == sl[64]["start_time"]


def test_argument_checks_are_host_only():
    """Every FRLW_ERR_ARG case of frlw_taf_encode_chain is answered before anything touches the device (the pointers are never
    dereferenced)."""
    lib = _lib.load()
    p = C.c_void_p(0x1000)
    dat = _lib.FrlwEvents(0x2000, 100, _lib.LAYOUT_DAT8, 0, None, None, 0, 0, None)
    f64 = _lib.FrlwEvents(0x2000, 100, _lib.LAYOUT_XYTP_F64, 4, None, None, 0, 0, None)

    def call(ev=dat, n_windows=8, mask=0b101, state=p, snap=p, window_us=WIN, K=8):
        return lib.frlw_taf_encode_chain(C.byref(ev) if ev is not None else None, 20, 300, K, 0, window_us, n_windows, mask, state,
                                         snap, 0, p, 1 << 20, None)
    assert call(mask=0) == _lib.FRLW_ERR_ARG
    assert call(mask=1 << 8) == _lib.FRLW_ERR_ARG
    assert call(mask=0b101 | 1 << 63) == _lib.FRLW_ERR_ARG
    assert call(n_windows=0) == _lib.FRLW_ERR_ARG
    assert call(n_windows=65, mask=1) == _lib.FRLW_ERR_ARG
    assert call(state=None) == _lib.FRLW_ERR_ARG
    assert call(snap=None) == _lib.FRLW_ERR_ARG
    assert call(ev=f64, n_windows=1, mask=1) == _lib.FRLW_ERR_ARG
    assert call(ev=None) == _lib.FRLW_ERR_ARG
    assert call(window_us=0) == _lib.FRLW_ERR_ARG
    assert call(window_us=-5) == _lib.FRLW_ERR_ARG
    assert call(K=0) == _lib.FRLW_ERR_ARG and call(K=9) == _lib.FRLW_ERR_ARG


# What -Rpass-analysis=kernel-resource-usage reports for k_taf_tile<NT> on the parent of the commit that added k_taf_tile_snap
# (a compile of that tree's encoders.hip with _build.HIPCC_FLAGS).
PARENT_TAF_TILE = {
    256: {"TotalSGPRs": "106", "VGPRs": "104", "AGPRs": "0", "ScratchSize": "0", "Dynamic Stack": "False", "Occupancy": "4",
          "SGPRs Spill": "13", "VGPRs Spill": "0", "LDS Size": "38336"},
    512: {"TotalSGPRs": "106", "VGPRs": "113", "AGPRs": "0", "ScratchSize": "0", "Dynamic Stack": "False", "Occupancy": "4",
          "SGPRs Spill": "29", "VGPRs Spill": "0", "LDS Size": "75200"},
    1024: {"TotalSGPRs": "106", "VGPRs": "108", "AGPRs": "0", "ScratchSize": "0", "Dynamic Stack": "False", "Occupancy": "4",
           "SGPRs Spill": "17", "VGPRs Spill": "0", "LDS Size": "148928"},
}


@pytest.fixture(scope="module")
def encoder_rows(tmp_path_factory):
    exe = _hipcc()
    if exe is None:
        pytest.skip("hipcc not installed")
    obj = tmp_path_factory.mktemp("resusage") / "encoders.o"
    flags = [f for f in _build.HIPCC_FLAGS if f != "-shared"] + ["-I", _build.INCLUDE, "-I", _build.CSRC, "-c",
                                                                "-Rpass-analysis=kernel-resource-usage"]
    p = subprocess.run([exe] + flags + [os.path.join(_build.CSRC, "encoders.hip"), "-o", str(obj)], capture_output=True, text=True,
                       timeout=900)
    assert p.returncode == 0, p.stderr[-4000:]
    return parse_resource_remarks(p.stderr)


def instance(rows, kernel, nt):
    hit = [r for name, r in rows.items() if f"{len(kernel)}{kernel}ILi{nt}E" in name]
    assert len(hit) == 1, (kernel, nt, sorted(rows))
    return hit[0]


@pytest.mark.parametrize("nt", [256, 512, 1024])
def test_snapshot_kernel_keeps_its_fifo_in_registers(encoder_rows, nt):
    """st[4][8], the sums and the counts live in VGPRs across the snapshot's look-ups: no scratch at any width (NT = 1024 has 128
    VGPRs per lane)."""
    r = instance(encoder_rows, "k_taf_tile_snap", nt)
    assert r["ScratchSize"] == "0" and r["VGPRs Spill"] == "0" and r["Dynamic Stack"] == "False", r


@pytest.mark.parametrize("nt", [256, 512, 1024])
def test_tile_kernel_is_the_one_it_was(encoder_rows, nt):
    assert instance(encoder_rows, "k_taf_tile", nt) == PARENT_TAF_TILE[nt]
