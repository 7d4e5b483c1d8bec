"""A file's labels per call on the GPU: the chained Surface of Active Events (frlw_sae_encode_chain) and the Event Volume over
record ranges (frlw_ev_encode_ranges).  Every comparison is bit-equal -- against the loop of single calls the new calls replace
(encode_sae_dat fed its own memory, encode_ev_dat per range), against the CPU oracle chained the same way, and, for the two offline
commands, against the files that loop writes."""
import ctypes as C
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import harness_data  # noqa: E402
from frlw_evd_amd import synth  # noqa: E402
from golden_util import LAMDAS, assert_bitexact  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def er():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from frlw_evd_amd import event_representation
    return event_representation


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def to_dev(rec):
    return torch.from_numpy(np.ascontiguousarray(rec).view(np.uint8).reshape(-1, 8).copy()).cuda()


def counts(symbol):
    from frlw_evd_amd import _lib
    c = (C.c_uint64 * 2)()
    _lib.check(getattr(_lib.load(), symbol)(c), symbol)
    return np.array(list(c), dtype=np.int64)


def chain_counts():
    return counts("frlw_encoder_chain_counts")


def batch_counts():
    return counts("frlw_encoder_batch_counts")


def single_chain(er, dat, steps, shape, memory, xm=None, ym=None):
    """The loop the chain replaces: one encode_sae_dat per step, each fed the previous one's memory.  Returns the f32 and u8
    volumes of the emitting steps and the final memory."""
    f32, u8 = [], []
    for lo, hi, now, win, emit in steps:
        f, u, memory = er.encode_sae_dat(dat[lo:hi], shape, LAMDAS, memory, now, win, want_u8=True, xmap=xm, ymap=ym)
        if emit:
            f32.append(f)
            u8.append(u)
    return f32, u8, memory


# ------------------------------------------------------------------------------------------
# Surface of Active Events, chained
# ------------------------------------------------------------------------------------------
SPAN, WIN = 1_000_000, 800_000   # a segment's events spread over SPAN, its step ends 1000 us later: the first fifth is dropped


def chain_round(seed, n_steps, sensor, maps, t_base):
    """One call's records and steps: ONE time-sorted stream cut into consecutive segments.  Segment 0 holds 12 500 records (four
    counting workgroups), one segment is empty, one holds a single record, the others 300-700.  From six steps on, steps 3, 4 and
    5 share one segment and one `now` with windows 200 000 < 800 000 < 3 000 000 and only the third emits (the test split of
    the offline command); every other step has window WIN and emits.  `now` ascends, and the last segment starts 6 000 000 us after
    the one before: its floor now - 5 000 000 overtakes everything the memory holds.  Returns (records, steps, end time)."""
    Hs, Ws = sensor
    rng = np.random.default_rng(seed)
    triple = n_steps >= 6
    n_seg = n_steps - 2 if triple else n_steps
    sizes = [12_500] + [int(rng.integers(300, 701)) for _ in range(n_seg - 1)]
    if n_seg >= 3:
        sizes[1], sizes[2] = 0, 1
    parts, ranges, nows, t0, at = [], [], [], t_base, 0
    for k, size in enumerate(sizes):
        if k == n_seg - 1 and n_seg > 1:
            t0 += 6_000_000
        ev = synth.synth_events(seed + 1 + k, size, Ws, Hs, SPAN, hotspot=bool(k & 1), t_offset=t0)
        if size > 40 and not maps:          # (the maps' tables end at the sensor: out-of-sensor coordinates would be an IndexError)
            ev["x"][::37] = Ws + 3          # outside the frame: dropped, no error
            ev["y"][5::41] = Hs + 1
            for key in ("x", "y", "p", "t"):  # the same cell twice at one timestamp: the later record is the last writer
                ev[key][21] = ev[key][20]
        parts.append(synth.to_dat8(ev))
        ranges.append((at, at + size))
        nows.append(t0 + SPAN + 1000)
        at += size
        t0 += SPAN + 1000
    steps = []
    for k in range(n_seg):
        if triple and k == 3:
            steps += [(*ranges[k], nows[k], w, w == 3_000_000) for w in (200_000, 800_000, 3_000_000)]
        else:
            steps.append((*ranges[k], nows[k], WIN, True))
    assert len(steps) == n_steps and [s[2] for s in steps] == sorted(s[2] for s in steps)
    return np.concatenate(parts), steps, t0


@pytest.mark.parametrize("n_steps,sensor,shape", [(1, (8, 12), (8, 12)), (7, (53, 91), (53, 91)), (64, (37, 70), (37, 70)),
                                                  (6, (120, 200), (60, 100))])
def test_sae_chain_equals_chained_single_calls_and_oracle(er, orc, n_steps, sensor, shape):
    H, W = shape
    maps = sensor != shape
    xm, ym = er.coordinate_maps(sensor, shape, "cuda") if maps else (None, None)
    c0, b0 = chain_counts(), batch_counts()
    mem = want_mem = omem = None
    t_base = 10_000_000
    for call in range(2):   # the second call starts from the memory the first one left
        rec, steps, t_base = chain_round(9000 + 1000 * call + n_steps, n_steps, sensor, maps, t_base)
        dat = to_dev(rec)
        n_emit = sum(1 for s in steps if s[4])
        f32, u8, mem = er.encode_sae_chain(dat, steps, shape, LAMDAS, mem, want_f32=True, want_u8=True, xmap=xm, ymap=ym)
        assert tuple(f32.shape) == (n_emit, 6, H, W) and tuple(u8.shape) == (n_emit, 6, H, W) and u8.dtype == torch.uint8
        assert tuple(mem.shape) == (2, H, W)
        want_f32, want_u8, want_mem = single_chain(er, dat, steps, shape, want_mem, xm, ym)
        assert len(want_f32) == n_emit
        for e in range(n_emit):
            assert torch.equal(f32[e], want_f32[e]), (call, e, "f32")
            assert torch.equal(u8[e], want_u8[e]), (call, e, "u8")
        assert torch.equal(mem, want_mem), (call, "memory")
        for lo, hi, now, win, _ in steps:
            _, omem = orc.sae_stream_dat8(rec[lo:hi], sensor, shape, LAMDAS, omem, now, win)
        assert_bitexact(mem.cpu().numpy(), omem, f"memory vs oracle, call {call}")
        only_u8 = er.encode_sae_chain(dat, steps, shape, LAMDAS, None, want_f32=False, want_u8=True, xmap=xm, ymap=ym)
        assert only_u8[0] is None and tuple(only_u8[1].shape) == (n_emit, 6, H, W)
    assert list(chain_counts() - c0) == [4, 0]   # two chained calls and two u8-only calls: one count per call
    assert list(batch_counts() - b0) == [0, 0]


def test_sae_chain_unsorted_stream_and_no_window(er):
    """The last writer of a cell is the last RECORD, also in a stream that is not time-sorted, and window_us <= 0 keeps every
    event -- as the single call does.  The ranges overlap."""
    H, W, n = 53, 91, 25_000
    ev = synth.synth_events(9500, n, W, H, 900_000, t_offset=1_000_000)
    perm = np.random.default_rng(3).permutation(n)
    dat = to_dev(synth.to_dat8({k: v[perm] for k, v in ev.items()}))
    steps = [(0, 9_000, 1_950_000, 600_000, True), (4_001, 16_000, 2_000_000, 0, True), (9_000, n, 2_000_500, -5, False),
             (0, n, 2_100_000, 700_000, True)]
    f32, u8, mem = er.encode_sae_chain(dat, steps[:3], (H, W), LAMDAS, None, want_u8=True)
    want_f32, want_u8, want_mem = single_chain(er, dat, steps[:3], (H, W), None)
    assert len(f32) == 2 and all(torch.equal(a, b) for a, b in zip(f32, want_f32)) and all(torch.equal(a, b) for a, b in zip(u8, want_u8))
    assert torch.equal(mem, want_mem)
    f32, u8, mem = er.encode_sae_chain(dat, steps, (H, W), LAMDAS, mem, want_u8=True)
    want_f32, want_u8, want_mem = single_chain(er, dat, steps, (H, W), want_mem)
    assert len(f32) == 3 and all(torch.equal(a, b) for a, b in zip(f32, want_f32)) and all(torch.equal(a, b) for a, b in zip(u8, want_u8))
    assert torch.equal(mem, want_mem)


def test_sae_chain_in_parts_carries_the_memory(er):
    """What the offline command does with a long file: the steps in parts of at most 64 (and, here, of 4: a part then ends between
    the three test-split steps of one label), the memory tensor carried from part to part -- equal to ONE loop of single calls."""
    from frlw_evd_amd import generate
    H, W, n, labels = 37, 70, 23_000, 23
    dat = to_dev(synth.to_dat8(synth.synth_events(9650, n, W, H, 2_300_000, t_offset=1_000_000)))
    slices = [{"start_count": k * 1_000, "end_count": (k + 1) * 1_000, "label_time": 1_000_000 + (k + 1) * 100_000} for k in range(labels)]
    steps = generate.sae_steps(slices, "test", [50_000, 150_000, 400_000])
    assert len(steps) == 3 * labels > 64
    want_f32, want_u8, want_mem = single_chain(er, dat, steps, (H, W), None)
    assert len(want_u8) == labels
    for max_steps in (64, 4):
        memory, got = None, []
        for part in generate.sae_parts(steps, max_steps):
            _, u8, memory = er.encode_sae_chain(dat, part, (H, W), LAMDAS, memory, want_f32=False, want_u8=True)
            emitting = sum(1 for s in part if s[4])
            assert (u8 is None) == (emitting == 0)
            got += [u8[e] for e in range(emitting)]
        assert len(got) == labels and all(torch.equal(a, b) for a, b in zip(got, want_u8)), max_steps
        assert torch.equal(memory, want_mem), max_steps


def test_sae_chain_steps_that_write_nothing(er):
    H, W, n = 37, 70, 6_000
    dat = to_dev(synth.to_dat8(synth.synth_events(9600, n, W, H, 900_000, t_offset=1_000_000)))
    quiet = [(0, 2_000, 1_400_000, 0, False), (2_000, 2_000, 1_500_000, 300_000, False), (1_000, n, 2_000_000, 500_000, False)]
    f32, u8, mem = er.encode_sae_chain(dat, quiet, (H, W), LAMDAS, None, want_f32=True, want_u8=True)
    assert f32 is None and u8 is None
    assert torch.equal(mem, single_chain(er, dat, quiet, (H, W), None)[2])
    # every step empty: the memory meets only the rising floors now - 5 000 000 (torch.where against a constant plane)
    empty = [(0, 0, 3_000_000, 800_000, True), (n, n, 6_500_000, 0, True), (77, 77, 7_000_000, 800_000, False),
             (5, 5, 13_000_000, 800_000, True)]
    f32, u8, new = er.encode_sae_chain(dat, empty, (H, W), LAMDAS, mem, want_u8=True)
    want_f32, want_u8, want_mem = single_chain(er, dat, empty, (H, W), mem)
    assert torch.equal(new, want_mem) and len(f32) == 3
    assert all(torch.equal(a, b) for a, b in zip(f32, want_f32)) and all(torch.equal(a, b) for a, b in zip(u8, want_u8))
    floor = torch.tensor(13_000_000.0, device="cuda") - 5_000_000.0
    assert torch.equal(new, torch.where(mem > floor, mem, floor.expand_as(mem)))   # 8 000 000 is above every event of the stream
    assert not torch.equal(new, mem)


# ------------------------------------------------------------------------------------------
# Event Volume over record ranges
# ------------------------------------------------------------------------------------------
EV_FRAMES = {"gen1": ((240, 304), (240, 304), 50_000), "gen4_maps": ((720, 1280), (512, 640), 80_000)}   # sensor, shape, window_us
EV_N = 60_000


def ev_ranges_case(B, n):
    """Ranges of a stream of n records.  64: a nested triple ending at the same record (the largest holds 25 000 records), two
    overlapping ranges (one starts at an odd record), an empty range, a single-record range and 57 sliding, overlapping ones;
    5: the triple, a range that starts at an odd record and overlaps the largest, an empty one; 1: one range of 25 000 records
    that starts at an odd record."""
    e = n - 10
    triple = [(e - 2_000, e), (e - 9_000, e), (e - 25_000, e)]
    if B == 1:
        return [(10_001, 35_001)]
    if B == 5:
        return triple + [(e - 26_001, e - 20_000), (777, 777)]
    step = n // 80
    out = triple + [(1_001, 7_001), (5_000, 12_000), (777, 777), (1_500, 1_501)] + [(i * step, i * step + 3 * step + i) for i in range(57)]
    assert len(out) == B == 64
    return out


@pytest.fixture(scope="module")
def ev_streams():
    """Per frame: the records (host) of one time-sorted stream, 60 000 events over three windows, the first one a window after
    time 0 (no window starts before 0): a range of 25 000 records spans 1.25 windows, so its front is dropped by its own t_end; the
    ranges of 9 000 records and fewer lie inside their window."""
    out = {}
    for key, (sensor, _, win) in EV_FRAMES.items():
        out[key] = synth.to_dat8(synth.synth_events(7700 + len(key), EV_N, sensor[1], sensor[0], win * 3, hotspot=True, t_offset=win + 1))
    return out


@pytest.fixture(scope="module")
def ev_reference(er, orc, ev_streams):
    """encode_ev_dat on the general path and the oracle, once per distinct (frame, lo, hi, t_end), shared by the cases."""
    seen = {}

    def get(key, lo, hi, t_end):
        k = (key, lo, hi, t_end)
        if k not in seen:
            sensor, shape, win = EV_FRAMES[key]
            rec = ev_streams[key]
            xm, ym = er.coordinate_maps(sensor, shape, "cuda") if sensor != shape else (None, None)
            want = orc.ev_stream_dat8(rec[lo:hi], sensor, shape, 5, t_end, win)
            if hi > lo:
                f, u = er.encode_ev_dat(to_dev(rec[lo:hi]), shape, t_end, win, 5, want_u8=True, xmap=xm, ymap=ym, fast=False)
                assert_bitexact(f.cpu().numpy(), want, f"single call vs oracle {k}")
            else:
                f, u = torch.zeros((10, *shape), device="cuda"), torch.zeros((10, *shape), dtype=torch.uint8, device="cuda")
                assert not want.any()
            seen[k] = (f, u, want)
        return seen[k]
    return get


@pytest.mark.parametrize("B,key", [(1, "gen1"), (5, "gen1"), (64, "gen1"), (1, "gen4_maps"), (5, "gen4_maps"), (64, "gen4_maps")])
def test_ev_ranges_equal_single_calls_and_oracle(er, ev_streams, ev_reference, B, key):
    sensor, shape, win = EV_FRAMES[key]
    H, W = shape
    rec = ev_streams[key]
    dat = to_dev(rec)
    xm, ym = er.coordinate_maps(sensor, shape, "cuda") if sensor != shape else (None, None)
    ranges = ev_ranges_case(B, len(rec))
    # every range ends at its own time: the last record's, moved on by 0..2 us (no event lies behind it)
    t_end = [int(rec["t"][hi - 1]) + b % 3 if hi > lo else 2 * win + b for b, (lo, hi) in enumerate(ranges)]
    assert len(set(t_end)) > 1 or B == 1
    lo, hi = max(ranges, key=lambda r: r[1] - r[0])
    assert int(rec["t"][lo]) <= int(rec["t"][hi - 1]) - win   # the front of the longest range lies outside its window
    if er.ev_ranges_max_windows(shape, win) < B:
        # 512 x 640 is 160 tiles: 64 windows are more (window, tile) pairs than the partition takes -- where the batch call answers
        # FRLW_ERR_UNSUPPORTED the ranged call does too (the offline command cuts its parts to ev_ranges_max_windows)
        assert key == "gen4_maps" and B == 64 and er.ev_ranges_max_windows(shape, win) == 51
        with pytest.raises(NotImplementedError):
            er.encode_ev_batch(dat, list(range(B + 1)), shape, t_end, win, 5, xmap=xm, ymap=ym)
        with pytest.raises(NotImplementedError):
            er.encode_ev_ranges(dat, ranges, shape, t_end, win, 5, xmap=xm, ymap=ym)
        return
    c0 = chain_counts()
    f32, u8 = er.encode_ev_ranges(dat, ranges, shape, t_end, win, 5, want_f32=True, want_u8=True, xmap=xm, ymap=ym)
    assert list(chain_counts() - c0) == [0, 1]
    assert tuple(f32.shape) == (B, 10, H, W) and tuple(u8.shape) == (B, 10, H, W) and u8.dtype == torch.uint8
    assert max(hi - lo for lo, hi in ranges) >= 20_000 and any(lo & 1 for lo, _ in ranges)
    for b, (lo, hi) in enumerate(ranges):
        f, u, want = ev_reference(key, lo, hi, t_end[b])
        assert torch.equal(f32[b], f), (b, lo, hi, "f32")
        assert torch.equal(u8[b], u), (b, lo, hi, "u8")
        assert_bitexact(f32[b].cpu().numpy(), want, f"range {b} ({lo}, {hi}) vs oracle")
    only_u8 = er.encode_ev_ranges(dat, ranges, shape, t_end, win, 5, want_f32=False, want_u8=True, xmap=xm, ymap=ym)
    assert only_u8[0] is None and torch.equal(only_u8[1], u8)


def test_ev_ranges_event_behind_its_window_end(er, ev_streams):
    sensor, shape, win = EV_FRAMES["gen1"]
    rec = ev_streams["gen1"]
    dat = to_dev(rec)
    ranges = [(0, 1_000), (2_001, 4_000)]
    good = [int(rec["t"][999]), int(rec["t"][3_999])]
    late = [good[0], int(rec["t"][3_000]) - 1]   # records 3 000 .. 3 999 of the second range lie behind its end
    assert int(rec["t"][3_999]) > late[1]
    with pytest.raises(ValueError):
        er.encode_ev_ranges(dat, ranges, shape, late, win, 5)
    er.encode_ev_ranges(dat, ranges, shape, late, win, 5, check=False)
    with pytest.raises(ValueError):
        er.raise_deferred()
    er.raise_deferred()   # read and cleared
    f32, _ = er.encode_ev_ranges(dat, ranges, shape, good, win, 5)
    for b, (lo, hi) in enumerate(ranges):
        assert torch.equal(f32[b], er.encode_ev_dat(dat[lo:hi], shape, good[b], win, 5, fast=False)[0])
    with pytest.raises(NotImplementedError):   # window beyond the 20 bits of the 4-byte record
        er.encode_ev_ranges(dat, ranges, shape, good, 2_000_000, 5)


# ------------------------------------------------------------------------------------------
# errors
# ------------------------------------------------------------------------------------------
def test_errors(er):
    H, W, n = 53, 91, 5_000
    dat = to_dev(synth.to_dat8(synth.synth_events(9800, n, W, H, 50_000, t_offset=1)))
    step = (0, 100, 60_000, 40_000, True)
    for steps in ([], [step] * 65, [(0, n + 1, 60_000, 40_000, True)], [(500, 400, 60_000, 40_000, True)], [(0, 100, 60_000, 40_000)],
                  [(0, 100, 60_000, 40_000, True, 0)]):
        with pytest.raises(ValueError):
            er.encode_sae_chain(dat, steps, (H, W), LAMDAS, None)
    with pytest.raises(ValueError):
        er.encode_sae_chain(dat, [step], (H, W), [1e-6] * 9, None)
    for ranges in ([], [(0, 10)] * 65, [(0, n + 1)], [(500, 400)]):
        with pytest.raises(ValueError):
            er.encode_ev_ranges(dat, ranges, (H, W), 60_000, 50_000)
    # the calls still work afterwards
    f32, _, mem = er.encode_sae_chain(dat, [step] * 64, (H, W), LAMDAS, None)
    assert tuple(f32.shape) == (64, 6, H, W) and torch.equal(f32[0], f32[63])   # the same step again leaves the same memory
    assert torch.equal(mem, er.encode_sae_dat(dat[0:100], (H, W), LAMDAS, None, 60_000, 40_000)[2])


# ------------------------------------------------------------------------------------------
# stream capture
# ------------------------------------------------------------------------------------------
def test_both_calls_replay_in_a_captured_graph(er):
    H, W, n, win = 53, 91, 24_000, 700_000
    recs = [synth.to_dat8(synth.synth_events(9700 + k, n, W, H, 900_000, hotspot=bool(k), t_offset=1_000_000)) for k in range(3)]
    steps = [(0, 7_000, 1_800_000, win, True), (7_000, 7_000, 1_900_000, win, False), (5_001, n, 2_000_000, 0, True)]
    ranges, t_end = [(0, n), (n // 2 + 1, n), (100, 100), (5_000, 17_000)], [1_900_000, 1_900_001, 1_900_002, 1_900_003]
    static = to_dev(recs[0])
    memory = torch.full((2, H, W), 1_234_567.0, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        # the workspaces of this stream (and the one-time self-test behind the Event Volume path) exist before the capture
        er.encode_sae_chain(static, steps, (H, W), LAMDAS, memory, want_u8=True, check=False)
        er.encode_ev_ranges(static, ranges, (H, W), t_end, win, 5, want_u8=True, check=False)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            g_f32, g_u8, g_mem = er.encode_sae_chain(static, steps, (H, W), LAMDAS, memory, want_u8=True, check=False)
            g_ev, g_ev8 = er.encode_ev_ranges(static, ranges, (H, W), t_end, win, 5, want_u8=True, check=False)
        for k in (1, 2):
            static.copy_(to_dev(recs[k]))
            graph.replay()
            side.synchronize()
            got = [t.clone() for t in (g_f32, g_u8, g_mem, g_ev, g_ev8)]
            e_f32, e_u8, e_mem = er.encode_sae_chain(static, steps, (H, W), LAMDAS, memory, want_u8=True)
            e_ev, e_ev8 = er.encode_ev_ranges(static, ranges, (H, W), t_end, win, 5, want_u8=True)
            for a, b, what in zip(got, (e_f32, e_u8, e_mem, e_ev, e_ev8), ("sae f32", "sae u8", "sae memory", "ev f32", "ev u8")):
                assert torch.equal(a, b), (k, what)
            assert torch.equal(e_ev[3], er.encode_ev_dat(static[5_000:17_000], (H, W), t_end[3], win, 5, fast=False)[0]), k
        er.raise_deferred()
    torch.cuda.current_stream().wait_stream(side)


# ------------------------------------------------------------------------------------------
# the offline commands
# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return harness_data.build(str(tmp_path_factory.mktemp("label_batches_gpu")))


def test_surfaceofactiveevents_command_writes_the_single_call_files(er, dataset, tmp_path):
    from frlw_evd_amd import dat_io, generate
    raw, lab = dataset
    target = str(tmp_path / "sae")
    lamdas, time_window = [0.00001, 0.0000025, 0.000001], [554126, 2216505, 5541263]
    c0 = chain_counts()
    n_files = generate.generate_surfaceofactiveevents(raw, lab, target, "gen1")
    moved = chain_counts() - c0
    _, tgt, enc, xmap, ymap = generate._geometry("gen1", "cuda")
    seen = calls = 0
    for mode, name, event_file, bbox_file in generate._sequences(raw, lab):
        f_event = dat_io.DatFile(event_file)
        dat = f_event.to_device(device="cuda")
        memory, n_steps = None, 0
        for sl in dat_io.sae_label_slices(f_event, generate.read_label_times(bbox_file)):
            rec = dat[sl["start_count"]:sl["end_count"]]
            u8 = None
            for tw in (time_window if mode == "test" else [max(time_window)]):
                _, u8, memory = er.encode_sae_dat(rec, enc, lamdas, memory, sl["label_time"], tw, want_f32=False, want_u8=True,
                                                  xmap=xmap, ymap=ymap)
                n_steps += 1
            vol = u8.view(len(lamdas), 2, enc[0], enc[1])
            for j, lam in enumerate(lamdas):
                want = er.resize_nearest(vol[j], tgt).cpu().numpy().tobytes()
                path = os.path.join(target, f"SurfaceOfActiveEvents{lam}", mode, f"{name}_{sl['label_time']}.npy")
                assert open(path, "rb").read() == want, path
                seen += 1
        steps = generate.sae_steps(dat_io.sae_label_slices(dat_io.DatFile(event_file), generate.read_label_times(bbox_file)), mode)
        assert len(steps) == n_steps
        calls += len(generate.sae_parts(steps))
    assert seen == n_files == sum(len(fs) for _, _, fs in os.walk(target)) and seen > 0
    assert list(moved) == [calls, 0] and calls > 0


def test_eventvolume_command_writes_the_single_call_files(er, dataset, tmp_path):
    from frlw_evd_amd import dat_io, generate
    raw, lab = dataset
    target = str(tmp_path / "ev")
    time_windows, bins = [250000, 500000, 1000000], 5
    c0 = chain_counts()
    n_files = generate.generate_eventvolume(raw, lab, target, "gen1")
    moved = chain_counts() - c0
    _, tgt, enc, xmap, ymap = generate._geometry("gen1", "cuda")
    seen = calls = 0
    for mode, name, event_file, bbox_file in generate._sequences(raw, lab):
        f_event = dat_io.DatFile(event_file)
        dat = f_event.to_device(device="cuda")
        slices = list(dat_io.ev_label_slices(f_event, generate.read_label_times(bbox_file), time_windows))
        for sl in slices:
            rec = dat[sl["start_count"]:sl["end_count"]]
            for tw in time_windows:
                _, u8 = er.encode_ev_dat(rec, enc, sl["end_time"], tw, bins, want_f32=False, want_u8=True, xmap=xmap, ymap=ymap)
                want = er.resize_nearest(u8, tgt).cpu().numpy().tobytes()
                path = os.path.join(target, f"EventVolume{tw}", mode, f"{name}_{sl['label_time']}.npy")
                assert open(path, "rb").read() == want, path
                seen += 1
        for tw in time_windows:
            jobs = generate.ev_jobs(slices, tw, os.path.join(target, f"EventVolume{tw}", mode, name), f_event._t)
            calls += len(generate.ev_parts(jobs, er.ev_ranges_max_windows(enc, tw)))
    assert seen == n_files == sum(len(fs) for _, _, fs in os.walk(target)) and seen > 0
    assert list(moved) == [0, calls] and calls > 0
