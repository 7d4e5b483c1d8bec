"""Batched Event Count Image / Surface of Active Events (frlw_eci_encode_batch, frlw_sae_encode_batch) on the GPU: every
comparison is bit-equal -- against the single-window calls (encode_eci_dat / encode_sae_dat) on the same record ranges, and
against the CPU oracle as tests/test_encoders_gpu.py calls it."""
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
    return torch.from_numpy(rec.view(np.uint8).reshape(-1, 8).copy()).cuda()


def batch_counts():
    from frlw_evd_amd import _lib
    c = (C.c_uint64 * 2)()
    _lib.check(_lib.load().frlw_encoder_batch_counts(c), "frlw_encoder_batch_counts")
    return np.array(list(c), dtype=np.int64)


def eci_value(n):
    """n sequential f32 adds of 0.05, clamped at 1, times 255 (generate_eventcountimage.py:32-34,41)."""
    acc = np.float32(0)
    for _ in range(n):
        acc = np.float32(acc + np.float32(0.05))
    return np.float32(min(acc, np.float32(1)) * np.float32(255))


# ------------------------------------------------------------------------------------------
# Event Count Image
# ------------------------------------------------------------------------------------------
FRAMES = {"8x12": ((8, 12), (8, 12), 30_000), "53x91": ((53, 91), (53, 91), 30_000), "240x304": ((240, 304), (240, 304), 120_000),
          "gen4": ((720, 1280), (512, 640), 120_000)}   # sensor, encode shape, events
SAT = ((2, 1, 19), (4, 1, 20), (6, 1, 21))   # target pixel (x, y) and how many events of polarity 1 it gets inside SAT_RANGE


def eci_stream(key):
    """A stream whose records [1000, 2000) hold three pixels with exactly 19 / 20 / 21 events of polarity 1 (nothing else of the
    stream lands on them), and events on the first and last row and column."""
    sensor, shape, n = FRAMES[key]
    (Hs, Ws), (H, W) = sensor, shape
    ev = synth.synth_events(8100 + n + H, n, Ws, Hs, 60_000, hotspot=True)
    xm = (np.arange(Ws, dtype=np.float64) * (W / Ws)).astype(np.int64)
    ym = (np.arange(Hs, dtype=np.float64) * (H / Hs)).astype(np.int64)
    for tx, ty, _ in SAT:   # clear the three pixels
        hit = (xm[ev["x"]] == tx) & (ym[ev["y"]] == ty)
        ev["x"][hit] = int(np.flatnonzero(xm == 0)[0])
    at = 1000
    for tx, ty, k in SAT:
        ev["x"][at:at + k] = int(np.flatnonzero(xm == tx)[0])
        ev["y"][at:at + k] = int(np.flatnonzero(ym == ty)[-1])
        ev["p"][at:at + k] = 1
        at += k + 7
    for j, (x, y) in enumerate(((0, 0), (Ws - 1, 0), (0, Hs - 1), (Ws - 1, Hs - 1))):
        ev["x"][1500 + j], ev["y"][1500 + j] = x, y
    return synth.to_dat8(ev)


def eci_ranges(n):
    nested = [(n - n // 8, n), (n - n // 4, n), (n - n // 2, n)]   # the command's three windows per label
    step = n // 80
    return {
        "single": [(0, n)],
        "mixed": nested + [(777, 777), (1500, 1501), (1000, 2000), (0, 1), (n - 1, n), (n, n)],
        "overlap64": [(i * step, i * step + 3 * step + i) for i in range(64)],
    }


@pytest.mark.parametrize("key", list(FRAMES))
def test_eci_batch_equals_single_calls_and_oracle(er, orc, key):
    sensor, shape, n = FRAMES[key]
    H, W = shape
    rec = eci_stream(key)
    dat = to_dev(rec)
    xm = ym = None
    if sensor != shape:
        xm, ym = er.coordinate_maps(sensor, shape, "cuda")
    want = {}   # one reference per distinct range, shared by the three calls

    def reference(lo, hi):
        if (lo, hi) not in want:
            f, u = er.encode_eci_dat(dat[lo:hi], shape, want_u8=True, xmap=xm, ymap=ym)
            assert_bitexact(f.cpu().numpy(), orc.eci_stream_dat8(rec[lo:hi], sensor, shape), f"single call vs oracle {lo}:{hi}")
            want[(lo, hi)] = (f, u)
        return want[(lo, hi)]

    for name, ranges in eci_ranges(n).items():
        c0 = batch_counts()
        f32, u8 = er.encode_eci_batch(dat, ranges, shape, want_f32=True, want_u8=True, xmap=xm, ymap=ym)
        assert list(batch_counts() - c0) == [1, 0], name
        assert tuple(f32.shape) == (len(ranges), 2, H, W) and u8.dtype == torch.uint8 and tuple(u8.shape) == tuple(f32.shape)
        for b, (lo, hi) in enumerate(ranges):
            f, u = reference(lo, hi)
            assert torch.equal(f32[b], f), (name, b, lo, hi)
            assert torch.equal(u8[b], u), (name, b, lo, hi)
        only_u8 = er.encode_eci_batch(dat, ranges, shape, want_f32=False, want_u8=True, xmap=xm, ymap=ym)
        assert only_u8[0] is None and torch.equal(only_u8[1], u8), name
        if name == "mixed":
            assert not f32[3].any() and not f32[8].any()          # empty ranges
            assert int((f32[4] != 0).sum()) == 1                   # one event
            sat = f32[5]                                           # the saturation edge: 19, 20 and 21 events of one polarity
            for tx, ty, k in SAT:
                assert sat[1, ty, tx].item() == eci_value(k), (tx, ty, k)
                assert sat[0, ty, tx].item() == 0.0
            assert eci_value(19) < 255.0 and eci_value(20) == 255.0 and eci_value(21) == 255.0


def test_eci_counter_neither_wraps_nor_saturates_early(er, orc):
    """A pixel with 70 000 events, one with 65 540 (a 16-bit counter would read 4: below the saturation) and one with 19 events
    spread over the whole stream (a skip-when-saturated shortcut must not skip it), in windows that hold all or part of them."""
    H, W = 53, 91
    n = 70_000 + 65_540 + 19 + 4_441
    rng = np.random.default_rng(5)
    ev = synth.synth_events(8200, n, W - 3, H, 60_000)   # background: columns 0 .. W - 4
    order = rng.permutation(n)
    a, b, c = order[:70_000], order[70_000:135_540], order[135_540:135_559]
    for idx, x, p in ((a, W - 1, 1), (b, W - 2, 0), (c, W - 3, 1)):
        ev["x"][idx], ev["y"][idx], ev["p"][idx] = x, 7, p
    rec = synth.to_dat8(ev)
    dat = to_dev(rec)
    ranges = [(0, n), (n // 2, n), (0, n // 3), (0, 4096), (n - 50, n)]
    f32, u8 = er.encode_eci_batch(dat, ranges, (H, W), want_u8=True)
    for i, (lo, hi) in enumerate(ranges):
        f, u = er.encode_eci_dat(dat[lo:hi], (H, W), want_u8=True)
        assert torch.equal(f32[i], f) and torch.equal(u8[i], u), (lo, hi)
        assert_bitexact(f32[i].cpu().numpy(), orc.eci_stream_dat8(rec[lo:hi], (H, W), (H, W)), f"oracle {lo}:{hi}")
    assert f32[0, 1, 7, W - 1].item() == 255.0 and f32[0, 0, 7, W - 2].item() == 255.0
    assert f32[0, 1, 7, W - 3].item() == eci_value(19)


def test_eci_batch_errors(er):
    H, W, n = 53, 91, 20_000
    rec = synth.to_dat8(synth.synth_events(8300, n, W, H, 50_000))
    dat = to_dev(rec)
    with pytest.raises(ValueError):
        er.encode_eci_batch(dat, [(0, 10)] * 65, (H, W))
    with pytest.raises(ValueError):
        er.encode_eci_batch(dat, [(0, 10), (500, 400)], (H, W))
    bad = rec.copy()
    bad["_"][9000] = (np.uint32(W - 1) & 16383) | (np.uint32(H + 5) << 14)   # flat index behind the frame
    datb = to_dev(bad)
    ranges = [(0, 5000), (8000, 12_000), (15_000, n)]
    with pytest.raises(IndexError):
        er.encode_eci_batch(datb, ranges, (H, W))
    er.encode_eci_batch(datb, ranges, (H, W), check=False)
    with pytest.raises(IndexError):
        er.raise_deferred()
    er.raise_deferred()   # read and cleared
    f32, _ = er.encode_eci_batch(datb, [(0, 5000), (15_000, n)], (H, W))   # ranges that leave the bad record out: a clean call
    for i, (lo, hi) in enumerate(((0, 5000), (15_000, n))):
        assert torch.equal(f32[i], er.encode_eci_dat(dat[lo:hi], (H, W))[0])
    f32, _ = er.encode_eci_batch(dat, ranges, (H, W))
    for i, (lo, hi) in enumerate(ranges):
        assert torch.equal(f32[i], er.encode_eci_dat(dat[lo:hi], (H, W))[0])


# ------------------------------------------------------------------------------------------
# Surface of Active Events
# ------------------------------------------------------------------------------------------
def sae_round(seed, B, sensor, sizes, t_lo, span):
    """One call's records: sequence s holds sizes[s] time-sorted events of [t_lo, t_lo + span]; some lie outside the frame
    (dropped, no error), and two events of one cell share their timestamp."""
    Hs, Ws = sensor
    parts, offs = [], [0]
    for s in range(B):
        ev = synth.synth_events(seed + s, sizes[s], Ws, Hs, span, hotspot=bool(s & 1), t_offset=t_lo)
        if sizes[s] > 40:
            ev["x"][::37] = Ws + 3          # only reachable without maps (the maps' tables end at the sensor)
            ev["y"][5::41] = Hs + 1
            for k in ("x", "y", "p", "t"):  # the same cell twice at one timestamp: the later record is the last writer
                ev[k][21] = ev[k][20]
        parts.append(synth.to_dat8(ev))
        offs.append(offs[-1] + sizes[s])
    return np.concatenate(parts), offs


@pytest.mark.parametrize("B,sensor,shape", [(1, (240, 304), (240, 304)), (5, (53, 91), (53, 91)), (64, (37, 70), (37, 70)),
                                            (3, (120, 200), (60, 100))])
def test_sae_batch_three_calls_equal_single_calls_and_oracle(er, orc, B, sensor, shape):
    H, W = shape
    maps = sensor != shape
    xm, ym = er.coordinate_maps(sensor, shape, "cuda") if maps else (None, None)
    rng = np.random.default_rng(B)
    span, win = 1_000_000, 800_000   # the first fifth of a call's events lies at or in front of now - window: dropped
    mem = None
    omem = [None] * B
    c0 = batch_counts()
    for call in range(3):
        # the first call is dense, the later ones sparse: most cells are then hit only in an earlier call
        sizes = [int(rng.integers(5_000, 30_000)) if call == 0 else int(rng.integers(1, 700)) for _ in range(B)]
        if B > 1:
            sizes[1] = 0    # an empty sequence: its memory passes through by the single call's rule (the floor may rise)
            sizes[B - 1] = 9_000
        t_lo = 10_000_000 + call * span
        rec, offs = sae_round(9000 + 100 * call, B, sensor, sizes, t_lo, span)
        if maps:   # (the coordinate maps end at the sensor: out-of-sensor coordinates would be an IndexError)
            w = rec["_"].astype(np.int64)
            x, y = np.minimum(w & 16383, sensor[1] - 1), np.minimum((w >> 14) & 16383, sensor[0] - 1)
            rec["_"] = ((w & (1 << 28)) | (y << 14) | x).astype(np.uint32)
        dat = to_dev(rec)
        now = [t_lo + span + 1000 * s for s in range(B)]   # differs per sequence
        f32, u8, new = er.encode_sae_batch(dat, offs, shape, LAMDAS, mem, now, win, want_u8=True, xmap=xm, ymap=ym)
        assert tuple(f32.shape) == (B, 6, H, W) and tuple(u8.shape) == (B, 6, H, W) and tuple(new.shape) == (B, 2, H, W)
        for s in range(B):
            sl = dat[offs[s]:offs[s + 1]]
            f1, u1, m1 = er.encode_sae_dat(sl, shape, LAMDAS, None if mem is None else mem[s], now[s], win, want_u8=True,
                                           xmap=xm, ymap=ym)
            assert torch.equal(new[s], m1), (call, s, "memory")
            assert torch.equal(f32[s], f1), (call, s, "f32")
            assert torch.equal(u8[s], u1), (call, s, "u8")
            _, omem[s] = orc.sae_stream_dat8(rec[offs[s]:offs[s + 1]], sensor, shape, LAMDAS, omem[s], now[s], win)
            assert_bitexact(new[s].cpu().numpy(), omem[s], f"memory vs oracle, call {call} sequence {s}")
        mem = new
    assert list(batch_counts() - c0) == [0, 3]
    with pytest.raises(ValueError):
        er.encode_sae_batch(dat, list(range(66)), shape, LAMDAS, None, 0, win)


def test_sae_batch_unsorted_stream_and_no_window(er):
    """The last writer of a cell is the last RECORD, also in a stream that is not time-sorted, and window_us <= 0 keeps every
    event -- as the single call does."""
    H, W, n = 53, 91, 25_000
    ev = synth.synth_events(9500, n, W, H, 900_000, t_offset=1_000_000)
    perm = np.random.default_rng(3).permutation(n)
    rec = synth.to_dat8({k: v[perm] for k, v in ev.items()})
    dat = to_dev(rec)
    offs = [0, 9_000, 9_000, n]
    for win in (600_000, 0):
        f32, u8, mem = er.encode_sae_batch(dat, offs, (H, W), LAMDAS, None, 2_000_000, win, want_u8=True)
        for s in range(3):
            f1, u1, m1 = er.encode_sae_dat(dat[offs[s]:offs[s + 1]], (H, W), LAMDAS, None, 2_000_000, win, want_u8=True)
            assert torch.equal(mem[s], m1) and torch.equal(f32[s], f1) and torch.equal(u8[s], u1), (win, s)


# ------------------------------------------------------------------------------------------
# stream capture
# ------------------------------------------------------------------------------------------
def test_both_batched_calls_replay_in_a_captured_graph(er):
    H, W, n = 53, 91, 24_000
    recs = [synth.to_dat8(synth.synth_events(9700 + k, n, W, H, 900_000, hotspot=bool(k), t_offset=1_000_000)) for k in range(3)]
    ranges = [(0, n), (n // 2, n), (100, 100), (5_000, 17_000)]
    offs, now, win = [0, 7_000, 7_000, n], [2_000_000, 2_100_000, 2_200_000], 700_000
    static = to_dev(recs[0])
    memory = torch.full((3, 2, H, W), 1_234_567.0, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        er.encode_eci_batch(static, ranges, (H, W), check=False)            # the workspaces of this stream exist before the capture
        er.encode_sae_batch(static, offs, (H, W), LAMDAS, memory, now, win, check=False)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            g_eci, _ = er.encode_eci_batch(static, ranges, (H, W), check=False)
            g_f32, g_u8, g_mem = er.encode_sae_batch(static, offs, (H, W), LAMDAS, memory, now, win, want_u8=True, check=False)
        for k in (1, 2):
            static.copy_(to_dev(recs[k]))
            graph.replay()
            side.synchronize()
            got = [t.clone() for t in (g_eci, g_f32, g_u8, g_mem)]
            e_eci, _ = er.encode_eci_batch(static, ranges, (H, W))
            e_f32, e_u8, e_mem = er.encode_sae_batch(static, offs, (H, W), LAMDAS, memory, now, win, want_u8=True)
            for a, b, what in zip(got, (e_eci, e_f32, e_u8, e_mem), ("eci", "sae f32", "sae u8", "sae memory")):
                assert torch.equal(a, b), (k, what)
        er.raise_deferred()
    torch.cuda.current_stream().wait_stream(side)


# ------------------------------------------------------------------------------------------
# the offline command
# ------------------------------------------------------------------------------------------
def test_eventcountimage_command_writes_the_single_call_files(er, tmp_path):
    from frlw_evd_amd import dat_io, generate
    raw, lab = harness_data.build(str(tmp_path / "data"))
    target = str(tmp_path / "eci")
    windows = [50000, 100000, 200000]
    c0 = batch_counts()
    n_files = generate.generate_eventcountimage(raw, lab, target, "gen1")
    moved = int((batch_counts() - c0)[0])
    _, tgt, enc, xmap, ymap = generate._geometry("gen1", "cuda")
    seen, calls = 0, 0
    for mode, name, event_file, bbox_file in generate._sequences(raw, lab):
        f_event = dat_io.DatFile(event_file)
        dat = f_event.to_device(device="cuda")
        ranges = 0
        for sl in dat_io.eci_label_slices(f_event, generate.read_label_times(bbox_file), windows):
            for n in windows:
                lo = max(sl["tail_start"], sl["end_count"] - n)
                _, u8 = er.encode_eci_dat(dat[lo:sl["end_count"]], enc, want_f32=False, want_u8=True, xmap=xmap, ymap=ymap)
                want = er.resize_nearest(u8, tgt).cpu().numpy().tobytes()
                path = os.path.join(target, f"EventCountImage{n}", mode, f"{name}_{sl['label_time']}.npy")
                assert open(path, "rb").read() == want, path
                seen += 1
                ranges += 1
        calls += -(-ranges // 64)
    assert seen == n_files == sum(len(fs) for _, _, fs in os.walk(target)) and seen > 0
    assert moved == calls
