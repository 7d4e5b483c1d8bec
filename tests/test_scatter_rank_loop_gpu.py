"""kf_scatter_cm's rank loop: the all-valid fast block of the 20-batch form next to the block it leaves for every other batch.

A batch of 64 events takes the fast block when it is full and every lane lies inside the frame and strictly inside the span
(csrc/taf_partition.h, FASTBLK); the call must allow it (FastGeom::m24: window_us > 256; at most 32 windows; t_start + span
below 2^32).  Everything here is the CPU oracle, bit for bit, on streams built so that batches fall on both sides of each of
those conditions.  Every case runs twice: with `batches_per_wave=20`, so that a small call takes the 20-batch instance (chunks of
20 480 events, 1280 per wavefront), and with the plan's own choice (8 batches: chunks of 8192 events, 512 per wavefront).

The issue's pair of configurations with `n_windows * window_us` just below and just above 2^24 does not exist: a record word
holds 12 cell bits, the window and the in-window time in 32 bits, so every call the fast path accepts has a span below 2^20
(test_no_supported_span_reaches_2_24 pins that).  The two multiply forms of the window division are met by window_us = 256
(win_magic = 2^24: the 32-bit form) and 257 (the 24-bit form) instead.
Frames of 3 to 9 tiles (256 x 8 pixels each), at most about 60 000 events per case."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from frlw_evd_amd import synth  # noqa: E402
from golden_util import assert_bitexact, assert_u8_budget  # noqa: E402

pytestmark = pytest.mark.gpu

W = 250
GEOMS = ((1280, 20480), (512, 8192))  # (events per wavefront, events per chunk) of the two forms


def frame(tiles):
    return 8 * tiles - 3, W


def events(n, tiles, seed, t_lo, t_hi, times=None):
    """n valid events, time-sorted, in [t_lo, t_hi) (or drawn from `times`)"""
    H, _ = frame(tiles)
    rng = np.random.default_rng(seed)
    t = np.sort(rng.integers(t_lo, t_hi, n) if times is None else rng.choice(np.asarray(times, dtype=np.int64), n))
    return {"x": rng.integers(0, W, n), "y": rng.integers(0, H, n), "p": rng.integers(0, 2, n), "t": t.astype(np.int64)}


def to_dev(recs):
    return torch.from_numpy(np.ascontiguousarray(np.concatenate(recs)).view(np.uint8).reshape(-1, 8).copy()).cuda()


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


def tunings(**more):
    from frlw_evd_amd import _lib
    return (("20 batches", _lib.FrlwTuning(chunk_major=1, direct_bins=0, batches_per_wave=20, **more)),
            ("plan's batches", _lib.FrlwTuning(chunk_major=1, direct_bins=0, **more)))


def check(er, orc, monkeypatch, what, tiles, recs, t_starts, K, n_win, win, tus=None):
    H, Wd = frame(tiles)
    B = len(recs)
    assert 3 <= tiles <= 9 and sum(len(r) for r in recs) <= 62_000, sum(len(r) for r in recs)
    state0 = np.random.default_rng(17).uniform(-50, 0, (B, H, Wd, 2, K)).astype(np.float32)
    want = []
    for j, r in enumerate(recs):  # (the oracle raises on an event it cannot encode)
        view, st = orc.taf_stream_dat8(r, (H, Wd), (H, Wd), K, t_starts[j], win, n_win, state0[j])
        u8 = orc.quantize_u8(orc.leaky_transform(view.reshape(K, 2, H, Wd)))
        want.append((view, st, np.ascontiguousarray(u8[::-1])))
    dat = to_dev(recs)
    offs = np.concatenate([[0], np.cumsum([len(r) for r in recs])])
    for tname, tu in tus or tunings():
        monkeypatch.setattr(er, "TUNING", tu)
        st = torch.from_numpy(state0).cuda()
        u8, view = er.encode_taf_batch(dat, offs, (H, Wd), st, list(t_starts), win, n_win, K, want_view=True)
        for j in range(B):
            w = f"{what}, {tname}, sequence {j} ({len(recs[j])} events)"
            assert_bitexact(st[j].cpu().numpy(), want[j][1], "state, " + w)
            assert_bitexact(view[j].cpu().numpy(), want[j][0], "view, " + w)
            assert_u8_budget(u8[j].cpu().numpy(), want[j][2], 1e-4, "uint8, " + w)


# ---- 1. run lengths at the fast / slow boundary -----------------------------------------------------------------------------
def lengths_tails():  # the third wavefront of a chunk gets a run of 64 k, 64 k + 1, 64 k + 63, 1 and 0 events
    return [2 * run + tail for run, _ in GEOMS for tail in (192, 193, 255, 1, 0)]


def lengths_last_chunk_few():  # a last chunk of 5 events: 15 (and more) wavefronts without any
    return [chunk + 5 for _, chunk in GEOMS]


RUN_LENGTHS = {"tails": lengths_tails(), "last_chunk_few": lengths_last_chunk_few(),
               "one_chunk_20": [20479, 20480, 20481], "one_chunk_8": [8191, 8192, 8193]}


@pytest.mark.parametrize("name", sorted(RUN_LENGTHS))
def test_run_lengths_vs_oracle(er, orc, monkeypatch, name):
    tiles = 5
    recs = [synth.to_dat8(events(n, tiles, 100 + j, 0, 80_000)) for j, n in enumerate(RUN_LENGTHS[name])]
    check(er, orc, monkeypatch, name, tiles, recs, [0] * len(recs), 8, 8, 10_000)


# ---- 2. one invalid or edge event inside an otherwise valid stream ---------------------------------------------------------
N_EDGE = 2 * 1280 + 100  # 20-batch form: two full runs, then a run of one full batch and a partial one of 36 events
# lane 0 and lane 63 of the first batch and of the last full batch of a run; lane 0 / lane 63 of the third run's full batch; the
# first and the last lane of the partial batch
POSITIONS = (0, 63, 19 * 64, 19 * 64 + 63, 2560, 2560 + 63, 2560 + 64, N_EDGE - 1)
T0, WIN, NWIN = 50_000, 10_000, 8


def edge_stream(tiles, pos, kind, seed):
    H, _ = frame(tiles)
    ev = events(N_EDGE, tiles, seed, T0, T0 + NWIN * WIN)
    if kind == "alias":      # x >= W, flat index still inside the frame: the pixel (x - W, y + 1)
        ev["x"][pos], ev["y"][pos] = W + 7, H - 2
    elif kind == "outside":  # flat index outside the frame
        ev["x"][pos], ev["y"][pos] = 3, H
    elif kind == "t_end":    # the end of the last window: valid, r == window_us
        ev["t"][pos] = T0 + NWIN * WIN
    elif kind == "t_late":
        ev["t"][pos] = T0 + NWIN * WIN + 1
    elif kind == "t_early":
        ev["t"][pos] = T0 - 1
    return synth.to_dat8(ev)


@pytest.mark.parametrize("kind", ["alias", "t_end"])
def test_valid_edge_event_vs_oracle(er, orc, monkeypatch, kind):
    tiles = 4
    recs = [edge_stream(tiles, pos, kind, 200 + j) for j, pos in enumerate(POSITIONS)]
    check(er, orc, monkeypatch, kind, tiles, recs, [T0] * len(recs), 8, NWIN, WIN)


@pytest.mark.parametrize("kind,error", [("outside", IndexError), ("t_late", ValueError), ("t_early", ValueError)])
def test_violation_raises_and_writes_nothing(er, monkeypatch, kind, error):
    from frlw_evd_amd import _lib
    tiles, K = 4, 8
    H, Wd = frame(tiles)
    lib = _lib.load()
    for tname, tu in tunings():
        monkeypatch.setattr(er, "TUNING", tu)
        for j, pos in enumerate(POSITIONS):
            dat = to_dev([edge_stream(tiles, pos, kind, 300 + j)])
            st = torch.full((1, H, Wd, 2, K), -7.25, device="cuda")
            u8 = torch.full((1, K, 2, H, Wd), 0xA5, dtype=torch.uint8, device="cuda")
            view = torch.full((1, 2 * K, H, Wd), 3.5, device="cuda")
            # encode_taf_batch's own call, with output buffers this test can see afterwards
            d, desc = er._events_dat(dat, None, None)
            ws = er._batch_workspace(N_EDGE, 1, H, Wd, WIN, d.device)
            rc = lib.frlw_taf_encode_batch(C.byref(desc), (C.c_int64 * 2)(0, N_EDGE), (C.c_int64 * 1)(T0), 1, H, Wd, K, WIN, NWIN,
                                           er._ptr(st), er._ptr(view), er._ptr(u8), _lib.TAF_U8_FLIP_K, er._ptr(ws), ws.numel(), er._stream())
            _lib.check(rc, "frlw_taf_encode_batch")
            with pytest.raises(error):
                er._finish(ws, f"{kind} at {pos}, {tname}")
            w = f"{kind} at event {pos}, {tname}"
            assert bool((st == -7.25).all()), "state written, " + w
            assert bool((u8 == 0xA5).all()), "uint8 output written, " + w
            assert bool((view == 3.5).all()), "view written, " + w


# ---- 3. window arithmetic --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win", [2, 255, 256, 257, 10_000])
def test_window_boundaries_vs_oracle(er, orc, monkeypatch, win):
    tiles, n_win, t0 = 3, 8, 1_000
    edges = [t0 + k * win - 1 for k in range(1, n_win + 1)] + [t0 + k * win for k in range(0, n_win + 1)]
    recs = [synth.to_dat8(events(1280 + 200, tiles, 400 + win, 0, 0, times=edges)),  # t_end among them: those batches go the slow way
            synth.to_dat8(events(1280 + 200, tiles, 401 + win, 0, 0, times=edges[:-1]))]  # without it: full batches go the fast way
    check(er, orc, monkeypatch, f"window_us={win}", tiles, recs, [t0, t0], 8, n_win, win)


def test_no_supported_span_reaches_2_24(er, monkeypatch):
    tiles, K = 3, 8
    H, Wd = frame(tiles)
    for n_win, win in ((8, (1 << 21) - 1), (8, 1 << 21)):  # spans 2^24 - 8 and 2^24
        rec = synth.to_dat8(events(2000, tiles, 5, 0, n_win * win))
        for _, tu in tunings():
            monkeypatch.setattr(er, "TUNING", tu)
            with pytest.raises(NotImplementedError):
                er.encode_taf_batch(to_dev([rec]), [0, len(rec)], (H, Wd), torch.zeros((1, H, Wd, 2, K), device="cuda"), 0, win, n_win, K)


# ---- 4. window counts, with windows that stay empty --------------------------------------------------------------------------
@pytest.mark.parametrize("n_win", [1, 8, 32, 33, 64])
def test_window_counts_and_empty_windows_vs_oracle(er, orc, monkeypatch, n_win):
    tiles, win = 6, 1_000
    empty = {0, n_win // 2, n_win - 1} if n_win >= 8 else set()  # at the front, in the middle and at the end
    times = [w * win + r for w in range(n_win) if w not in empty for r in range(0, win, 7)]
    recs = [synth.to_dat8(events(2 * 1280 + 300, tiles, 500 + n_win, 0, 0, times=times))]
    check(er, orc, monkeypatch, f"n_windows={n_win}", tiles, recs, [0], 8, n_win, win)


# ---- 5. a batch of sequences ------------------------------------------------------------------------------------------------
def test_batch_of_sequences_vs_oracle(er, orc, monkeypatch):
    tiles, n_win, win = 9, 8, 10_000
    span = n_win * win
    # the last start leaves t_start + span one tick past 2^32 - 1: `relu >= span` alone would not see t < t_start there, so the
    # kernel may not take the fast block; its events stay inside 32 bits
    starts = [100_000, 7, 3_000_000_000, (1 << 32) - span, 123_456]
    lens = [20_480 + 1_400, 0, 8_192 + 640, 3 * 1280 + 17, 777]
    his = [span, span, span, span - 1, span]
    recs = [synth.to_dat8(events(n, tiles, 600 + j, starts[j], starts[j] + his[j])) for j, n in enumerate(lens)]
    check(er, orc, monkeypatch, "batch", tiles, recs, starts, 8, n_win, win)


# ---- 6. direct mode is what it was -------------------------------------------------------------------------------------------
def test_direct_bins_same_bits_as_tile_bins(er, orc, monkeypatch):
    from frlw_evd_amd import _lib
    tiles = 3
    recs = [synth.to_dat8(events(3 * 1280 + 90, tiles, 700, 0, 80_000))]
    tus = (("direct bins", _lib.FrlwTuning(chunk_major=1, direct_bins=1)), ("tile bins", _lib.FrlwTuning(chunk_major=1, direct_bins=0)),
           ("tile bins, 20 batches", _lib.FrlwTuning(chunk_major=1, direct_bins=0, batches_per_wave=20)))
    check(er, orc, monkeypatch, "direct", tiles, recs, [0], 8, 8, 10_000, tus=tus)
