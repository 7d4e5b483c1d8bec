"""frlw_taf_encode_chain / encode_taf_chain: the TAF volume after chosen windows of ONE launch (k_taf_tile_snap, csrc/enc_taf.h).

The stream is the one of tests/test_tile_forms_gpu.py -- ragged on both edges at every tile width, the busiest tile longer than
one counting-sort slice -- sorted and under that file's permutation, 8 windows of 10 000 us.  Every snapshot and the final state
are bit-equal to the route the library already had: one ``encode_taf_dat(fast=False)`` call per step on the time-cut records
with the state carried.  Against the CPU oracle the bars of the tile tests hold: float32 state bit for bit, uint8 within 1 LSB
in at most 1e-4 of the bytes.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from frlw_evd_amd import synth  # noqa: E402
from golden_util import assert_bitexact, assert_u8_budget  # noqa: E402
from test_tile_forms_gpu import header_words, tile_counts  # noqa: E402

pytestmark = pytest.mark.gpu

H, W, N, SPAN = 20, 300, 60_000, 80_000
WINDOW_US, N_WINDOWS = 10_000, 8
HOT_RECORDS = 2000
MODES = {"quarter": {}, "whole": dict(quarter_below=0, hot_tile_records=2 ** 30),
         "hot": dict(quarter_below=0, hot_tile_records=HOT_RECORDS)}
MASKS = (0xFF, 0b10100100)


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


def host(t):
    return t.cpu().numpy()


def state0(K, shape=(H, W)):
    return np.random.default_rng(K).uniform(-50, 0, size=(shape[0], shape[1], 2, K)).astype(np.float32)


def bits_of(mask):
    return [w for w in range(64) if (mask >> w) & 1]


@pytest.fixture(scope="module")
def stream():
    ev = synth.synth_events(41, N, W, H, SPAN, hotspot=True)
    perm = np.random.default_rng(5).permutation(N)
    return {"sorted": synth.to_dat8(ev), "shuffled": synth.to_dat8({k: v[perm] for k, v in ev.items()})}


def chain_call(er, rec, K, n_windows, mask, st, shape=(H, W), t_start=0, window_us=WINDOW_US, flags=None):
    """One frlw_taf_encode_chain call on the records ``rec`` -> snapshots (popcount(mask), K, 2, H, W); ``st`` in place."""
    from frlw_evd_amd import _lib
    d, desc = er._events_dat(to_dev(rec))
    ws = er._workspace(desc.n, shape[0], shape[1], d.device)
    snaps = torch.empty((bin(mask).count("1"), K, 2, shape[0], shape[1]), dtype=torch.uint8, device="cuda")
    rc = _lib.load().frlw_taf_encode_chain(C.byref(desc), shape[0], shape[1], K, t_start, window_us, n_windows, mask, er._ptr(st),
                                           er._ptr(snaps), _lib.TAF_U8_FLIP_K if flags is None else flags, er._ptr(ws), ws.numel(),
                                           er._stream())
    _lib.check(rc, "frlw_taf_encode_chain")
    er._finish(ws, "frlw_taf_encode_chain")
    return snaps


def sequential(er, rec, K, mask, st, n_windows=N_WINDOWS, shape=(H, W), t_start=0, window_us=WINDOW_US):
    """The route without the chain: one encode_taf_dat(fast=False) per step on the records of the step's time range (stream order
    kept, a boundary event to the later step, the tail of the stream to the last one) with the state carried -> list of uint8
    volumes, one per bit of ``mask``; ``st`` holds the state after all ``n_windows`` windows."""
    t = rec["t"].astype(np.int64)
    ends = bits_of(mask)
    steps = [(a + 1, b + 1) for a, b in zip([-1] + ends[:-1], ends)]
    if ends[-1] + 1 < n_windows:
        steps.append((ends[-1] + 1, n_windows))
    out = []
    for w0, w1 in steps:
        lo, hi = t_start + w0 * window_us, t_start + w1 * window_us
        sel = (t >= lo) & ((t < hi) if w1 < n_windows else np.ones(len(t), bool))
        if w0 == 0:
            sel |= t < lo
        u8, _ = er.encode_taf_dat(to_dev(rec[sel]), shape, st, lo, window_us, w1 - w0, K, want_u8=True, fast=False)
        if w1 - 1 in ends:
            out.append(u8)
    return out


@pytest.fixture(scope="module")
def want(er, stream):
    """The sequential route at the library's own launch choice, once for all the cases: (K, order, mask) -> (uint8 volumes, state)."""
    out = {}
    for K in (8, 5):
        for order in ("sorted", "shuffled"):
            for mask in MASKS:
                st = torch.from_numpy(state0(K)).cuda()
                vols = sequential(er, stream[order], K, mask, st)
                out[K, order, mask] = ([host(v) for v in vols], host(st))
    return out


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("twl", [6, 7, 8])
def test_every_form_equals_the_sequential_route(er, stream, want, monkeypatch, twl, mode):
    """k_taf_tile_snap at each width in each launch mode, K = 8 and 5, sorted (window-sorted loop) and shuffled (the loop gives up
    after it has written snapshots; the window-interleaved pass writes them all again): snapshots and state bit-equal."""
    from frlw_evd_amd import _lib
    monkeypatch.setattr(er, "TUNING", _lib.FrlwTuning(tile_width_log2=twl, **MODES[mode]))
    ev = synth.from_dat8(stream["sorted"])
    n_listed = int((tile_counts(ev, twl) > HOT_RECORDS).sum())
    for K in (8, 5):
        for order in ("sorted", "shuffled"):
            for mask in MASKS:
                what = f"width {twl} {mode} K={K} {order} mask {mask:#x}"
                vols, wst = want[K, order, mask]
                st = torch.from_numpy(state0(K)).cuda()
                snaps = host(chain_call(er, stream[order], K, N_WINDOWS, mask, st))
                # WHICH form ran, as tests/test_tile_forms_gpu.py reads it: the sorted stream stays on the window-sorted loop in every
                # tile, the shuffled one leaves it; the hot list holds the tiles above the threshold in "hot" mode, nothing in "whole"
                pad, n_hot, _ = header_words(er)
                assert (pad > 0) == (order == "shuffled"), what
                assert n_hot == (n_listed if mode == "hot" else n_hot if mode == "quarter" else 0), (what, n_hot)
                assert len(vols) == snaps.shape[0]
                for s, v in enumerate(vols):
                    assert_bitexact(snaps[s], v, f"snapshot {s}, {what}")
                assert_bitexact(host(st), wst, f"state, {what}")


@pytest.mark.parametrize("order", ["sorted", "shuffled"])
def test_emitted_windows_against_the_oracle(er, orc, stream, order):
    """After each emitted window w: the state equals taf_stream_dat8 on the records with t < (w + 1) windows bit for bit (a chain
    that ends at w hands it out), and the snapshot of the FULL chain is the oracle's uint8 volume within the tile tests' budget."""
    K, mask = 8, 0b10100100
    rec = stream[order]
    st = torch.from_numpy(state0(K)).cuda()
    snaps = host(chain_call(er, rec, K, N_WINDOWS, mask, st))
    for s, w in enumerate(bits_of(mask)):
        part = rec[rec["t"].astype(np.int64) < (w + 1) * WINDOW_US] if w + 1 < N_WINDOWS else rec
        oview, ost = orc.taf_stream_dat8(part, (H, W), (H, W), K, 0, WINDOW_US, w + 1, state0(K))
        ou8 = np.ascontiguousarray(orc.quantize_u8(orc.leaky_transform(oview.reshape(K, 2, H, W)))[::-1])
        sw = torch.from_numpy(state0(K)).cuda()
        last = host(chain_call(er, part, K, w + 1, 1 << w, sw))
        assert_bitexact(host(sw), ost, f"state after window {w}, {order}")
        assert_bitexact(last[0], snaps[s], f"snapshot after window {w}: chain that ends there vs full chain, {order}")
        assert_u8_budget(snaps[s], ou8, 1e-4, f"uint8 after window {w}, {order}")
    assert_bitexact(host(st), ost, f"final state, {order}")


def test_empty_window_emits_the_previous_volume(er, stream):
    """No event in window 3: the FIFO does not step (generate_taf.py:40-41), its snapshot is the one of window 2."""
    K, mask = 8, 0b1100
    rec = stream["sorted"]
    t = rec["t"].astype(np.int64)
    rec = rec[(t < 3 * WINDOW_US) | (t >= 4 * WINDOW_US)]
    per_window = np.bincount(np.minimum(rec["t"].astype(np.int64) // WINDOW_US, N_WINDOWS - 1), minlength=N_WINDOWS)
    assert per_window[3] == 0 and (np.delete(per_window, 3) > 0).all(), per_window
    st = torch.from_numpy(state0(K)).cuda()
    snaps = host(chain_call(er, rec, K, N_WINDOWS, mask, st))
    assert_bitexact(snaps[1], snaps[0], "snapshot of the empty window")
    ss = torch.from_numpy(state0(K)).cuda()
    vols = sequential(er, rec, K, mask, ss)
    assert_bitexact(snaps[0], host(vols[0]), "window 2")
    assert_bitexact(snaps[1], host(vols[1]), "window 3 (empty)")
    assert_bitexact(host(st), host(ss), "state")
    assert not np.array_equal(snaps[0], host(chain_call(er, rec, K, N_WINDOWS, 0b10000, torch.from_numpy(state0(K)).cuda()))[0])


def test_boundary_events(er, orc, stream):
    """An event at exactly t_start + 3 windows lands in window 3 (the later one), one at exactly t_start + 8 windows in window 7
    (the clamp): the snapshot in front of its window does not see it, the snapshot of its window does."""
    K = 8
    base = stream["sorted"][::50]
    t = base["t"].astype(np.int64)
    base = base[(t % WINDOW_US != 0)]   # no other event on a boundary
    assert (np.bincount(base["t"].astype(np.int64) // WINDOW_US, minlength=N_WINDOWS) > 0).all()

    def with_event(at, x, y):
        one = synth.to_dat8({"x": np.array([x]), "y": np.array([y]), "p": np.array([1]), "t": np.array([at])})
        k = int(np.searchsorted(base["t"], at, side="left"))
        return np.concatenate([base[:k], one, base[k:]])

    def run(rec):
        st = torch.from_numpy(state0(K)).cuda()
        return host(chain_call(er, rec, K, N_WINDOWS, 0xFF, st)), host(st)

    plain, _ = run(base)
    for at, x, y, window in ((3 * WINDOW_US, 7, 3, 3), (8 * WINDOW_US, 290, 19, 7)):
        rec = with_event(at, x, y)
        got, gst = run(rec)
        for s in range(window):
            assert_bitexact(got[s], plain[s], f"event at {at}: snapshot {s} lies in front of window {window}")
        diff = np.argwhere(got[window] != plain[window])
        assert len(diff) and {(int(d[1]), int(d[2]), int(d[3])) for d in diff} == {(1, y, x)}, (at, diff[:4])
        _, ost = orc.taf_stream_dat8(rec, (H, W), (H, W), K, 0, WINDOW_US, N_WINDOWS, state0(K))
        assert_bitexact(gst, ost, f"event at {at}: final state against the oracle")


def test_more_than_64_windows_equals_label_calls(er):
    """bins = [70, 1, 5, 64, 3] at 1 000 us: groups of 64 windows that do not line up with the steps, a step that spans two
    groups, a group that emits nothing of its own -- equal to five encode_taf_label calls on the time-cut records."""
    h, w, K, win, bins = 16, 44, 8, 1000, [70, 1, 5, 64, 3]
    total = sum(bins)
    rec = synth.to_dat8(synth.synth_events(43, 30_000, w, h, total * win))
    d = to_dev(rec)
    ends = np.cumsum(bins) * win
    cuts = [0] + [int(c) for c in np.searchsorted(rec["t"], ends[:-1], side="left")] + [len(rec)]
    sl = torch.from_numpy(state0(K, (h, w))).cuda()
    vols = [host(er.encode_taf_label(d[cuts[i]:cuts[i + 1]], (h, w), sl, int(ends[i]) - b * win, win, b, K, fast=False))
            for i, b in enumerate(bins)]
    sc = torch.from_numpy(state0(K, (h, w))).cuda()
    snaps = host(er.encode_taf_chain(d, (h, w), sc, 0, win, bins, K))
    assert snaps.shape == (len(bins), K, 2, h, w)
    for i, v in enumerate(vols):
        assert_bitexact(snaps[i], v, f"step {i}")
    assert_bitexact(host(sc), host(sl), "state")
    with pytest.raises(ValueError):
        er.encode_taf_chain(d, (h, w), sc, 0, win, [3, 0, 2], K)


def test_argument_checks(er, stream):
    """Each FRLW_ERR_ARG case of the entry point, beside a call that is served."""
    from frlw_evd_amd import _lib
    lib = _lib.load()
    K = 8
    d, desc = er._events_dat(to_dev(stream["sorted"][:1000]))
    ws = er._workspace(desc.n, H, W, d.device)
    st = torch.from_numpy(state0(K)).cuda()
    snaps = torch.empty((2, K, 2, H, W), dtype=torch.uint8, device="cuda")

    def call(ev=desc, n_windows=8, mask=0b101, state=st, snap=snaps, window_us=WINDOW_US):
        return lib.frlw_taf_encode_chain(C.byref(ev) if ev is not None else None, H, W, K, 0, window_us, n_windows, mask,
                                         er._ptr(state), er._ptr(snap), 0, er._ptr(ws), ws.numel(), er._stream())
    f64 = _lib.FrlwEvents(d.data_ptr(), 100, _lib.LAYOUT_XYTP_F64, 4, None, None, 0, 0, None)
    assert call(mask=0) == _lib.FRLW_ERR_ARG
    assert call(mask=1 << 8) == _lib.FRLW_ERR_ARG
    assert call(mask=(1 << 63) | 1, n_windows=63) == _lib.FRLW_ERR_ARG
    assert call(n_windows=0) == _lib.FRLW_ERR_ARG
    assert call(n_windows=65) == _lib.FRLW_ERR_ARG
    assert call(state=None) == _lib.FRLW_ERR_ARG
    assert call(snap=None) == _lib.FRLW_ERR_ARG
    assert call(ev=f64, n_windows=1, mask=1) == _lib.FRLW_ERR_ARG
    assert call(window_us=0) == _lib.FRLW_ERR_ARG
    before = host(st).copy()
    torch.cuda.synchronize()
    assert_bitexact(host(st), before, "a refused call leaves the state alone")
    assert call() == _lib.FRLW_OK
    er._finish(ws, "frlw_taf_encode_chain")
    assert not np.array_equal(host(st), before)
