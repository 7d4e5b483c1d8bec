"""EVT 3.0 decode on the GPU (csrc/evt3.hip through frlw_evd_amd.raw_io) against tests/evt3_restated.py: the output bytes and every
counter must be equal.  The streams put words on the real edges of the kernels' plan -- C words per workgroup chunk, L per lane
piece, 64 L per wavefront (frlw_evt3_geometry) -- and none is longer than about three chunks, but the one that gives the
single-workgroup scans more chunks than they have threads."""
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import evt3_data as D  # noqa: E402
import evt3_restated as R  # noqa: E402
from frlw_evd_amd import _lib, raw_io, synth  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = (240, 304)


@pytest.fixture(scope="module")
def geom():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return raw_io.geometry()


def to_dev(words):
    return torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint16).view(np.int16).copy()).cuda()


def as_records(dat):
    return dat.cpu().numpy().view(synth.DAT_DTYPE).reshape(-1)


def check(words, size=SIZE, time_shift=True):
    """Decode on the GPU and by the restatement: equal bytes, equal counters.  -> (records, counters)."""
    words = np.asarray(words, dtype=np.uint16)
    want, want_c, _ = R.decode(words, size[1], size[0], time_shift=time_shift)
    dat, got_c, _ = raw_io.decode_evt3(to_dev(words), size, time_shift=time_shift)
    got = as_records(dat)
    assert got_c == want_c, (got_c, want_c)
    assert len(got) == len(want)
    differ = np.flatnonzero((got["t"] != want["t"]) | (got["_"] != want["_"]))
    assert len(differ) == 0, "{0} records differ, the first at {1}".format(len(differ), int(differ[0]))
    return got, got_c


PROLOGUE = [D.th(7), D.tl(1), D.ay(3), D.vb(10, 1)]


def mixed(n, seed, setters=True):
    """n words: single events, vector words with random masks, words of no effect, and (setters) a VECT_BASE_X now and then -- no
    TIME_HIGH, TIME_LOW or ADDR_Y.  Starts with PROLOGUE."""
    rng = np.random.default_rng(seed)
    kind = rng.integers(0, 100, size=n)
    x = rng.integers(0, 300, size=n)
    p = rng.integers(0, 2, size=n)
    w = 0x2000 | (p << 11) | x
    w = np.where(kind < 12, D.OTHERS, w)
    w = np.where((kind >= 12) & (kind < 22), D.CONTINUED_12 | rng.integers(0, 4096, size=n), w)
    w = np.where((kind >= 22) & (kind < 40), 0x4000 | rng.integers(0, 4096, size=n), w)
    w = np.where((kind >= 40) & (kind < 50), 0x5000 | rng.integers(0, 4096, size=n), w)
    w = np.where((kind >= 50) & (kind < 55), (0x3000 | (p << 11) | x) if setters else D.TRIGGER, w)
    w = w.astype(np.uint16)
    w[:len(PROLOGUE)] = PROLOGUE[:n]
    return w


# ---- the two reference streams -----------------------------------------------------------------------------------------------
def test_hand_assembled_stream(geom):
    got, counters = check(D.HAND_WORDS, D.HAND_SIZE)
    assert got.tobytes() == D.records_of(D.HAND_EVENTS).tobytes() and counters == D.HAND_COUNTERS
    check(D.HAND_WORDS, D.HAND_SIZE, time_shift=False)


def test_burst_round_trip(geom):
    rec = synth.to_dat8(D.burst_events())
    words = raw_io.encode_evt3(rec)
    assert len(words) <= 5 * geom[0]
    for shift in (False, True):   # the stream opens with EVT_TIME_HIGH 0: the shift is 0
        got, counters = check(words, D.BURST_SIZE, time_shift=shift)
        assert got.tobytes() == rec.tobytes() and counters["events"] == len(rec)


# ---- setters on the edges ------------------------------------------------------------------------------------------------------
SETTERS = {"time_high": D.th(9), "time_low": D.tl(0x777), "addr_y": D.ay(40), "vect_base_x": D.vb(150, 0)}
POSITIONS = ("piece_last", "piece_first", "wave0_last", "chunk0_last", "chunk1_first", "through_chunk")


@pytest.mark.parametrize("where", POSITIONS)
@pytest.mark.parametrize("setter", list(SETTERS))
def test_setter_on_an_edge(geom, setter, where):
    C, L = geom
    pos = {"piece_last": 5 * L - 1, "piece_first": 5 * L, "wave0_last": 64 * L - 1, "chunk0_last": C - 1, "chunk1_first": C,
           "through_chunk": C - 4}[where]
    n = 3 * C if where == "through_chunk" else 2 * C + 9
    words = mixed(n, 100 + POSITIONS.index(where))
    if where == "through_chunk":   # chunk 1 sets nothing: single events and words of no effect only
        words[pos + 1:C] = D.filler(C - pos - 1, 5)
        words[C:2 * C] = D.filler(C, 6)
        assert not np.isin(words[C:2 * C] >> 12, [0x0, 0x3, 0x4, 0x5, 0x6, 0x8]).any()
    plain = words.copy()
    words[pos] = SETTERS[setter]
    got, _ = check(words)
    # the setter is seen by what follows it: the decode differs from the stream without it, behind the edge too
    base = R.decode(plain, SIZE[1], SIZE[0])[0]
    assert got.tobytes() != base.tobytes()
    if where == "through_chunk":
        tail = R.decode(words[:2 * C], SIZE[1], SIZE[0])[2]
        tail_plain = R.decode(plain[:2 * C], SIZE[1], SIZE[0])[2]
        assert {k: tail[k] for k in ("high", "low", "y", "base")} != {k: tail_plain[k] for k in ("high", "low", "y", "base")}


# ---- vector runs across edges ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edge", ["chunk", "piece", "wave"])
def test_vector_run_straddles_an_edge(geom, edge):
    C, L = geom
    at = {"chunk": C, "piece": 7 * L, "wave": 64 * L}[edge]
    words = mixed(C + 500, 31, setters=False)
    run = [D.vb(40, 1), D.v12(0xA5F), D.v8(0x3C), D.v12(0x801), D.v12(0xFFF), D.v8(0xFF), D.ax(9), D.v12(0x111)]
    words[at - 3:at - 3 + len(run)] = run
    check(words)


def test_vector_run_crosses_the_width(geom):
    C, L = geom
    words = mixed(2 * L, 32, setters=False)
    words[L - 2:L + 3] = [D.vb(294, 0), D.v12(0xFFF), D.v12(0xFFF), D.v8(0xFF), D.v12(0x001)]
    got, counters = check(words)
    alone = R.decode(np.concatenate([PROLOGUE, words[L - 2:L + 3]]), SIZE[1], SIZE[0])[1]
    assert alone["events"] == 10 and alone["out_of_frame"] == 2 + 12 + 8 + 1
    assert counters["out_of_frame"] >= alone["out_of_frame"]


# ---- clock wraps -------------------------------------------------------------------------------------------------------------
def wrap_stream(C, placed, n=None):
    """Single events everywhere, TIME_HIGH words where `placed` says ({position: value})."""
    n = n or 2 * C + 40
    words = D.filler(n, 41, x_max=300)
    words[:3] = [D.th(50), D.tl(5), D.ay(2)]
    for pos, v in placed.items():
        words[pos] = D.th(v)
    return words


@pytest.mark.parametrize("case", ["in_piece", "across_pieces", "across_waves", "across_chunks"])
def test_clock_wrap_position(geom, case):
    C, L = geom
    a = {"in_piece": 3 * L + 4, "across_pieces": 3 * L - 1, "across_waves": 64 * L - 1, "across_chunks": C - 1}[case]
    _, counters = check(wrap_stream(C, {a: 4095, a + 1: 0}))
    assert counters["time_loops"] == 1


@pytest.mark.parametrize("back, loops", [(9, 0), (10, 0), (11, 1)])
@pytest.mark.parametrize("gap", ["adjacent", "across_chunks"])
def test_small_steps_back_are_no_wrap(geom, back, loops, gap):
    C, L = geom
    a = C - 1 if gap == "across_chunks" else 2 * L + 3
    words = wrap_stream(C, {a - 2: 100, a + 1: 100 - back})
    words[a] = D.ax(5)                                         # an event between the two TIME_HIGH words
    _, counters = check(words)
    assert counters["time_loops"] == loops and counters["unsorted"] == (1 if loops == 0 else 0)


def test_two_wraps_in_one_chunk_and_a_wrap_across_a_silent_chunk(geom):
    C, L = geom
    _, counters = check(wrap_stream(C, {100: 4095, 900: 0, 901: 4094, 64 * L + 7: 3, 64 * L + 8: 4095, C + 3: 2}))
    assert counters["time_loops"] == 3
    # the two TIME_HIGH words of one wrap in chunks 0 and 2, none in chunk 1
    words = wrap_stream(C, {C - 2: 4095, 2 * C + 1: 0}, n=2 * C + 50)
    assert not (words[C:2 * C] >> 12 == 0x8).any()
    _, counters = check(words)
    assert counters["time_loops"] == 1


# ---- expansion, sync, frame --------------------------------------------------------------------------------------------------
def test_full_expansion(geom):
    """Two chunks of VECT_12 with every bit set: 12 records per word, every offset of the plan in use."""
    C, L = geom
    words = np.full(2 * C, D.v12(0xFFF), dtype=np.uint16)
    words[0::100] = D.vb(0, 1)
    words[:3] = [D.th(0), D.ay(700), D.vb(0, 1)]
    got, counters = check(words, (720, 1280))
    n_vec = int((words >> 12 == 0x4).sum())
    assert counters["events"] == 12 * n_vec and counters["out_of_frame"] == 0
    x = got["_"] & 16383
    assert (x.reshape(-1, 12) % 12 == np.arange(12)).all()


def test_before_sync_junk(geom):
    """Events and vector words ahead of the first TIME_HIGH, the first ADDR_Y and the first VECT_BASE_X, which come in chunk 1."""
    C, L = geom
    words = mixed(2 * C + 100, 51, setters=False)
    words[:4] = [D.ax(1), D.v12(0xF0F), D.v8(0x81), D.ax(2, 1)]
    words[C + 100], words[C + 200], words[C + 300] = D.th(77), D.ay(9), D.vb(30, 1)
    junk = R.decode(words[:C + 100], SIZE[1], SIZE[0])[1]
    assert junk["events"] == 0 and junk["before_sync"] > C
    _, counters = check(words)
    assert counters["before_sync"] > junk["before_sync"] and counters["events"] > 100
    check(words, time_shift=False)


def test_out_of_frame_on_a_smaller_frame(geom):
    words = raw_io.encode_evt3(synth.to_dat8(D.burst_events()))
    got, counters = check(words, (48, 64))
    assert counters["out_of_frame"] > 10_000 and counters["events"] > 100
    assert ((got["_"] & 16383) < 64).all() and (((got["_"] >> 14) & 16383) < 48).all()


def test_sizes(geom):
    C, L = geom
    words = mixed(2 * C + 17, 61)
    for n in (0, 1, L - 1, L, L + 1, C - 1, C, C + 1, 2 * C + 17):
        check(words[:n])


def test_unaligned_words_pointer(geom):
    C, L = geom
    words = mixed(C + 300, 62)
    dev = to_dev(np.concatenate([[0], words]))[1:]            # 2 bytes behind an aligned address
    assert dev.data_ptr() % 16 == 2
    dat, counters, _ = raw_io.decode_evt3(dev.contiguous() if not dev.is_contiguous() else dev, SIZE)
    want, want_c, _ = R.decode(words, SIZE[1], SIZE[0])
    assert as_records(dat).tobytes() == want.tobytes() and counters == want_c


def test_more_chunks_than_scan_threads(geom):
    """258 chunks and 17 words: each thread of the two single-workgroup scans has a range of two chunks, threads 0..129 have
    work, the ranges of the rest are clipped to nothing.  TIME_HIGH (rising, no wrap), TIME_LOW and ADDR_Y words spread over the
    stream, so the state a range carries in differs from range to range."""
    C, L = geom
    n = 258 * C + 17
    words = mixed(n, 91)
    rng = np.random.default_rng(92)
    at = np.sort(rng.choice(np.arange(8, n), size=900, replace=False))
    highs = 7 + np.sort(rng.integers(0, 3000, size=300))
    for i, pos in enumerate(at):
        words[pos] = (D.th(int(highs[i // 3])), D.tl(int(rng.integers(0, 4096))), D.ay(int(rng.integers(0, 250))))[i % 3]
    assert -(-n // C) > 256
    _, counters = check(words)
    assert counters["events"] > 0 and counters["unsorted"] > 0 and counters["out_of_frame"] > 0


# ---- carried state -----------------------------------------------------------------------------------------------------------
def test_carried_state(geom):
    C, L = geom
    words = mixed(2 * C + 40, 71)
    words[C + 50:C + 55] = [D.vb(60, 1), D.v12(0x333), D.v12(0xFFF), D.v8(0x18), D.v12(0x800)]
    words[C - 9], words[C + 20] = D.th(4090), D.th(1)         # a wrap whose halves the cuts around C separate
    want, want_c, _ = R.decode(words, SIZE[1], SIZE[0])
    one, one_c, _ = raw_io.decode_evt3(to_dev(words), SIZE)
    assert as_records(one).tobytes() == want.tobytes() and one_c == want_c
    for cut in (C - 1, C, C + 1, C + 52, 3):
        a, ca, state = raw_io.decode_evt3(to_dev(words[:cut]), SIZE)
        b, cb, _ = raw_io.decode_evt3(to_dev(words[cut:]), SIZE, state=state)
        assert (as_records(a).tobytes() + as_records(b).tobytes()) == want.tobytes(), cut
        for k in ("events", "before_sync", "out_of_frame", "triggers", "other_words", "time_loops", "unsorted"):
            assert ca[k] + cb[k] == want_c[k], (cut, k)
        # the shift is the first call's first TIME_HIGH (7), also for the second call that holds none before the wrap's words
        assert state.first_high == 7 and (cb["last_t"] if cb["events"] else ca["last_t"]) == want_c["last_t"]


def test_rawfile_decodes_piece_by_piece(geom, tmp_path, monkeypatch):
    C, L = geom
    rec = synth.to_dat8(D.burst_events())
    path = str(tmp_path / "r.raw")
    raw_io.write_raw(path, rec, 240, 304)
    f = raw_io.RawFile(path)
    dat, counters = f.decode()
    assert as_records(dat).tobytes() == rec.tobytes() and f.total_time() == int(rec["t"][-1])
    monkeypatch.setattr(raw_io.RawFile, "PIECE_WORDS", C + 5)
    assert len(f) > 2 * (C + 5)
    dat2, counters2 = raw_io.RawFile(path).decode()
    assert torch.equal(dat, dat2) and counters2 == counters


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_t_beyond_32_bits_is_refused_and_nothing_written(geom):
    words = np.array([D.th(0), D.ay(0), D.ax(1)] + [D.th(4095), D.th(0)] * 257 + [D.ax(2)], dtype=np.uint16)
    with pytest.raises(ValueError):
        R.decode(words, SIZE[1], SIZE[0])
    dev = to_dev(words)
    counters, state, ws = raw_io.evt3_count(dev, SIZE)
    assert counters.events == 2 and counters.time_loops == 257
    out = torch.full((2, 8), 0xA5, dtype=torch.uint8, device="cuda")
    assert raw_io.evt3_emit(dev, SIZE, ws, out, 2) == _lib.FRLW_ERR_SPAN
    assert bool((out == 0xA5).all())
    with pytest.raises(ValueError, match="2\\^32"):
        raw_io.decode_evt3(dev, SIZE)
    got, _ = check(np.concatenate([words[:3 + 2 * 255], [D.ax(2)]]))   # 255 wraps still fit
    assert got["t"].tolist() == [0, 255 << 24]


def test_short_capacity_is_refused_and_nothing_written(geom):
    C, L = geom
    words = mixed(C + 77, 81)
    dev = to_dev(words)
    counters, state, ws = raw_io.evt3_count(dev, SIZE)
    n = int(counters.events)
    assert n > 1000
    out = torch.full((n + 4, 8), 0x5A, dtype=torch.uint8, device="cuda")
    assert raw_io.evt3_emit(dev, SIZE, ws, out, n - 1) == _lib.FRLW_ERR_ARG
    assert bool((out == 0x5A).all())
    # the right capacity on the same plan: the records, and nothing behind them
    assert raw_io.evt3_emit(dev, SIZE, ws, out, n) == _lib.FRLW_OK
    assert as_records(out[:n]).tobytes() == R.decode(words, SIZE[1], SIZE[0])[0].tobytes() and bool((out[n:] == 0x5A).all())


def test_one_unsorted_event(geom):
    words = [D.th(3), D.ay(1), D.tl(500), D.ax(1), D.ax(2), D.tl(499), D.ax(3), D.tl(501), D.ax(4)]
    _, counters = check(words)
    assert counters["unsorted"] == 1


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def test_detect_recording_raw_equals_dat(geom, tmp_path):
    """detect_recording.py on one synthetic GEN1-sized recording written as *_td.dat and as EVT 3.0 .raw: byte-identical box files."""
    from test_stream_detect_gpu import PERIOD, T_BEGIN, recording
    from frlw_evd_amd import dat_io
    from frlw_evd_amd.yolox import build_yolox
    from frlw_evd_amd.yolox.model import recipe_state_dict
    rec = recording((240, 304), 21)
    dat_path, raw_path = str(tmp_path / "rec_td.dat"), str(tmp_path / "rec.raw")
    dat_io.write_dat(dat_path, rec, 240, 304)
    raw_io.write_raw(raw_path, rec, 240, 304)
    assert raw_io.RawFile(raw_path).words[0] == 0x8000           # the first TIME_HIGH is 0: the shift is 0
    net = build_yolox(16, 2)
    ck = str(tmp_path / "weights.pth")
    torch.save({"state_dict": {"module." + k: v for k, v in recipe_state_dict(net, seed=1004).items()}, "epoch": 0}, ck)
    outs = {}
    for flag, path in (("--dat", dat_path), ("--raw", raw_path)):
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
        out = str(tmp_path / ("boxes" + flag[2:]))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "detect_recording.py"), flag, path, "--dataset", "gen1", "--exp_type", "yolox",
                            "--checkpoint", ck, "--event_volume_bins", "8", "--period", str(PERIOD), "--t_begin", str(T_BEGIN), "--out", out,
                            "--log_path", str(tmp_path) + "/"], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs[flag] = (open(out + ".npy", "rb").read(), r.stdout)
    assert outs["--dat"][0] == outs["--raw"][0]
    frames = [int(re.search(r"'frames': (\d+)", outs[flag][1]).group(1)) for flag in ("--dat", "--raw")]
    assert frames[0] == frames[1] >= 10 and len(outs["--raw"][0]) > 200
    assert "'before_sync': 0" in outs["--raw"][1] and "'out_of_frame': 0" in outs["--raw"][1] and "'unsorted': 0" in outs["--raw"][1]
    assert "'events': {0}".format(len(rec)) in outs["--raw"][1] and "before_sync" not in outs["--dat"][1]
