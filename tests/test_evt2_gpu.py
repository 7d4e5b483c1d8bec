"""EVT 2.0 / EVT 2.1 decode on the GPU (csrc/evt2.hip through frlw_evd_amd.raw_io) against tests/evt2_restated.py: the output bytes,
every counter and the carried state must be equal.  The streams put words on the real edges of the kernels' plan -- C words per
workgroup chunk, L per lane piece, 64 L per wavefront (frlw_evt2_geometry, per encoding) -- and none is longer than three chunks and
a few words, but the one that gives the single-workgroup scans more chunks than they have threads."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import evt2_data as D  # noqa: E402
import evt2_restated as R  # noqa: E402
from frlw_evd_amd import _lib, raw_io, synth  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = (240, 304)
ENCS = D.ENCODINGS
DECODE = {"EVT2": raw_io.decode_evt2, "EVT21": raw_io.decode_evt21}
ENCODE = {"EVT2": raw_io.encode_evt2, "EVT21": raw_io.encode_evt21}
SIGNED = {"EVT2": np.int32, "EVT21": np.int64}
SUMMED = R.COUNTERS[:7]


@pytest.fixture(scope="module", params=ENCS)
def plan(request):
    """(encoding, C, L)"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return (request.param,) + raw_io.geometry(request.param)


def to_dev(words, enc):
    return torch.from_numpy(np.ascontiguousarray(words, dtype=D.DTYPE[enc]).view(SIGNED[enc]).copy()).cuda()


def as_records(dat):
    return dat.cpu().numpy().view(synth.DAT_DTYPE).reshape(-1)


def assert_same_state(got, want):
    """A FrlwEvt2State against the restatement's state dict."""
    assert bool(got.flags & 1) == (want["high"] is not None) and got.loops == want["loops"]
    if want["high"] is not None:
        assert (got.first_high, got.last_high) == (want["first_high"], want["high"])
    assert bool(got.has_last_t) == (want["prev_t"] is not None)
    if want["prev_t"] is not None:
        assert got.last_t == want["prev_t"]


def assert_same_records(got, want):
    assert len(got) == len(want)
    differ = np.flatnonzero((got["t"] != want["t"]) | (got["_"] != want["_"]))
    assert len(differ) == 0, "{0} records differ, the first at {1}".format(len(differ), int(differ[0]))


def check(words, enc, size=SIZE, time_shift=True):
    """Decode on the GPU and by the restatement: equal bytes, equal counters, equal carried state.  -> (records, counters).  A
    stream the restatement refuses fails the test here: no case is skipped."""
    words = np.asarray(words, dtype=D.DTYPE[enc])
    want, want_c, want_s = R.decode(words, size[1], size[0], enc, time_shift=time_shift)
    dat, got_c, got_s = DECODE[enc](to_dev(words, enc), size, time_shift=time_shift)
    assert got_c == want_c, (got_c, want_c)
    assert_same_records(as_records(dat), want)
    assert_same_state(got_s, want_s)
    return as_records(dat), got_c


def event_stream(n, seed, enc, high=50):
    """n words of events and words of no effect behind an opening EVT_TIME_HIGH."""
    words = D.filler(n, seed, enc)
    words[0] = D.th(high, enc)
    return words


# ---- the reference streams ---------------------------------------------------------------------------------------------------
def test_hand_assembled_stream(plan):
    enc = plan[0]
    got, counters = check(D.HAND_WORDS[enc], enc, D.HAND_SIZE)
    assert got.tobytes() == D.records_of(D.HAND_EVENTS[enc], D.HAND_SHIFT).tobytes()
    assert counters == D.shifted(D.HAND_COUNTERS[enc], D.HAND_SHIFT)
    got, counters = check(D.HAND_WORDS[enc], enc, D.HAND_SIZE, time_shift=False)
    assert got.tobytes() == D.records_of(D.HAND_EVENTS[enc]).tobytes() and counters == D.HAND_COUNTERS[enc]


def test_writer_round_trip(plan):
    enc, C, L = plan
    rec = synth.to_dat8(D.burst_events(n={"EVT2": 8_000, "EVT21": 6_500}[enc], t_span=50_000))
    words = ENCODE[enc](rec)
    assert 2 * C < len(words) <= 3 * C + 17
    for shift in (False, True):   # the stream opens with EVT_TIME_HIGH 0: the shift is 0
        got, counters = check(words, enc, D.BURST_SIZE, time_shift=shift)
        assert got.tobytes() == rec.tobytes() and counters["events"] == len(rec)


# ---- EVT_TIME_HIGH on the edges ----------------------------------------------------------------------------------------------
POSITIONS = ("piece_last", "piece_first", "wave0_last", "chunk0_last", "chunk1_first", "through_chunk")


@pytest.mark.parametrize("where", POSITIONS)
def test_time_high_on_an_edge(plan, where):
    enc, C, L = plan
    pos = {"piece_last": 5 * L - 1, "piece_first": 5 * L, "wave0_last": 64 * L - 1, "chunk0_last": C - 1, "chunk1_first": C,
           "through_chunk": C - 4}[where]
    n = 3 * C if where == "through_chunk" else 2 * C + 9
    plain = event_stream(n, 100 + POSITIONS.index(where), enc)
    words = plain.copy()
    words[pos] = D.th(60, enc)
    got, _ = check(words, enc)
    # the word is seen by everything behind the edge: all of those records differ from the stream without it
    base = R.decode(plain, SIZE[1], SIZE[0], enc)[0]
    behind = R.decode(words[pos + 1:], SIZE[1], SIZE[0], enc, state=R.decode(words[:pos + 1], SIZE[1], SIZE[0], enc)[2])[1]["events"]
    assert behind > 100 and (got["t"][-behind:] != base["t"][-behind:]).all() and (got["_"][-behind:] == base["_"][-behind:]).all()
    in_front = len(got) - behind
    assert in_front > 20 and (got["t"][:in_front] == base["t"][:in_front]).all()
    if where == "through_chunk":   # chunk 1 holds no EVT_TIME_HIGH: it takes its time from chunk 0, and hands it to chunk 2
        tail = R.decode(words[:2 * C], SIZE[1], SIZE[0], enc)[2]
        assert tail["high"] == 60 and R.decode(plain[:2 * C], SIZE[1], SIZE[0], enc)[2]["high"] == 50


# ---- sync --------------------------------------------------------------------------------------------------------------------
def bits_of(words, enc):
    """Events the event words of the stream stand for."""
    w = np.asarray(words, dtype=D.DTYPE[enc])
    if enc == "EVT2":
        return int((w >> np.uint32(28) <= 1).sum())
    masks = (w & np.uint64(0xFFFFFFFF))[(w >> np.uint64(60)) <= 1]
    return int(sum(bin(int(m)).count("1") for m in masks))


def test_first_time_high_behind_a_whole_chunk(plan):
    enc, C, L = plan
    words = D.filler(2 * C + 50, 51, enc)
    words[C + 3] = D.th(77, enc)
    got, counters = check(words, enc)
    assert counters["before_sync"] == bits_of(words[:C + 3], enc) > C // 2 and counters["events"] > 100
    check(words, enc, time_shift=False)


def test_no_time_high_at_all(plan):
    enc, C, L = plan
    words = D.filler(C + 40, 52, enc)
    got, counters = check(words, enc)
    assert counters["events"] == 0 and len(got) == 0 and counters["before_sync"] == bits_of(words, enc) > C // 2
    assert counters["triggers"] > 0 and counters["other_words"] > 0


# ---- the clock ---------------------------------------------------------------------------------------------------------------
TOP = (1 << 28) - 1


@pytest.mark.parametrize("edge", ["chunk", "lane", "wave"])
def test_wrap_across_an_edge(plan, edge):
    """The two EVT_TIME_HIGH words of a wrap on either side of a chunk, lane-piece or wavefront boundary."""
    enc, C, L = plan
    a = {"chunk": C - 1, "lane": 3 * L - 1, "wave": 64 * L - 1}[edge]
    words = event_stream(C + 300, 41, enc, high=TOP - 2)
    words[a], words[a + 1] = D.th(TOP, enc), D.th(0, enc)
    got, counters = check(words, enc)
    assert counters["time_loops"] == 1 and int(got["t"][-1]) >> 6 == 3      # (2^28 + 0) - (2^28 - 3)
    # the same wrap with a silent chunk between its words
    words = event_stream(2 * C + 50, 42, enc, high=TOP - 2)
    words[C - 2], words[2 * C + 1] = D.th(TOP, enc), D.th(0, enc)
    assert check(words, enc)[1]["time_loops"] == 1


@pytest.mark.parametrize("back", [1, 9, 10])
def test_backward_step_across_a_chunk_boundary(plan, back):
    """A step back inside the no-wrap slack whose EVT_TIME_HIGH is the first word of chunk 1.  The events have one constant low
    value, so the only unsorted step is that one: the last event of chunk 0 against the first of chunk 1.  (A step of 11 is a
    wrap, and a wrap adds 2^34 to t: test_wrap_across_an_edge has the streams in which that fits.)"""
    enc, C, L = plan
    rng = np.random.default_rng(43)
    n = C + 200
    words = D.words_of([D.cd(int(x), int(y), int(p), 7, enc) for x, y, p in zip(rng.integers(0, 300, n), rng.integers(0, 240, n), rng.integers(0, 2, n))], enc)
    words[0], words[1], words[C] = D.th(80, enc), D.th(100, enc), D.th(100 - back, enc)
    got, counters = check(words, enc)
    assert counters["time_loops"] == 0 and counters["unsorted"] == 1 and counters["events"] == n - 3
    assert int(got["t"][C - 3]) == (20 << 6) + 7 and int(got["t"][C - 2]) == ((20 - back) << 6) + 7


# ---- expansion and the frame -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x_of", ["inside", "half_outside"])
def test_evt21_full_expansion(x_of):
    """Two chunks of EVT 2.1 words with all 32 bits set: 32 records a word (16 where the word straddles the right edge), the output
    sized to the event exactly, nothing written behind it."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    enc, size = "EVT21", (720, 1280)
    C, L = raw_io.geometry(enc)
    i = np.arange(2 * C)
    x = 32 * (i % 40) if x_of == "inside" else np.full(2 * C, size[1] - 16)
    words = D.words_of([D.cd(int(a), int(b), int(b & 1), int(b % 64), enc, 0xFFFFFFFF) for a, b in zip(x, i % 720)], enc)
    words[0] = D.th(5, enc)
    want, want_c, _ = R.decode(words, size[1], size[0], enc)
    per_word = 32 if x_of == "inside" else 16
    assert want_c["events"] == per_word * (2 * C - 1) and want_c["out_of_frame"] == (32 - per_word) * (2 * C - 1)
    dev = to_dev(words, enc)
    counters, _, ws = raw_io.evt2_count(dev, size, encoding=enc)
    n = int(counters.events)
    assert n == want_c["events"] and int(counters.out_of_frame) == want_c["out_of_frame"]
    out = torch.full((n + 64, 8), 0xA5, dtype=torch.uint8, device="cuda")
    assert raw_io.evt2_emit(dev, size, ws, out, n, encoding=enc) == _lib.FRLW_OK        # capacity == events exactly
    assert_same_records(as_records(out[:n]), want)
    assert bool((out[n:] == 0xA5).all())
    got = as_records(out[:n])
    assert ((got["_"] & 16383).reshape(-1, per_word) - x[1:, None] == np.arange(per_word)).all()


def test_single_words_on_the_frame_edges(plan):
    enc, C, L = plan
    H, W = SIZE
    mask = 0xFFFFFFFF if enc == "EVT21" else 1
    for x, y, events, dropped in ((W - 5, 3, 5, 27), (W - 1, H - 1, 1, 31), (W, 3, 0, 32), (0, H, 0, 32), (W - 40, H - 1, 32, 0)):
        got, counters = check([D.th(1, enc), D.cd(x, y, 1, 9, enc, mask)], enc)
        if enc == "EVT21":
            assert (counters["events"], counters["out_of_frame"]) == (events, dropped)
            assert (got["_"] & 16383).tolist() == list(range(x, x + events))
        else:
            assert (counters["events"], counters["out_of_frame"]) == (min(events, 1), 1 - min(events, 1))


# ---- pointers and lengths ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skip", [1, 3])
def test_unaligned_words_pointer(plan, skip):
    """A view that starts `skip` words into a device tensor: word-aligned, not 16-byte aligned: the narrow loads."""
    enc, C, L = plan
    words = D.fuzz(C + 300, 62, enc)
    dev = to_dev(np.concatenate([np.zeros(skip, D.DTYPE[enc]), words]), enc)[skip:]
    assert dev.data_ptr() % 16 == (skip * D.DTYPE[enc]().itemsize) % 16 != 0 and dev.is_contiguous()
    dat, counters, state = DECODE[enc](dev, SIZE)
    want, want_c, want_s = R.decode(words, SIZE[1], SIZE[0], enc)
    assert_same_records(as_records(dat), want)
    assert counters == want_c
    assert_same_state(state, want_s)


def test_sizes(plan):
    enc, C, L = plan
    words = D.fuzz(C + 1, 61, enc)
    for n in (0, 1, L - 1, L, C - 1, C, C + 1):
        check(words[:n], enc)
        check(words[-n:] if n else words[:0], enc)       # the same lengths without an EVT_TIME_HIGH at their start


# ---- refusals ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["beyond", "negative"])
def test_t_out_of_range_is_refused_and_nothing_written(plan, which):
    enc = plan[0]
    words = D.clock_streams(enc)["beyond"] if which == "beyond" else D.words_of([D.th(100, enc), D.th(95, enc), D.cd(1, 1, 0, 0, enc)], enc)
    with pytest.raises(ValueError):
        R.decode(words, SIZE[1], SIZE[0], enc)
    dev = to_dev(words, enc)
    counters, state, ws = raw_io.evt2_count(dev, SIZE, encoding=enc)
    n = int(counters.events)
    assert n == (2 if which == "beyond" else 1)
    out = torch.full((n + 2, 8), 0xA5, dtype=torch.uint8, device="cuda")
    assert raw_io.evt2_emit(dev, SIZE, ws, out, n, encoding=enc) == _lib.FRLW_ERR_SPAN
    assert bool((out == 0xA5).all())
    with pytest.raises(ValueError, match="2\\^32"):
        DECODE[enc](dev, SIZE)
    if which == "negative":      # without the shift the same words are in range
        assert check(words, enc, time_shift=False)[0]["t"].tolist() == [95 << 6]


def test_t_on_the_edges_of_the_range(plan):
    enc = plan[0]
    s = D.clock_streams(enc)
    got, counters = check(s["wrap"], enc)
    assert got["t"].tolist() == [63, 64] and counters["time_loops"] == 1
    for shift in (True, False):
        assert check(s["edge"], enc, time_shift=shift)[0]["t"].tolist() == [0, (1 << 32) - 1]
    dev = to_dev(s["wrap"], enc)                        # unshifted, the wrap stream's t need 35 bits
    counters, _, ws = raw_io.evt2_count(dev, SIZE, encoding=enc)
    out = torch.full((2, 8), 0xA5, dtype=torch.uint8, device="cuda")
    assert raw_io.evt2_emit(dev, SIZE, ws, out, 2, time_shift=False, encoding=enc) == _lib.FRLW_ERR_SPAN and bool((out == 0xA5).all())


def test_short_capacity_is_refused_and_nothing_written(plan):
    enc, C, L = plan
    words = D.fuzz(C + 77, 81, enc)
    dev = to_dev(words, enc)
    counters, state, ws = raw_io.evt2_count(dev, SIZE, encoding=enc)
    n = int(counters.events)
    assert n > 1000
    out = torch.full((n + 4, 8), 0x5A, dtype=torch.uint8, device="cuda")
    assert raw_io.evt2_emit(dev, SIZE, ws, out, n - 1, encoding=enc) == _lib.FRLW_ERR_ARG
    assert bool((out == 0x5A).all())
    # the right capacity on the same plan: the records, and nothing behind them
    assert raw_io.evt2_emit(dev, SIZE, ws, out, n, encoding=enc) == _lib.FRLW_OK
    assert_same_records(as_records(out[:n]), R.decode(words, SIZE[1], SIZE[0], enc)[0])
    assert bool((out[n:] == 0x5A).all())
    # other words behind the same plan: a chunk whose count differs writes nothing and says so
    other = words.copy()
    other[:40] = D.trigger(enc)
    n0 = R.decode(words[:C], SIZE[1], SIZE[0], enc, time_shift=False)[1]["events"]
    assert n0 > 200 and R.decode(other[:C], SIZE[1], SIZE[0], enc, time_shift=False)[1]["events"] != n0
    out.fill_(0x5A)
    assert raw_io.evt2_emit(to_dev(other, enc), SIZE, ws, out, n, encoding=enc) == _lib.FRLW_ERR_HIP
    assert bool((out[:200] == 0x5A).all())


# ---- carried state -----------------------------------------------------------------------------------------------------------
def test_split_calls(plan):
    enc, C, L = plan
    words = D.fuzz(3 * C + 17, 71, enc)
    H, W = SIZE
    want, want_c, _ = R.decode(words, W, H, enc)
    rng = np.random.default_rng(72)
    # a cut across which t steps back: the second call counts it only because the first call's last t is carried
    stepping = None
    for cut in range(int(rng.integers(C + 1, 2 * C)), 3 * C):
        st = R.decode(words[:cut], W, H, enc)[2]
        alone = R.decode(words[cut:], W, H, enc, state=dict(st, prev_t=None))[1]["unsorted"]
        if R.decode(words[cut:], W, H, enc, state=st)[1]["unsorted"] == alone + 1:
            stepping = cut
            break
    assert stepping is not None
    for cut in (1, L, C - 1, C, stepping):
        ra, rca, rs = R.decode(words[:cut], W, H, enc)
        a, ca, state = DECODE[enc](to_dev(words[:cut], enc), SIZE)
        assert_same_state(state, rs)
        b, cb, state2 = DECODE[enc](to_dev(words[cut:], enc), SIZE, state=state)
        rb, rcb, rs2 = R.decode(words[cut:], W, H, enc, state=rs)
        assert_same_state(state2, rs2)
        assert ca == rca and cb == rcb, cut
        assert (as_records(a).tobytes() + as_records(b).tobytes()) == want.tobytes(), cut
        for k in SUMMED:
            assert ca[k] + cb[k] == want_c[k], (cut, k)
        assert (cb["last_t"] if cb["events"] else ca["last_t"]) == want_c["last_t"]


# ---- fuzz --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_fuzz(plan, seed):
    """A stream built this way is never refused (the EVT_TIME_HIGH value never goes below the stream's first, and stays small):
    a refusal by the restatement raises inside check() and fails the test."""
    enc, C, L = plan
    words = D.fuzz(3 * C + 17, 1000 + seed, enc)
    for shift in (True, False):
        got, counters = check(words, enc, time_shift=shift)
        assert counters["events"] > 1000 and len(got) == counters["events"]
        for k in ("before_sync", "out_of_frame", "unsorted", "triggers", "other_words"):
            assert counters[k] > 0, k


def test_more_chunks_than_scan_threads(plan):
    """258 chunks and 17 words: each thread of the two single-workgroup scans has a range of two chunks, threads 0..129 have
    work, the ranges of the rest are clipped to nothing."""
    enc, C, L = plan
    words = D.fuzz(258 * C + 17, 1100, enc)
    assert -(-len(words) // C) > 256
    _, counters = check(words, enc)
    assert counters["events"] > 0 and counters["unsorted"] > 0 and counters["out_of_frame"] > 0


# ---- the three encodings -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def test_three_encodings_of_the_same_records(gpu):
    rec = synth.to_dat8(D.burst_events(n=4_000, t_span=50_000))
    a, _, _ = raw_io.decode_evt2(to_dev(raw_io.encode_evt2(rec), "EVT2"), D.BURST_SIZE, time_shift=False)
    b, _, _ = raw_io.decode_evt21(to_dev(raw_io.encode_evt21(rec), "EVT21"), D.BURST_SIZE, time_shift=False)
    w3 = torch.from_numpy(raw_io.encode_evt3(rec).view(np.int16).copy()).cuda()
    c, _, _ = raw_io.decode_evt3(w3, D.BURST_SIZE, time_shift=False)
    assert as_records(a).tobytes() == as_records(b).tobytes() == as_records(c).tobytes() == rec.tobytes()


@pytest.mark.parametrize("enc", raw_io.ENCODINGS)
def test_rawfile_end_to_end(gpu, enc, tmp_path, monkeypatch):
    from frlw_evd_amd import dat_io
    rec = synth.to_dat8(D.burst_events(n=6_000, t_span=60_000))
    path, dat_path = str(tmp_path / "r.raw"), str(tmp_path / "r_td.dat")
    raw_io.write_raw(path, rec, 240, 304, encoding=enc)
    f = raw_io.RawFile(path)
    dat, counters = f.decode()
    assert f.encoding == enc and as_records(dat).tobytes() == rec.tobytes() and f.total_time() == int(rec["t"][-1])
    assert counters["events"] == len(rec)
    assert raw_io.raw_to_dat(path, dat_path)["events"] == len(rec)
    back = dat_io.DatFile(dat_path)
    assert back.size == (240, 304) and np.array(back.records).tobytes() == rec.tobytes()
    # several pieces, the state carried from one to the next
    C = raw_io.geometry(enc)[0]
    monkeypatch.setattr(raw_io.RawFile, "PIECE_WORDS", C + 5)
    assert len(f) > (C + 5) + 10
    dat2, counters2 = raw_io.RawFile(path).decode()
    assert torch.equal(dat, dat2) and counters2 == counters


def test_detect_recording_takes_the_three_encodings(gpu, tmp_path):
    """detect_recording.py --raw on one synthetic GEN1-sized recording written in the three encodings: byte-identical box files."""
    from test_stream_detect_gpu import PERIOD, T_BEGIN, recording
    from frlw_evd_amd.yolox import build_yolox
    from frlw_evd_amd.yolox.model import recipe_state_dict
    rec = recording((240, 304), 21)
    net = build_yolox(16, 2)
    ck = str(tmp_path / "weights.pth")
    torch.save({"state_dict": {"module." + k: v for k, v in recipe_state_dict(net, seed=1004).items()}, "epoch": 0}, ck)
    outs = {}
    for enc in raw_io.ENCODINGS:
        path = str(tmp_path / (enc + ".raw"))
        raw_io.write_raw(path, rec, 240, 304, encoding=enc)
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
        out = str(tmp_path / ("boxes_" + enc))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "detect_recording.py"), "--raw", path, "--dataset", "gen1", "--exp_type", "yolox",
                            "--checkpoint", ck, "--event_volume_bins", "8", "--period", str(PERIOD), "--t_begin", str(T_BEGIN), "--out", out,
                            "--log_path", str(tmp_path) + "/"], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs[enc] = open(out + ".npy", "rb").read()
        assert "'events': {0}".format(len(rec)) in r.stdout and "'before_sync': 0" in r.stdout and "'out_of_frame': 0" in r.stdout
    assert outs["EVT2"] == outs["EVT3"] and outs["EVT21"] == outs["EVT3"] and len(outs["EVT3"]) > 200
