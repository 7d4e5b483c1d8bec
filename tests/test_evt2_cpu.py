"""EVT 2.0 and EVT 2.1 without a GPU: the restatement against the hand-decoded streams and the literal clock streams, the writers'
round trips, the header reader for all three encodings, the state record's algebra in a host program, the host-side checks of the
C entry points and the resources of the kernels."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import evt2_data as D
import evt2_restated as R
import evt3_restated as R3
from frlw_evd_amd import _build, _lib, raw_io, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENCS = D.ENCODINGS
H, W = D.HAND_SIZE


# ---- the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("enc", ENCS)
def test_restatement_decodes_the_hand_assembled_stream(enc):
    """Ties tests/evt2_restated.py to the format tables: ~30 literal words, every type at least once, records and counters written
    out."""
    words = D.HAND_WORDS[enc]
    assert words.dtype == D.DTYPE[enc] and 25 <= len(words) <= 35
    bits = 60 if enc == "EVT21" else 28
    assert set(int(w) >> bits for w in words) >= {0x0, 0x1, 0x8, 0xA, 0xE, 0xF, 0x3}
    rec0, counters0, _ = R.decode(words, W, H, enc, time_shift=False)
    assert rec0.tobytes() == D.records_of(D.HAND_EVENTS[enc]).tobytes()
    assert counters0 == D.HAND_COUNTERS[enc]
    rec, counters, state = R.decode(words, W, H, enc, time_shift=True)
    assert rec.tobytes() == D.records_of(D.HAND_EVENTS[enc], D.HAND_SHIFT).tobytes()
    assert counters == D.shifted(D.HAND_COUNTERS[enc], D.HAND_SHIFT) and counters["first_t"] == 0
    assert state["first_high"] == 0x11 and state["high"] == 0x31


def test_the_two_hand_streams_say_the_same_where_they_can():
    """An EVT 2.0 word is the upper half of an EVT 2.1 word with the one-bit mask: the same stream in both widths, same decode."""
    wide = (D.HAND_WORDS["EVT2"].astype(np.uint64) << np.uint64(32)) | np.uint64(1)
    a = R.decode(D.HAND_WORDS["EVT2"], W, H, "EVT2")
    b = R.decode(wide, W, H, "EVT21")
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1]


@pytest.mark.parametrize("enc", ENCS)
def test_restatement_carries_its_state(enc):
    words = D.HAND_WORDS[enc]
    whole, cw, _ = R.decode(words, W, H, enc)
    for cut in (1, 2, 3, 10, 15, 16, 20, 27):
        a, ca, st = R.decode(words[:cut], W, H, enc, time_shift=False)
        b, cb, st2 = R.decode(words[cut:], W, H, enc, time_shift=False, state=st)
        both = np.concatenate([a, b])
        both["t"] -= D.HAND_SHIFT
        assert both.tobytes() == whole.tobytes(), cut
        assert all(ca[k] + cb[k] == cw[k] for k in R.COUNTERS[:7]), cut
        assert st2["first_high"] == 0x11


@pytest.mark.parametrize("enc", ENCS)
def test_literal_streams_pin_the_clock(enc):
    s = D.clock_streams(enc)
    rec, counters, _ = R.decode(s["wrap"], W, H, enc)
    assert rec["t"].tolist() == [63, 64] and counters["time_loops"] == 1 and counters["unsorted"] == 0
    with pytest.raises(ValueError):
        R.decode(s["wrap"], W, H, enc, time_shift=False)      # unshifted these t need 35 bits
    for shift in (True, False):
        with pytest.raises(ValueError):
            R.decode(s["beyond"], W, H, enc, time_shift=shift)
        rec, counters, _ = R.decode(s["edge"], W, H, enc, time_shift=shift)
        assert rec["t"].tolist() == [0, (1 << 32) - 1] and counters["time_loops"] == 0 and counters["last_t"] == (1 << 32) - 1


@pytest.mark.parametrize("enc", ENCS)
def test_slack_rule(enc):
    ev = D.cd(1, 1, 0, 0, enc)
    assert R.decode([D.th(100, enc), D.th(90, enc)], W, H, enc)[1]["time_loops"] == 0
    assert R.decode([D.th(100, enc), D.th(89, enc)], W, H, enc)[1]["time_loops"] == 1
    # a backward step right behind the first EVT_TIME_HIGH: negative behind the shift
    with pytest.raises(ValueError):
        R.decode([D.th(100, enc), D.th(95, enc), ev], W, H, enc)
    rec, _, _ = R.decode([D.th(100, enc), D.th(95, enc), ev], W, H, enc, time_shift=False)
    assert rec["t"].tolist() == [95 << 6]


# ---- the writers -------------------------------------------------------------------------------------------------------------
ENCODERS = {"EVT2": raw_io.encode_evt2, "EVT21": raw_io.encode_evt21}


@pytest.mark.parametrize("enc", ENCS)
def test_burst_stream_round_trip(enc):
    """encode -> restatement gives the records back byte for byte (time_shift off, and on: the stream opens with EVT_TIME_HIGH 0)."""
    ev = D.burst_events()
    rec = synth.to_dat8(ev)
    assert 19_000 <= len(rec) <= 21_000 and (np.diff(ev["t"]) >= 0).all()
    words = ENCODERS[enc](rec)
    assert words.dtype == D.DTYPE[enc]
    hi = (words >> np.uint64(32)).astype(np.uint32) if enc == "EVT21" else words
    assert hi[0] == 0x80000000
    kinds = np.bincount(hi >> 28, minlength=16)
    n_high = len(np.unique(np.concatenate([[0], ev["t"] >> 6]))) - 1     # t ascends: one EVT_TIME_HIGH per new value of t >> 6
    assert kinds[0x8] == 1 + n_high and kinds[0] + kinds[1] + kinds[0x8] == len(words)
    for shift in (False, True):
        back, counters, _ = R.decode(words, W, H, enc, time_shift=shift)
        assert back.tobytes() == rec.tobytes()
        assert counters["events"] == len(rec) and counters["before_sync"] == counters["out_of_frame"] == counters["unsorted"] == 0
    if enc == "EVT2":
        assert kinds[0] + kinds[1] == len(rec)
    else:
        # the bursts travel as vectors: a good share of the events in words of two bits and more
        masks = (words & np.uint64(0xFFFFFFFF))[(hi >> 28) <= 1]
        pop = np.array([bin(int(m)).count("1") for m in masks])
        assert pop.sum() == len(rec) and pop.min() >= 1
        assert pop[pop >= 2].sum() >= 0.25 * len(rec), pop[pop >= 2].sum()
        assert (((hi[(hi >> 28) <= 1] >> 11) & 0x7FF) % 32 == 0).all()


@pytest.mark.parametrize("enc", ENCS)
def test_writers_refuse_what_the_decoder_would_not_give_back(enc):
    def rec(t, x=(1, 2), y=(1, 1)):
        return synth.to_dat8({"x": np.array(x), "y": np.array(y), "p": np.array([0, 1]), "t": np.array(t, dtype=np.int64)})
    with pytest.raises(ValueError, match="slack"):
        ENCODERS[enc](rec([100_000, 10]))
    with pytest.raises(ValueError, match="11 bits"):
        ENCODERS[enc](rec([1, 2], x=(1, 2048)))
    with pytest.raises(ValueError, match="11 bits"):
        ENCODERS[enc](rec([1, 2], y=(2048, 1)))
    # a step back inside the slack (10 units of 64 us) is written as it is and decoded as it is
    r = rec([64 * 50 + 3, 64 * 40 + 1])
    back, counters, _ = R.decode(ENCODERS[enc](r), W, H, enc, time_shift=False)
    assert back.tobytes() == r.tobytes() and counters["unsorted"] == 1 and counters["time_loops"] == 0
    # no record: the opening EVT_TIME_HIGH alone
    empty = ENCODERS[enc](synth.to_dat8({k: np.zeros(0, np.int64) for k in "xypt"}))
    assert len(empty) == 1 and R.decode(empty, W, H, enc)[1]["events"] == 0


def test_evt21_writer_packs_only_what_one_word_holds():
    """Equal (t, y, p) and strictly ascending x inside one 32-aligned block share a word; anything else opens a new one."""
    x = np.array([30, 31, 32, 33, 33, 40, 39, 41, 41])
    y = np.array([5, 5, 5, 5, 5, 5, 5, 6, 6])
    p = np.array([1, 1, 1, 1, 1, 1, 1, 1, 0])
    t = np.array([9, 9, 9, 9, 9, 9, 9, 9, 9], dtype=np.int64)
    rec = synth.to_dat8({"x": x, "y": y, "p": p, "t": t})
    words = raw_io.encode_evt21(rec)
    masks = [int(w) & 0xFFFFFFFF for w in words[1:]]
    # [30, 31] | [32, 33] | [33, 40] | [39] | [41] (y) | [41] (p)
    assert masks == [0xC0000000, 0x3, (1 << 1) | (1 << 8), 1 << 7, 1 << 9, 1 << 9]
    assert R.decode(words, W, H, "EVT21", time_shift=False)[0].tobytes() == rec.tobytes()


def test_the_three_encodings_of_the_same_records_decode_to_the_same_bytes():
    rec = synth.to_dat8(D.burst_events(n=3_000))
    a = R.decode(raw_io.encode_evt2(rec), W, H, "EVT2", time_shift=False)[0]
    b = R.decode(raw_io.encode_evt21(rec), W, H, "EVT21", time_shift=False)[0]
    c = R3.decode(raw_io.encode_evt3(rec), W, H, time_shift=False)[0]
    assert a.tobytes() == b.tobytes() == c.tobytes() == rec.tobytes()


# ---- the header --------------------------------------------------------------------------------------------------------------
def _write(path, header, payload=b""):
    with open(path, "wb") as f:
        f.write(header)
        f.write(payload)
    return str(path)


PAYLOAD = bytes(range(1, 25))      # 24 bytes: 12 / 6 / 3 words
OLD_STYLE = {"EVT2": b"2.0", "EVT21": b"2.1", "EVT3": b"3.0"}
N_WORDS = {"EVT2": 6, "EVT21": 3, "EVT3": 12}
WORD_DTYPE = {"EVT2": "<u4", "EVT21": "<u8", "EVT3": "<u2"}


@pytest.mark.parametrize("enc", raw_io.ENCODINGS)
def test_raw_header_old_and_new_style(tmp_path, enc):
    p = _write(tmp_path / "a.raw", b"% date 2021-01-01 10:00:00\n% evt " + OLD_STYLE[enc] + b"\n% geometry 1280x720\n% serial_number 0001\n", PAYLOAD)
    off, size, fields, got = raw_io.raw_header(p)
    assert got == enc and size == (720, 1280) and fields["evt"] == OLD_STYLE[enc].decode() and off == os.path.getsize(p) - len(PAYLOAD)
    f = raw_io.RawFile(p)
    assert f.encoding == enc and f.size == (720, 1280) and f.words.dtype == np.dtype(WORD_DTYPE[enc]) and len(f) == N_WORDS[enc]
    assert f.words.tobytes() == PAYLOAD
    name = enc.encode()
    for fmt in (name + b";height=720;width=1280", name + b";width=1280;height=720", name + b";sensor=x;width=1280;endianness=little;height=720"):
        # a '%' line behind '% end' belongs to the data
        p = _write(tmp_path / "b.raw", b"% camera_integrator_name Prophesee\n% format " + fmt + b"\n% end\n", b"%\n" + PAYLOAD)
        off, size, fields, got = raw_io.raw_header(p)
        assert got == enc and size == (720, 1280) and off == os.path.getsize(p) - len(PAYLOAD) - 2
    # '% format' wins over '% geometry' and names the encoding without a '% evt' line
    p = _write(tmp_path / "c.raw", b"% geometry 640x480\n% format " + name + b";height=720;width=1280\n% end\n", PAYLOAD)
    assert raw_io.raw_header(p)[1] == (720, 1280) and raw_io.raw_header(p)[3] == enc
    # no geometry
    for header in (b"% evt " + OLD_STYLE[enc] + b"\n% end\n", b"% format " + name + b"\n% end\n", b"% format " + name + b";height=720\n% end\n"):
        p = _write(tmp_path / "d.raw", header, PAYLOAD)
        assert raw_io.raw_header(p)[1] is None and raw_io.RawFile(p).size is None and raw_io.raw_header(p)[3] == enc


@pytest.mark.parametrize("header, found", [(b"% format EVT21;height=720;width=1280;endianness=legacy\n% end\n", "endianness=legacy"),
                                           (b"% format EVT21;endianness=legacy;height=720;width=1280\n% end\n", "endianness=legacy"),
                                           (b"% format EVT4;height=720;width=1280\n% end\n", "format EVT4"),
                                           (b"% evt 4.0\n% geometry 640x480\n", "evt 4.0"),
                                           (b"% date 2021\n% end\n", "no encoding line"), (b"", "no encoding line")])
def test_raw_header_refusals(tmp_path, header, found):
    p = _write(tmp_path / "f.raw", header, PAYLOAD)
    with pytest.raises(ValueError, match=found):
        raw_io.raw_header(p)
    with pytest.raises(ValueError):
        raw_io.RawFile(p)


def test_parse_raw_header_still_takes_evt3_alone(tmp_path):
    p = _write(tmp_path / "g.raw", b"% evt 2.0\n% geometry 640x480\n", PAYLOAD)
    with pytest.raises(ValueError, match="evt 2.0"):
        raw_io.parse_raw_header(p)
    assert raw_io.raw_header(p)[3] == "EVT2"


@pytest.mark.parametrize("enc", raw_io.ENCODINGS)
def test_write_raw_reads_back(tmp_path, enc):
    rec = synth.to_dat8(D.burst_events(n=2_000))
    p = str(tmp_path / "w.raw")
    raw_io.write_raw(p, rec, 240, 304, encoding=enc)
    words = {"EVT2": raw_io.encode_evt2, "EVT21": raw_io.encode_evt21, "EVT3": raw_io.encode_evt3}[enc](rec)
    f = raw_io.RawFile(p)
    assert f.encoding == enc and f.size == (240, 304) and "end" in f.fields and f.fields["format"].startswith(enc + ";")
    assert f.words.dtype == np.dtype(WORD_DTYPE[enc]) and len(f) == len(words) and np.array_equal(np.array(f.words), words)
    decode = (lambda w: R3.decode(w, 304, 240)) if enc == "EVT3" else (lambda w: R.decode(w, 304, 240, enc))
    assert decode(np.array(f.words))[0].tobytes() == rec.tobytes()
    # trailing bytes that do not fill a word are ignored
    with open(p, "ab") as g:
        g.write(b"\x07" * (np.dtype(WORD_DTYPE[enc]).itemsize - 1))
    f2 = raw_io.RawFile(p)
    assert len(f2) == len(words) and np.array_equal(np.array(f2.words), words)


def test_write_raw_default_is_evt3(tmp_path):
    rec = synth.to_dat8(D.burst_events(n=500))
    a, b = str(tmp_path / "a.raw"), str(tmp_path / "b.raw")
    raw_io.write_raw(a, rec, 240, 304)
    raw_io.write_raw(b, rec, 240, 304, encoding="EVT3")
    assert open(a, "rb").read() == open(b, "rb").read() and raw_io.RawFile(a).encoding == "EVT3"
    with pytest.raises(ValueError):
        raw_io.write_raw(a, rec, 240, 304, encoding="EVT4")


# ---- the state record on the host ------------------------------------------------------------------------------------------
def _host_cxx():
    for name in ("c++", "g++", "clang++"):
        exe = shutil.which(name)
        if exe:
            return exe
    return None


def test_state_records_compose_associatively_under_asan_and_ubsan(tmp_path):
    """tests/host/evt2_state_check.cpp, built from csrc/evt2_state.h with the host compiler and run as a stand-alone program."""
    exe = _host_cxx()
    assert exe, "no host C++ compiler (c++, g++, clang++)"
    prog = str(tmp_path / "evt2_state_check")
    cmd = [exe, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", _build.CSRC,
           os.path.join(ROOT, "tests", "host", "evt2_state_check.cpp"), "-o", prog]
    c = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True, timeout=300)
    if c.returncode != 0:
        c = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr[-4000:]
    r = subprocess.run([prog], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "300 streams" in r.stdout and " 0 failed" in r.stdout, r.stdout


# ---- the C entry points, host side -----------------------------------------------------------------------------------------
ARG = {"EVT2": _lib.EVT_20, "EVT21": _lib.EVT_21}


@pytest.mark.parametrize("enc", ENCS)
def test_workspace_and_geometry_queries_are_host_only(enc):
    lib = _lib.load()
    chunk, lane = raw_io.geometry(enc)
    word_bytes = 4 if enc == "EVT2" else 8
    assert chunk % (64 * lane) == 0 and (lane * word_bytes) % 16 == 0 and chunk * word_bytes >= 4096    # whole wavefronts of 16-byte loads
    sizes = [lib.frlw_evt2_workspace_bytes(ARG[enc], n) for n in (0, 1, chunk, chunk + 1, 100 * chunk, 1 << 27, 1 << 31)]
    assert sizes[0] >= 1024 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[1] and sizes[3] < sizes[4] < sizes[5] < sizes[6]
    assert sizes[-1] < (1 << 31) * word_bytes // 64          # the plan is a small fraction of the input
    assert lib.frlw_evt2_workspace_bytes(ARG[enc], -1) == 0 and lib.frlw_evt2_workspace_bytes(ARG[enc], (1 << 31) + 1) == 0
    assert lib.frlw_evt2_geometry(ARG[enc], None, None) == _lib.FRLW_ERR_ARG


def test_geometry_default_and_unknown_encoding():
    lib = _lib.load()
    c, l = C.c_int(0), C.c_int(0)
    assert lib.frlw_evt3_geometry(C.byref(c), C.byref(l)) == 0 and raw_io.geometry() == raw_io.geometry("EVT3") == (c.value, l.value)
    assert raw_io.geometry("EVT2")[1] == 2 * raw_io.geometry("EVT21")[1]     # the same bytes per lane piece
    for bad in (0, 3, 30):
        assert lib.frlw_evt2_geometry(bad, C.byref(c), C.byref(l)) == _lib.FRLW_ERR_ARG and lib.frlw_evt2_workspace_bytes(bad, 100) == 0
    with pytest.raises(ValueError):
        raw_io.geometry("EVT4")


@pytest.mark.parametrize("enc", ENCS)
def test_argument_checks_answer_without_a_gpu(enc):
    lib = _lib.load()
    p = C.c_void_p(0x10000)      # never dereferenced: every answer below comes from the host-side checks
    need = lib.frlw_evt2_workspace_bytes(ARG[enc], 5000)

    def count(e=ARG[enc], words=p, n=5000, w=304, h=240, state=None, ws=p, ws_bytes=need):
        return lib.frlw_evt2_count(e, words, n, w, h, state, ws, ws_bytes, None)

    def emit(e=ARG[enc], words=p, n=5000, w=304, h=240, ws=p, ws_bytes=need, out=p, cap=10):
        return lib.frlw_evt2_emit(e, words, n, w, h, ws, ws_bytes, out, cap, 1, None)

    for call in (count, emit):
        assert call(words=None) == _lib.FRLW_ERR_ARG and call(ws=None) == _lib.FRLW_ERR_ARG and call(n=-1) == _lib.FRLW_ERR_ARG
        assert call(n=(1 << 31) + 1, ws_bytes=1 << 40) == _lib.FRLW_ERR_ARG and call(e=3) == _lib.FRLW_ERR_ARG
        assert call(words=C.c_void_p(0x10002)) == _lib.FRLW_ERR_ARG                 # not aligned to a word
        for bad in (0, 2049, -3):
            assert call(w=bad) == _lib.FRLW_ERR_ARG and call(h=bad) == _lib.FRLW_ERR_ARG
        assert call(ws_bytes=need - 1) == _lib.FRLW_ERR_WORKSPACE and call(ws_bytes=0) == _lib.FRLW_ERR_WORKSPACE
    assert emit(out=None) == _lib.FRLW_ERR_ARG and emit(cap=-1) == _lib.FRLW_ERR_ARG
    state = raw_io.FrlwEvt2State()
    assert C.sizeof(state) == 40 and state.struct_size == 40 and state.shift() == 0
    state.flags, state.first_high = 1, 5
    assert state.shift() == 5 << 6
    state.struct_size = 48
    assert count(state=C.byref(state)) == _lib.FRLW_ERR_ARG
    counters = raw_io.FrlwEvt3Counters()
    counters.struct_size = 16
    assert lib.frlw_evt2_result(p, None, C.byref(counters), None, None) == _lib.FRLW_ERR_ARG
    assert lib.frlw_evt2_result(None, None, C.byref(raw_io.FrlwEvt3Counters()), None, None) == _lib.FRLW_ERR_ARG
    assert lib.frlw_evt2_result(p, None, C.byref(raw_io.FrlwEvt3Counters()), C.byref(state), None) == _lib.FRLW_ERR_ARG
    # the records the EVT 3.0 decoder shares or keeps are as they were
    assert C.sizeof(raw_io.FrlwEvt3State) == 48 and C.sizeof(raw_io.FrlwEvt3Counters) == 96


# ---- the kernels' resources ------------------------------------------------------------------------------------------------
def test_no_kernel_of_evt2_has_scratch(tmp_path):
    """-Rpass-analysis=kernel-resource-usage with the project's flags: the three per-chunk kernels once per encoding and the two
    scans, none with a scratch byte."""
    flags = [f for f in _build.HIPCC_FLAGS if f != "-shared"]
    c = subprocess.run([_build.hipcc()] + flags + ["-I", _build.INCLUDE, "-I", _build.CSRC, "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(_build.CSRC, "evt2.hip"), "-o", str(tmp_path / "evt2.o")], capture_output=True, text=True, timeout=600)
    assert c.returncode == 0, c.stderr[-4000:]
    names = re.findall(r"Function Name: \S*?(k_evt_[a-z_]+)I\S*Evt2", c.stderr)    # the kernels of csrc/evt_plan.h, made for EVT 2.x
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", c.stderr)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", c.stderr)]
    assert sorted(names) == sorted(["k_evt_count", "k_evt_emit", "k_evt_summary"] * 2 + ["k_evt_scan_counts", "k_evt_scan_states"]), names
    assert scratch == [0] * 8 and max(lds) <= 160 * 1024, (scratch, lds)


def test_detect_recording_names_the_three_encodings():
    import detect_recording as dr
    text = dr.__doc__ + dr.build_parser().format_help()
    assert "EVT 2.0" in text and "EVT 2.1" in text and "EVT 3.0" in text
