"""EVT 3.0 without a GPU: the restatement against a hand-decoded stream, the writer's round trip, the header parser, the state
record's algebra in a host program, the host-side checks of the C entry points and the command's parser."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import evt3_data as D
import evt3_restated as R
from frlw_evd_amd import _build, _lib, raw_io, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_decodes_the_hand_assembled_stream():
    """Ties tests/evt3_restated.py to the format table: ~40 literal words, every type once, records and counters written out."""
    assert len(D.HAND_WORDS) == 38 and set(int(w) >> 12 for w in D.HAND_WORDS) >= {0, 1, 2, 3, 4, 5, 6, 7, 8, 0xA, 0xE, 0xF}
    rec, counters, _ = R.decode(D.HAND_WORDS, D.HAND_SIZE[1], D.HAND_SIZE[0], time_shift=True)
    assert rec.tobytes() == D.records_of(D.HAND_EVENTS).tobytes()
    assert counters == D.HAND_COUNTERS
    # without the shift: the same records 0x110000 later
    rec0, counters0, _ = R.decode(D.HAND_WORDS, D.HAND_SIZE[1], D.HAND_SIZE[0], time_shift=False)
    assert (rec0["t"] == rec["t"] + 0x110000).all() and (rec0["_"] == rec["_"]).all()
    assert counters0["first_t"] == 0x110000 and counters0["last_t"] == 0x1000000


def test_restatement_carries_its_state():
    whole, cw, _ = R.decode(D.HAND_WORDS, 304, 240)
    for cut in (1, 10, 11, 22, 23, 31):
        a, ca, st = R.decode(D.HAND_WORDS[:cut], 304, 240)
        b, cb, _ = R.decode(D.HAND_WORDS[cut:], 304, 240, state=st)
        assert np.concatenate([a, b]).tobytes() == whole.tobytes()
        assert all(ca[k] + cb[k] == cw[k] for k in R.COUNTERS[:7])


def test_restatement_refuses_a_t_beyond_32_bits():
    words = [D.th(0), D.ay(0)] + [D.th(4095), D.th(0)] * 257 + [D.ax(1)]
    with pytest.raises(ValueError):
        R.decode(words, 304, 240)
    R.decode(words[:2 + 2 * 255] + [D.ax(1)], 304, 240)


def test_burst_stream_round_trip():
    """encode_evt3 -> restatement gives the records back byte for byte (time_shift off), and the stream is made of vectors."""
    ev = D.burst_events()
    rec = synth.to_dat8(ev)
    assert 19_000 <= len(rec) <= 21_000 and (np.diff(ev["t"]) >= 0).all()
    words = raw_io.encode_evt3(rec)
    assert words.dtype == np.uint16
    kinds = np.bincount(words >> 12, minlength=16)
    assert kinds[0x3] > 500 and kinds[0x4] > 500 and kinds[0x5] > 50 and kinds[0x2] > 5_000
    back, counters, _ = R.decode(words, 304, 240, time_shift=False)
    assert back.tobytes() == rec.tobytes()
    assert counters["events"] == len(rec) and counters["before_sync"] == counters["out_of_frame"] == counters["unsorted"] == 0
    # about half of the events travel in vector words
    in_vectors = len(rec) - kinds[0x2]
    assert 0.35 * len(rec) <= in_vectors <= 0.65 * len(rec)
    # with the shift: the stream opens with EVT_TIME_HIGH 0, so nothing moves
    assert words[0] == 0x8000 and R.decode(words, 304, 240, time_shift=True)[0].tobytes() == rec.tobytes()


def test_encoder_writes_clock_wraps_and_setters_on_change_only():
    t = np.array([5, 5, (1 << 24) - 1, 1 << 24, (3 << 24) + 0x5123], dtype=np.int64)
    rec = synth.to_dat8({"x": np.array([1, 2, 3, 4, 5]), "y": np.array([9, 9, 9, 9, 8]), "p": np.array([0, 0, 1, 1, 0]), "t": t})
    words = raw_io.encode_evt3(rec)
    back, counters, _ = R.decode(words, 304, 240, time_shift=False)
    assert back.tobytes() == rec.tobytes() and counters["time_loops"] == 3
    kinds = np.bincount(words >> 12, minlength=16)
    assert kinds[0x0] == 2 and kinds[0x6] == 4   # y: 9, 8; low: 5, 0xFFF, 0, 0x123
    with pytest.raises(ValueError):
        raw_io.encode_evt3(synth.to_dat8({"x": np.array([1, 2]), "y": np.array([1, 1]), "p": np.array([0, 0]),
                                          "t": np.array([100_000, 10], dtype=np.int64)}))


# ---- the header ------------------------------------------------------------------------------------------------------
def _write(path, header, payload=b""):
    with open(path, "wb") as f:
        f.write(header)
        f.write(payload)
    return str(path)


WORDS = np.array([0x8000, 0x0003, 0x2005], dtype="<u2").tobytes()


def test_header_old_style(tmp_path):
    p = _write(tmp_path / "a.raw", b"% date 2021-01-01 10:00:00\n% evt 3.0\n% geometry 1280x720\n% serial_number 0001\n", WORDS)
    off, size, fields = raw_io.parse_raw_header(p)
    assert size == (720, 1280) and fields["evt"] == "3.0" and off == os.path.getsize(p) - len(WORDS)
    f = raw_io.RawFile(p)
    assert f.size == (720, 1280) and f.words.tolist() == [0x8000, 0x0003, 0x2005]


def test_header_new_style_and_key_order(tmp_path):
    for fmt in (b"EVT3;height=720;width=1280", b"EVT3;width=1280;height=720"):
        # a '%' line behind '% end' belongs to the data
        p = _write(tmp_path / "b.raw", b"% camera_integrator_name Prophesee\n% format " + fmt + b"\n% end\n", b"%\n" + WORDS)
        off, size, fields = raw_io.parse_raw_header(p)
        assert size == (720, 1280) and off == os.path.getsize(p) - len(WORDS) - 2
        assert len(raw_io.RawFile(p)) == 4
    # '% format' wins over '% geometry'
    p = _write(tmp_path / "c.raw", b"% geometry 640x480\n% format EVT3;height=720;width=1280\n% end\n", WORDS)
    assert raw_io.parse_raw_header(p)[1] == (720, 1280)


def test_header_without_geometry(tmp_path):
    p = _write(tmp_path / "d.raw", b"% evt 3.0\n% end\n", WORDS)
    assert raw_io.parse_raw_header(p)[1] is None and raw_io.RawFile(p).size is None
    p = _write(tmp_path / "e.raw", b"% format EVT3\n% end\n", WORDS)
    assert raw_io.parse_raw_header(p)[1] is None


@pytest.mark.parametrize("header, found", [(b"% evt 2.0\n% geometry 640x480\n", "evt 2.0"),
                                           (b"% format EVT21;height=720;width=1280\n% end\n", "EVT21"),
                                           (b"% date 2021\n% end\n", "no encoding line"), (b"", "no encoding line")])
def test_header_refuses_other_encodings(tmp_path, header, found):
    p = _write(tmp_path / "f.raw", header, WORDS)
    with pytest.raises(ValueError, match=found):
        raw_io.parse_raw_header(p)


def test_header_empty_data_and_odd_trailing_byte(tmp_path):
    p = _write(tmp_path / "g.raw", b"% evt 3.0\n% geometry 304x240\n% end\n")
    f = raw_io.RawFile(p)
    assert len(f) == 0 and f.size == (240, 304)
    p = _write(tmp_path / "h.raw", b"% evt 3.0\n% geometry 304x240\n% end\n", WORDS + b"\x07")
    assert raw_io.RawFile(p).words.tolist() == [0x8000, 0x0003, 0x2005]


def test_write_raw_reads_back(tmp_path):
    rec = synth.to_dat8(D.burst_events(n=2_000))
    p = str(tmp_path / "w.raw")
    raw_io.write_raw(p, rec, 240, 304)
    f = raw_io.RawFile(p)
    assert f.size == (240, 304) and "end" in f.fields
    assert R.decode(np.array(f.words), 304, 240)[0].tobytes() == rec.tobytes()


# ---- the state record on the host ------------------------------------------------------------------------------------------
def _host_cxx():
    for name in ("c++", "g++", "clang++"):
        exe = shutil.which(name)
        if exe:
            return exe
    return None


def test_state_records_compose_associatively_under_asan_and_ubsan(tmp_path):
    """tests/host/evt3_state_check.cpp, built from csrc/evt3_state.h with the host compiler: random streams cut into runs of every
    length, composed left to right and as a balanced tree, against the summary of the whole stream and a sequential decoder."""
    exe = _host_cxx()
    assert exe, "no host C++ compiler (c++, g++, clang++)"
    prog = str(tmp_path / "evt3_state_check")
    cmd = [exe, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", _build.CSRC,
           os.path.join(ROOT, "tests", "host", "evt3_state_check.cpp"), "-o", prog]
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
def test_workspace_and_geometry_queries_are_host_only():
    lib = _lib.load()
    chunk, lane = raw_io.geometry()
    assert chunk % (64 * lane) == 0 and lane % 8 == 0 and chunk >= 1024      # whole wavefronts of 16-byte loads
    sizes = [lib.frlw_evt3_workspace_bytes(n) for n in (0, 1, chunk, chunk + 1, 100 * chunk, 1 << 27, 1 << 31)]
    assert sizes[0] >= 1024 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[1] and sizes[3] < sizes[4] < sizes[5] < sizes[6]
    assert sizes[-1] < (1 << 31) * 2 // 64          # the plan is a small fraction of the input
    assert lib.frlw_evt3_workspace_bytes(-1) == 0 and lib.frlw_evt3_workspace_bytes((1 << 31) + 1) == 0
    assert lib.frlw_evt3_geometry(None, None) == _lib.FRLW_ERR_ARG


def test_argument_checks_answer_without_a_gpu():
    lib = _lib.load()
    p = C.c_void_p(0x10000)      # never dereferenced: every answer below comes from the host-side checks
    need = lib.frlw_evt3_workspace_bytes(5000)

    def count(words=p, n=5000, w=304, h=240, state=None, ws=p, ws_bytes=need):
        return lib.frlw_evt3_count(words, n, w, h, state, ws, ws_bytes, None)

    def emit(words=p, n=5000, w=304, h=240, ws=p, ws_bytes=need, out=p, cap=10):
        return lib.frlw_evt3_emit(words, n, w, h, ws, ws_bytes, out, cap, 1, None)

    for call in (count, emit):
        assert call(words=None) == _lib.FRLW_ERR_ARG and call(ws=None) == _lib.FRLW_ERR_ARG and call(n=-1) == _lib.FRLW_ERR_ARG
        for bad in (0, 2049, -3):
            assert call(w=bad) == _lib.FRLW_ERR_ARG and call(h=bad) == _lib.FRLW_ERR_ARG
        assert call(ws_bytes=need - 1) == _lib.FRLW_ERR_WORKSPACE and call(ws_bytes=0) == _lib.FRLW_ERR_WORKSPACE
    assert emit(out=None) == _lib.FRLW_ERR_ARG and emit(cap=-1) == _lib.FRLW_ERR_ARG
    state = raw_io.FrlwEvt3State()
    assert C.sizeof(state) == 48 and state.struct_size == 48 and C.sizeof(raw_io.FrlwEvt3Counters) == 8 + 11 * 8
    state.struct_size = 40
    assert count(state=C.byref(state)) == _lib.FRLW_ERR_ARG
    counters = raw_io.FrlwEvt3Counters()
    counters.struct_size = 16
    assert lib.frlw_evt3_result(p, None, C.byref(counters), None, None) == _lib.FRLW_ERR_ARG
    assert lib.frlw_evt3_result(None, None, C.byref(raw_io.FrlwEvt3Counters()), None, None) == _lib.FRLW_ERR_ARG


# ---- the command's parser --------------------------------------------------------------------------------------------------
def test_detect_recording_parser_takes_dat_or_raw():
    import detect_recording as dr
    a = dr.build_parser().parse_args(["--raw", "x.raw", "--out", "y"])
    assert a.raw == "x.raw" and a.dat is None and dr.recording_source(a) == ("raw", "x.raw")
    b = dr.build_parser().parse_args(["--dat", "a_td.dat", "--dataset", "gen1", "--exp_type", "yolox", "--checkpoint", "c.pth",
                                      "--event_volume_bins", "8", "--period", "50000", "--out", "o", "--log_path", "l/"])
    assert b.dat == "a_td.dat" and b.raw is None and b.period == 50000 and dr.recording_source(b) == ("dat", "a_td.dat")
    for argv in (["--out", "y"], ["--dat", "a.dat", "--raw", "x.raw", "--out", "y"]):
        with pytest.raises(SystemExit):
            dr.build_parser().parse_args(argv)
    assert dr.frame_stem("d/rec_01.raw") == "rec_01" and dr.frame_stem("d/seq_td.dat") == "seq"


def test_no_kernel_of_evt3_has_scratch(tmp_path):
    """-Rpass-analysis=kernel-resource-usage with the project's flags: five kernels, none with a scratch byte."""
    import re
    flags = [f for f in _build.HIPCC_FLAGS if f != "-shared"]
    c = subprocess.run([_build.hipcc()] + flags + ["-I", _build.INCLUDE, "-I", _build.CSRC, "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(_build.CSRC, "evt3.hip"), "-o", str(tmp_path / "evt3.o")], capture_output=True, text=True, timeout=600)
    assert c.returncode == 0, c.stderr[-4000:]
    names = re.findall(r"Function Name: \S*?(k_evt_[a-z_]+)I\S*Evt3", c.stderr)    # the kernels of csrc/evt_plan.h, made for EVT 3.0
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", c.stderr)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", c.stderr)]
    assert sorted(names) == ["k_evt_count", "k_evt_emit", "k_evt_scan_counts", "k_evt_scan_states", "k_evt_summary"], names
    assert scratch == [0] * 5 and max(lds) <= 160 * 1024, (scratch, lds)
