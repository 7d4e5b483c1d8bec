"""Prophesee ``.raw`` recordings in the EVT 2.0, EVT 2.1 and EVT 3.0 encodings: header, GPU decode to DAT8 records, and writers for
tests and tools.

The formats as this project implements them are DESIGN.md's "EVT 3.0 decode" and "EVT 2.0 and EVT 2.1 decode" sections (written
from the public descriptions; agreement with the vendor's decoder is unmeasured).  The decode runs on the GPU (csrc/evt3.hip through
``frlw_evt3_count`` / ``frlw_evt3_emit``, csrc/evt2.hip through ``frlw_evt2_count`` / ``frlw_evt2_emit``, both on the plan of
csrc/evt_plan.h) and returns what
``dat_io.DatFile.to_device`` returns: ``(n, 8)`` uint8 records, ``t:u32`` then ``x | y << 14 | p << 28``, so every encoder,
``StreamDetector`` and the renderer take a camera-native recording as they take a ``*_td.dat`` one.  There is no CPU decode here;
``encode_evt2`` / ``encode_evt21`` / ``encode_evt3`` / ``write_raw`` are host-only numpy.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib
from .synth import DAT_DTYPE, from_dat8

ADDR_Y, ADDR_X, VECT_BASE_X, VECT_12, VECT_8, TIME_LOW, TIME_HIGH = 0x0, 0x2, 0x3, 0x4, 0x5, 0x6, 0x8
COUNTERS = ("events", "before_sync", "out_of_frame", "triggers", "other_words", "time_loops", "unsorted", "first_t", "last_t")
_SUMMED = COUNTERS[:7]
MAX_CALL_WORDS = 1 << 31


# ---- the file ------------------------------------------------------------------------------------------------------
def _header_lines(path):
    """-> ``(offset of the first word, fields)``: ``fields`` maps the first token of every header line to the rest of it."""
    fields = {}
    with open(path, "rb") as f:
        while True:
            offset = f.tell()
            if f.read(1) != b"%":
                break
            line = (b"%" + f.readline()).decode("latin-1").strip()
            offset = f.tell()
            tokens = line[1:].split(None, 1)
            if tokens:
                fields[tokens[0]] = tokens[1].strip() if len(tokens) > 1 else ""
            if line[1:].strip() == "end":
                break
    return offset, fields


def _header_geometry(fields):
    """``(height, width)`` from the ``height=`` / ``width=`` pairs of ``% format`` if both are there, else from ``% geometry WxH``,
    else None."""
    pairs = dict(kv.split("=", 1) for kv in fields.get("format", "").split(";")[1:] if "=" in kv)
    if "height" in pairs and "width" in pairs:
        return (int(pairs["height"]), int(pairs["width"]))
    if "geometry" in fields and "x" in fields["geometry"]:
        w, h = fields["geometry"].lower().split("x", 1)
        return (int(h), int(w))
    return None


def parse_raw_header(path):
    """-> ``(offset of the first word, (height, width) or None, fields)``.  Header lines start with ``%``; the header ends behind a
    line ``% end`` or in front of the first line that does not start with ``%``.  ``fields`` maps the first token of every line to
    the rest of it.  The geometry comes from ``% format EVT3;height=H;width=W`` (key=value pairs in any order), else from
    ``% geometry WxH``.  ``ValueError`` unless ``% evt 3.0`` or ``format EVT3`` announces the encoding (``raw_header`` takes the
    other two encodings as well)."""
    offset, fields = _header_lines(path)
    fmt_name = fields.get("format", "").split(";")[0].strip()
    if not (fields.get("evt") == "3.0" or fmt_name == "EVT3"):
        found = ("format " + fmt_name) if fmt_name else (("evt " + fields["evt"]) if "evt" in fields else "no encoding line")
        raise ValueError(f"{path}: only EVT 3.0 recordings are decoded ('% evt 3.0' or '% format EVT3'); found: {found}")
    # ('% evt 3.0' beside a '% format' of another name: that line's pairs are not taken)
    size = _header_geometry(fields if fmt_name == "EVT3" else {k: v for k, v in fields.items() if k != "format"})
    return offset, size, fields


ENCODINGS = ("EVT2", "EVT21", "EVT3")
_EVT_LINE = {"2.0": "EVT2", "2.1": "EVT21", "3.0": "EVT3"}
_WORD_DTYPE = {"EVT2": "<u4", "EVT21": "<u8", "EVT3": "<u2"}


def raw_header(path):
    """-> ``(offset of the first word, (height, width) or None, fields, encoding)`` with ``encoding`` in ``ENCODINGS``: announced by
    ``% format EVT2|EVT21|EVT3[;...]``, else by ``% evt 2.0|2.1|3.0``.  Header rules and geometry as ``parse_raw_header``.
    ``ValueError`` naming what was found for anything else, and for ``endianness=legacy`` (EVT 2.1 with its 32-bit halves
    swapped), which is not guessed."""
    offset, fields = _header_lines(path)
    fmt = fields.get("format", "")
    fmt_name = fmt.split(";")[0].strip()
    if fmt_name:
        encoding = fmt_name if fmt_name in ENCODINGS else None
        found = "format " + fmt_name
    else:
        encoding = _EVT_LINE.get(fields.get("evt"))
        found = ("evt " + fields["evt"]) if "evt" in fields else "no encoding line"
    if encoding is None:
        raise ValueError(f"{path}: EVT 2.0, EVT 2.1 and EVT 3.0 recordings are decoded ('% evt 2.0|2.1|3.0' or "
                         f"'% format EVT2|EVT21|EVT3'); found: {found}")
    if any(kv.strip().replace(" ", "") == "endianness=legacy" for kv in fmt.split(";")[1:]):
        raise ValueError(f"{path}: '% format {fmt_name}' with endianness=legacy (32-bit halves swapped) is not decoded")
    return offset, _header_geometry(fields), fields, encoding


def write_raw(path, records, height, width, encoding="EVT3"):
    """Write DAT8 ``records`` as a ``.raw`` file in ``encoding`` (``% format EVT3;height=..;width=..`` ... ``% end``, then the
    words)."""
    if encoding not in ENCODINGS:
        raise ValueError(f"encoding: one of {ENCODINGS}, not {encoding!r}")
    words = {"EVT2": encode_evt2, "EVT21": encode_evt21, "EVT3": encode_evt3}[encoding](records)
    evt_line = {v: k for k, v in _EVT_LINE.items()}[encoding]
    with open(path, "wb") as f:
        f.write(f"% camera_integrator_name frlw_evd_amd\n% date 2020-01-01 00:00:00\n% evt {evt_line}\n".encode())
        f.write(f"% format {encoding};height={int(height)};width={int(width)}\n% geometry {int(width)}x{int(height)}\n% end\n".encode())
        f.write(words.astype(_WORD_DTYPE[encoding]).tobytes())


# ---- the writer ----------------------------------------------------------------------------------------------------
def encode_evt3(records) -> np.ndarray:
    """DAT8 records -> EVT 3.0 words (uint16), decoded back to the same records by the decoder with ``time_shift=False``.

    The stream opens with EVT_TIME_HIGH 0, so a decoder that shifts by the first EVT_TIME_HIGH keeps the timestamps too.
    EVT_TIME_HIGH, EVT_TIME_LOW and EVT_ADDR_Y are written only on change.  A run of two or more events of equal ``(t, y, p)`` whose x
    ascends by steps below 12 becomes VECT_BASE_X plus VECT_12 words (the last one a VECT_8 when its bits fit), every other event an
    EVT_ADDR_X.  Clock wraps (t crossing a multiple of 2^24) are written as EVT_TIME_HIGH 4095, 0.  t may step back only inside the
    decoder's no-wrap slack (at most 10 EVT_TIME_HIGH units, 40.96 ms); x and y must fit 11 bits."""
    rec = np.ascontiguousarray(records)
    if rec.dtype != DAT_DTYPE:
        rec = rec.view(DAT_DTYPE).reshape(-1)
    ev = from_dat8(rec)
    t, x, y, p = ev["t"], ev["x"], ev["y"], ev["p"]
    n = len(t)
    if n == 0:
        return np.array([TIME_HIGH << 12], dtype=np.uint16)
    if int(x.max()) > 2047 or int(y.max()) > 2047:
        raise ValueError("EVT 3.0 addresses have 11 bits")
    # runs: equal (t, y, p), x ascending by less than 12
    cont = np.zeros(n, bool)
    cont[1:] = (t[1:] == t[:-1]) & (y[1:] == y[:-1]) & (p[1:] == p[:-1]) & (x[1:] > x[:-1]) & (x[1:] - x[:-1] < 12)
    run_of = np.cumsum(~cont) - 1
    run_len = np.bincount(run_of)
    run_first = np.flatnonzero(~cont)
    # groups: a vector run, or a single event (runs of one)
    g_t, g_y, g_p, g_x = t[run_first], y[run_first], p[run_first], x[run_first]
    is_vec = run_len >= 2
    last_x = x[run_first + run_len - 1]
    n_vec_words = np.where(is_vec, (last_x - g_x) // 12 + 1, 0)
    high, low, loops = (g_t >> 12) & 0xFFF, g_t & 0xFFF, g_t >> 24
    prev_high = np.concatenate([[0], high[:-1]])
    prev_loops = np.concatenate([[0], loops[:-1]])
    d_loops = loops - prev_loops
    if (d_loops < 0).any() or ((d_loops == 0) & (high + 10 < prev_high)).any():
        raise ValueError("t steps back by more than the decoder's no-wrap slack (10 EVT_TIME_HIGH units)")
    # after a wrap sequence (4095, 0 per loop) the clock reads 0
    n_high = 2 * d_loops + (high != np.where(d_loops > 0, 0, prev_high))
    n_low = np.ones(len(g_t), np.int64)
    n_low[1:] = low[1:] != low[:-1]
    n_y = np.ones(len(g_t), np.int64)
    n_y[1:] = g_y[1:] != g_y[:-1]
    body = np.where(is_vec, 1 + n_vec_words, 1)
    total = n_high + n_low + n_y + body
    start = 1 + np.cumsum(total) - total                       # word 0: EVT_TIME_HIGH 0
    words = np.zeros(1 + int(total.sum()), dtype=np.uint16)
    words[0] = TIME_HIGH << 12
    # time high: the common case is one word; wraps (one per 16.8 s) are written group by group
    plain = (d_loops == 0) & (n_high == 1)
    words[start[plain]] = (TIME_HIGH << 12) | high[plain]
    for g in np.flatnonzero(d_loops > 0):
        seq = [4095, 0] * int(d_loops[g]) + ([int(high[g])] if high[g] != 0 else [])
        words[start[g]:start[g] + len(seq)] = (TIME_HIGH << 12) | np.array(seq, dtype=np.int64)
    at = start + n_high
    m = n_low == 1
    words[at[m]] = (TIME_LOW << 12) | low[m]
    at = at + n_low
    m = n_y == 1
    words[at[m]] = (ADDR_Y << 12) | g_y[m]
    at = at + n_y
    single = ~is_vec
    words[at[single]] = (ADDR_X << 12) | (g_p[single] << 11) | g_x[single]
    words[at[is_vec]] = (VECT_BASE_X << 12) | (g_p[is_vec] << 11) | g_x[is_vec]
    # the vector words: one token per (run, 12-pixel window), its mask the OR (= sum: the bits differ) of its events' bits
    in_vec = is_vec[run_of]
    if in_vec.any():
        rel = x[in_vec] - g_x[run_of[in_vec]]
        token = (at[run_of[in_vec]] + 1 + rel // 12).astype(np.int64)   # the word's position in the stream
        masks = np.bincount(token, weights=(1 << (rel % 12)).astype(np.float64)).astype(np.int64)
        pos = np.flatnonzero(masks)
        words[pos] = (VECT_12 << 12) | masks[pos]
        # the last word of a run as VECT_8 when no bit above 7 is set
        last_pos = (at + n_vec_words)[is_vec]
        narrow = last_pos[masks[last_pos] < 256]
        words[narrow] = (VECT_8 << 12) | masks[narrow]
    return words


def _evt2_fields(records):
    rec = np.ascontiguousarray(records)
    if rec.dtype != DAT_DTYPE:
        rec = rec.view(DAT_DTYPE).reshape(-1)
    ev = from_dat8(rec)
    t, x, y, p = (ev[k].astype(np.int64) for k in ("t", "x", "y", "p"))
    if len(t) and (int(x.max()) > 2047 or int(y.max()) > 2047):
        raise ValueError("EVT 2.0 / EVT 2.1 addresses have 11 bits")
    return t, x, y, p


def _evt2_interleave(high, body, type_shift, dtype):
    """The words of an EVT 2.x stream: EVT_TIME_HIGH 0 first, then per group (``high``: its t >> 6, ``body``: its event word) an
    EVT_TIME_HIGH where the value differs from the one in force, and the event word."""
    prev = np.concatenate([[0], high[:-1]])
    if (high + 10 < prev).any():
        raise ValueError("t steps back by more than the decoder's no-wrap slack (10 EVT_TIME_HIGH units)")
    n_high = (high != prev).astype(np.int64)
    at = 1 + np.cumsum(n_high + 1) - 1                        # position of each group's event word (word 0: EVT_TIME_HIGH 0)
    words = np.zeros(1 + len(high) + int(n_high.sum()), dtype=dtype)
    th = np.array(TIME_HIGH, dtype=dtype) << dtype(type_shift + 28)
    words[0] = th
    m = n_high == 1
    words[at[m] - 1] = th | (high[m].astype(dtype) << dtype(type_shift))
    words[at] = body
    return words


def encode_evt2(records) -> np.ndarray:
    """DAT8 records -> EVT 2.0 words (uint32), decoded back to the same records by the decoder.

    The stream opens with EVT_TIME_HIGH 0, so a decoder that shifts by the first EVT_TIME_HIGH keeps the timestamps too; another
    EVT_TIME_HIGH is written whenever ``t >> 6`` changes.  t may step back only inside the decoder's no-wrap slack (at most 10
    EVT_TIME_HIGH units, 640 us); x and y must fit 11 bits."""
    t, x, y, p = _evt2_fields(records)
    body = (p << 28) | ((t & 63) << 22) | (x << 11) | y
    return _evt2_interleave(t >> 6, body.astype(np.uint32), 0, np.uint32)


def encode_evt21(records) -> np.ndarray:
    """DAT8 records -> EVT 2.1 words (uint64), decoded back to the same records by the decoder.

    As ``encode_evt2``; a run of consecutive records of equal ``(t, y, p)`` whose x ascends strictly inside one 32-aligned block of
    columns becomes one word: x the block's first column, one mask bit per record."""
    t, x, y, p = _evt2_fields(records)
    n = len(t)
    cont = np.zeros(n, bool)
    cont[1:] = (t[1:] == t[:-1]) & (y[1:] == y[:-1]) & (p[1:] == p[:-1]) & (x[1:] > x[:-1]) & (x[1:] >> 5 == x[:-1] >> 5)
    first = np.flatnonzero(~cont)
    mask = np.zeros(len(first), dtype=np.uint64)
    if n:
        np.bitwise_or.at(mask, np.cumsum(~cont) - 1, np.uint64(1) << (x & 31).astype(np.uint64))
    g_t, g_x, g_y, g_p = t[first], x[first] & ~31, y[first], p[first]
    hi = (g_p << 28) | ((g_t & 63) << 22) | (g_x << 11) | g_y
    return _evt2_interleave(g_t >> 6, (hi.astype(np.uint64) << np.uint64(32)) | mask, 32, np.uint64)


# ---- the decode ----------------------------------------------------------------------------------------------------
class FrlwEvt2State(C.Structure):
    """frlw_evt2_state_t: the EVT 2.0 / EVT 2.1 decoder state carried from one call to the next."""
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("flags", C.c_uint32), ("loops", C.c_uint32),
                ("first_high", C.c_uint32), ("last_high", C.c_uint32), ("has_last_t", C.c_uint32), ("reserved2", C.c_uint32),
                ("last_t", C.c_uint64)]

    def __init__(self):
        super().__init__()
        self.struct_size = C.sizeof(type(self))

    def shift(self):
        """What ``time_shift`` subtracts: the stream's first EVT_TIME_HIGH << 6 (0 before one was seen)."""
        return (int(self.first_high) << 6) if self.flags & 1 else 0


class FrlwEvt3State(C.Structure):
    """frlw_evt3_state_t: the decoder state carried from one call to the next."""
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("flags", C.c_uint32), ("loops", C.c_uint32),
                ("first_high", C.c_uint32), ("last_high", C.c_uint32), ("low_y", C.c_uint32), ("base", C.c_uint32),
                ("has_last_t", C.c_uint32), ("reserved2", C.c_uint32), ("last_t", C.c_uint64)]

    def __init__(self):
        super().__init__()
        self.struct_size = C.sizeof(type(self))

    def shift(self):
        """What ``time_shift`` subtracts: the stream's first EVT_TIME_HIGH << 12 (0 before one was seen)."""
        return (int(self.first_high) << 12) if self.flags & 1 else 0


class FrlwEvt3Counters(C.Structure):
    """frlw_evt3_counters_t (t values unshifted)."""
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32)] + \
        [(name, C.c_uint64) for name in COUNTERS + ("min_t", "max_t")]

    def __init__(self):
        super().__init__()
        self.struct_size = C.sizeof(type(self))


class _Decoder:
    """What the decode calls need to know about one encoding: the five ``<prefix>_*`` entry points, the ``encoding`` argument that
    leads their arguments (EVT 2.x) or none (EVT 3.0), the state record and the width of a word."""

    def __init__(self, name, prefix, lead, state, word_bits):
        self.name, self.prefix, self.lead, self.state, self.word_bits = name, prefix, lead, state, word_bits

    def call(self, what, *args):
        entry = f"{self.prefix}_{what}"
        return _lib.check(getattr(_lib.load(), entry)(*self.lead, *args), entry)


_DECODERS = {"EVT2": _Decoder("EVT 2.0", "frlw_evt2", (_lib.EVT_20,), FrlwEvt2State, 32),
             "EVT21": _Decoder("EVT 2.1", "frlw_evt2", (_lib.EVT_21,), FrlwEvt2State, 64),
             "EVT3": _Decoder("EVT 3.0", "frlw_evt3", (), FrlwEvt3State, 16)}


def _evt2_decoder(encoding):
    if encoding not in ("EVT2", "EVT21"):
        raise ValueError(f"encoding: 'EVT2' or 'EVT21', not {encoding!r}")
    return _DECODERS[encoding]


def geometry(encoding="EVT3"):
    """(words per workgroup chunk, words per lane piece) of the decode kernels of ``encoding``."""
    c, l = C.c_int(0), C.c_int(0)
    (_DECODERS["EVT3"] if encoding == "EVT3" else _evt2_decoder(encoding)).call("geometry", C.byref(c), C.byref(l))
    return c.value, l.value


def _words_on_device(words, encoding="EVT3"):
    import torch
    bits = _DECODERS[encoding].word_bits
    if not isinstance(words, torch.Tensor) or not words.is_cuda or words.dim() != 1 or not words.is_contiguous() \
            or words.element_size() * 8 != bits:
        raise ValueError(f"words: a contiguous 1-d {bits}-bit tensor on the GPU")
    if words.numel() > MAX_CALL_WORDS:
        raise ValueError("at most 2^31 words per call: decode a longer stream piece by piece with the state carried")
    return words


def _stream(t):
    import torch
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _result(d, workspace, words, state_out):
    """-> (counters, the data-dependent status) behind the work enqueued on the stream of ``words``."""
    counters, status = FrlwEvt3Counters(), C.c_int(0)
    _lib.check(getattr(_lib.load(), d.prefix + "_result")(C.c_void_p(workspace.data_ptr()), _stream(words), C.byref(counters),
                                                          None if state_out is None else C.byref(state_out), C.byref(status)),
               d.prefix + "_result")
    return counters, status.value


def _count(words, size, state, encoding):
    import torch
    d = _DECODERS[encoding]
    words = _words_on_device(words, encoding)
    n = words.numel()
    ws = torch.empty(getattr(_lib.load(), d.prefix + "_workspace_bytes")(*d.lead, n), dtype=torch.uint8, device=words.device)
    d.call("count", C.c_void_p(words.data_ptr()), n, int(size[1]), int(size[0]), None if state is None else C.byref(state),
           C.c_void_p(ws.data_ptr()), ws.numel(), _stream(words))
    out = d.state()
    return _result(d, ws, words, out)[0], out, ws


def _emit(words, size, workspace, out, capacity, time_shift, encoding):
    d = _DECODERS[encoding]
    words = _words_on_device(words, encoding)
    if out.numel() * out.element_size() < 8 * capacity:
        raise ValueError("out is shorter than capacity records")
    d.call("emit", C.c_void_p(words.data_ptr()), words.numel(), int(size[1]), int(size[0]), C.c_void_p(workspace.data_ptr()),
           workspace.numel(), C.c_void_p(out.data_ptr()), int(capacity), 1 if time_shift else 0, _stream(words))
    return _result(d, workspace, words, None)[1]


def evt3_count(words, size, state=None):
    """The count call on ``words`` (GPU tensor of 16-bit words): -> ``(counters, state_out, workspace)``; ``counters`` a
    ``FrlwEvt3Counters`` (unshifted t), ``workspace`` the tensor that holds the plan ``evt3_emit`` needs."""
    return _count(words, size, state, "EVT3")


def evt3_emit(words, size, workspace, out, capacity, time_shift=True):
    """The emit call: records to ``out`` (GPU uint8 tensor, at least ``8 * capacity`` bytes); -> the data-dependent status
    (``_lib.FRLW_OK``, ``FRLW_ERR_SPAN``: a t does not fit, ``FRLW_ERR_ARG``: capacity too small -- nothing is written then)."""
    return _emit(words, size, workspace, out, capacity, time_shift, "EVT3")


def evt2_count(words, size, state=None, encoding="EVT2"):
    """``evt3_count`` for ``encoding`` 'EVT2' (32-bit words) or 'EVT21' (64-bit words): -> ``(counters, state_out, workspace)``;
    ``counters`` a ``FrlwEvt3Counters`` (unshifted t), ``state_out`` a ``FrlwEvt2State``."""
    _evt2_decoder(encoding)
    return _count(words, size, state, encoding)


def evt2_emit(words, size, workspace, out, capacity, time_shift=True, encoding="EVT2"):
    """``evt3_emit`` for ``encoding`` 'EVT2' or 'EVT21': -> the data-dependent status (nothing is written unless it is
    ``_lib.FRLW_OK``)."""
    _evt2_decoder(encoding)
    return _emit(words, size, workspace, out, capacity, time_shift, encoding)


def _raise_for(status, encoding="EVT3"):
    d = _DECODERS[encoding]
    if status == _lib.FRLW_ERR_SPAN:
        raise ValueError(f"{d.name} decode: recording longer than 2^32 us (a timestamp does not fit the 32 bits of a DAT record)")
    _lib.check(status, d.prefix + "_emit")


def _counters_dict(parts, shift):
    """The counters of successive calls as one dict; first_t / last_t as written (shifted)."""
    out = {name: sum(int(getattr(c, name)) for c in parts) for name in _SUMMED}
    emitting = [c for c in parts if c.events]
    out["first_t"] = int(emitting[0].first_t) - shift if emitting else 0
    out["last_t"] = int(emitting[-1].last_t) - shift if emitting else 0
    return out


def decode_evt3(words, size, state=None, time_shift=True):
    """``words`` (GPU tensor of 16-bit words) -> ``(dat, counters, state)``: ``dat`` an ``(n, 8)`` uint8 tensor of DAT8 records in
    stream order, ``counters`` a dict (``COUNTERS``), ``state`` what to pass to the call on the words that follow (the cut may
    fall anywhere).  ``size``: ``(height, width)``; events outside are dropped and counted."""
    return _decode(words, size, state, time_shift, "EVT3")


def _decode(words, size, state, time_shift, encoding):
    import torch
    counters, out_state, ws = _count(words, size, state, encoding)
    n = int(counters.events)
    dat = torch.empty((n, 8), dtype=torch.uint8, device=words.device)
    _raise_for(_emit(words, size, ws, dat, n, time_shift, encoding), encoding)
    return dat, _counters_dict([counters], out_state.shift() if time_shift else 0), out_state


def decode_evt2(words, size, state=None, time_shift=True):
    """``decode_evt3`` for EVT 2.0: ``words`` a contiguous 1-d 32-bit GPU tensor; ``state`` a ``FrlwEvt2State``."""
    return _decode(words, size, state, time_shift, "EVT2")


def decode_evt21(words, size, state=None, time_shift=True):
    """``decode_evt3`` for EVT 2.1: ``words`` a contiguous 1-d 64-bit GPU tensor; ``state`` a ``FrlwEvt2State``."""
    return _decode(words, size, state, time_shift, "EVT21")


class RawFile:
    """The words of one ``.raw`` file, memory-mapped (``<u4`` / ``<u8`` / ``<u2`` by ``encoding``: 'EVT2' / 'EVT21' / 'EVT3');
    ``size`` is the header's ``(height, width)`` or None."""
    PIECE_WORDS = 1 << 27   # words per decode call (256 MiB of EVT 3.0 input on the device at a time, 512 MiB / 1 GiB of EVT 2.0 / 2.1)

    def __init__(self, path):
        self.path = path
        self.start, self.size, self.fields, self.encoding = raw_header(path)
        dtype = np.dtype(_WORD_DTYPE[self.encoding])
        n = (os.path.getsize(path) - self.start) // dtype.itemsize      # trailing bytes that do not fill a word are ignored
        self.words = np.memmap(path, dtype=dtype, mode="r", offset=self.start, shape=(n,)) if n > 0 else np.empty(0, dtype)
        self.counters = None

    def __len__(self):
        return len(self.words)

    def _piece(self, lo, device):
        import torch
        host = np.array(self.words[lo:lo + self.PIECE_WORDS])                  # a writable copy of the mapped slice
        host = host.view({2: np.int16, 4: np.int32, 8: np.int64}[host.dtype.itemsize])
        return torch.from_numpy(host).to(device)

    def decode(self, device="cuda", time_shift=True, size=None):
        """-> ``(dat, counters)``: one count sweep over the pieces of the file with the state carried, one allocation, the emit
        sweep.  ``size`` overrides / supplies the sensor shape."""
        import torch
        size = size or self.size
        if size is None:
            raise ValueError(f"{self.path}: the header names no geometry: pass size=(height, width)")
        starts = list(range(0, len(self.words), self.PIECE_WORDS)) or [0]
        state, plans = None, []
        for lo in starts:
            piece = self._piece(lo, device)
            counters, out_state, ws = _count(piece, size, state, self.encoding)
            plans.append((lo, counters, ws, piece if len(starts) == 1 else None))
            state = out_state
        total = sum(int(c.events) for _, c, _, _ in plans)
        dat = torch.empty((total, 8), dtype=torch.uint8, device=device)
        at = 0
        for lo, counters, ws, piece in plans:
            piece = self._piece(lo, device) if piece is None else piece
            n = int(counters.events)
            _raise_for(_emit(piece, size, ws, dat[at:at + n], n, time_shift, self.encoding), self.encoding)
            at += n
        self.counters = _counters_dict([c for _, c, _, _ in plans], state.shift() if time_shift else 0)
        return dat, self.counters

    def total_time(self):
        """Timestamp of the last event, as decoded (known after ``decode``)."""
        if self.counters is None:
            raise RuntimeError("total_time() is known after decode()")
        return self.counters["last_t"]


def raw_to_dat(raw_path, dat_path, device="cuda", size=None):
    """Decode ``raw_path`` on the GPU and write it as a ``*_td.dat`` file, so the offline ``generate_*.py`` commands and training
    read a camera recording.  -> the decode counters."""
    from . import dat_io
    f = RawFile(raw_path)
    dat, counters = f.decode(device=device, time_shift=True, size=size)
    size = size or f.size
    dat_io.write_dat(dat_path, dat.cpu().numpy().view(DAT_DTYPE).reshape(-1), size[0], size[1])
    return counters
