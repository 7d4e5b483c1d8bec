"""Streams the EVT 2.0 / EVT 2.1 tests share: word builders, one hand-assembled stream per encoding with its decode written out
literally, the burst recording for the round trips and the fuzz stream of the GPU tests."""
import numpy as np

from frlw_evd_amd import synth

ENCODINGS = ("EVT2", "EVT21")
DTYPE = {"EVT2": np.uint32, "EVT21": np.uint64}


# ---- word builders: Python ints ------------------------------------------------------------------------------------------
def _place(hi, lo, enc):
    return hi if enc == "EVT2" else (hi << 32) | lo


def th(v, enc, ignored=0):
    """EVT_TIME_HIGH v (28 bits); `ignored`: bits 31..0 of an EVT 2.1 word."""
    return _place(0x80000000 | v, ignored, enc)


def cd(x, y, p, low, enc, mask=1):
    """An event word: CD_OFF / CD_ON for EVT 2.0 (mask must stay 1), EVT_NEG / EVT_POS with `mask` for EVT 2.1."""
    assert enc == "EVT21" or mask == 1
    return _place((p << 28) | (low << 22) | (x << 11) | y, mask, enc)


def trigger(enc, payload=1):
    return _place(0xA0000000 | payload, 0, enc)


def other(kind, enc, payload=0):
    """A word of no effect: kind 0xE OTHERS, 0xF CONTINUED, or an unknown type."""
    assert kind not in (0x0, 0x1, 0x8, 0xA)
    return _place((kind << 28) | payload, payload, enc)


def words_of(seq, enc):
    return np.array(seq, dtype=DTYPE[enc])


# ---- the hand-assembled streams, on a 304 x 240 frame ------------------------------------------------------------------------
# The first EVT_TIME_HIGH is 0x11: with time_shift the records are 0x440 earlier than the t written beside the words.
HAND_SIZE = (240, 304)
HAND_SHIFT = 0x11 << 6
_E = "EVT2"
HAND_WORDS_EVT2 = words_of([
    cd(5, 6, 1, 3, _E),             # in front of the first EVT_TIME_HIGH: before_sync
    trigger(_E),                    # EXT_TRIGGER
    th(0x11, _E),                   # the stream's first EVT_TIME_HIGH
    cd(7, 20, 1, 0, _E),            # -> (7, 20, 1, 0x440)
    cd(10, 20, 0, 63, _E),          # -> (10, 20, 0, 0x47F)
    other(0xE, _E),                 # OTHERS
    other(0xF, _E, 0x456),          # CONTINUED
    other(0x3, _E),                 # unknown type
    other(0x2, _E, 0xABCDEF0),      # unknown type
    th(0x24, _E),
    cd(304, 5, 0, 1, _E),           # x == width: out_of_frame
    cd(303, 5, 0, 1, _E),           # -> (303, 5, 0, 0x901)
    cd(1, 240, 1, 2, _E),           # y == height: out_of_frame
    cd(0, 239, 1, 2, _E),           # -> (0, 239, 1, 0x902)
    th(0x1A, _E),                   # 10 below 0x24: taken as it is, no wrap
    cd(2, 0, 0, 1, _E),             # -> (2, 0, 0, 0x681): earlier than its predecessor: unsorted
    th(0x30, _E),
    cd(3, 0, 0, 63, _E),            # -> (3, 0, 0, 0xC3F)
    trigger(_E, 0x8000001),
    cd(303, 239, 1, 0, _E),         # -> (303, 239, 1, 0xC00): unsorted
    th(0x30, _E),                   # the same value again
    cd(2047, 2047, 1, 5, _E),       # out_of_frame
    cd(0, 0, 0, 5, _E),             # -> (0, 0, 0, 0xC05)
    th(0x31, _E),
    cd(100, 100, 1, 32, _E),        # -> (100, 100, 1, 0xC60)
    other(0xE, _E, 0x1234567),
    cd(100, 100, 0, 32, _E),        # -> (100, 100, 0, 0xC60)
    cd(150, 7, 1, 33, _E),          # -> (150, 7, 1, 0xC61)
], _E)
# (x, y, p, t) as written without the shift
HAND_EVENTS_EVT2 = [
    (7, 20, 1, 0x440), (10, 20, 0, 0x47F), (303, 5, 0, 0x901), (0, 239, 1, 0x902), (2, 0, 0, 0x681), (3, 0, 0, 0xC3F),
    (303, 239, 1, 0xC00), (0, 0, 0, 0xC05), (100, 100, 1, 0xC60), (100, 100, 0, 0xC60), (150, 7, 1, 0xC61),
]
HAND_COUNTERS_EVT2 = {"events": 11, "before_sync": 1, "out_of_frame": 3, "triggers": 2, "other_words": 5, "time_loops": 0, "unsorted": 2,
                      "first_t": 0x440, "last_t": 0xC61}

_E = "EVT21"
HAND_WORDS_EVT21 = words_of([
    cd(0, 6, 1, 3, _E, 0x7),                # in front of the first EVT_TIME_HIGH: 3 x before_sync
    trigger(_E),
    th(0x11, _E, ignored=0xDEADBEEF),       # bits 31..0 of an EVT_TIME_HIGH are ignored
    cd(7, 20, 1, 0, _E, 0b101),             # x need not be a multiple of 32 -> x = 7, 9 at 0x440
    cd(288, 5, 0, 63, _E, 0xFFFFFFFF),      # straddles the right edge -> x = 288 .. 303 at 0x47F; 304 .. 319: 16 x out_of_frame
    other(0xE, _E),
    other(0xF, _E, 0x456),
    other(0x3, _E),
    other(0x2, _E, 0xABCDEF0),
    th(0x24, _E),
    cd(304, 5, 0, 1, _E, 0x3),              # 2 x out_of_frame
    cd(32, 240, 1, 2, _E, 0x80000001),      # y == height: 2 x out_of_frame
    cd(300, 239, 1, 2, _E, 0x80000009),     # -> x = 300, 303 at 0x902; 331: out_of_frame
    cd(1, 1, 0, 2, _E, 0),                  # no bit: nothing
    th(0x1A, _E),                           # 10 below 0x24: no wrap
    cd(2, 0, 0, 1, _E, 0x1),                # -> (2, 0, 0, 0x681): unsorted
    th(0x30, _E),
    cd(64, 0, 0, 63, _E, 0x80000000),       # -> (95, 0, 0, 0xC3F)
    trigger(_E, 0x8000001),
    cd(272, 239, 1, 0, _E, 0xC0000000),     # -> x = 302, 303 at 0xC00: the first of them unsorted
    th(0x30, _E),
    cd(2047, 2047, 1, 5, _E, 0xFFFFFFFF),   # 32 x out_of_frame
    cd(0, 0, 0, 5, _E, 0x10001),            # -> x = 0, 16 at 0xC05
    th(0x31, _E),
    cd(100, 100, 1, 32, _E, 0x3),           # -> x = 100, 101 at 0xC60
    other(0xE, _E, 0x1234567),
    cd(100, 100, 0, 32, _E, 0x1),           # -> (100, 100, 0, 0xC60)
    cd(150, 7, 1, 33, _E, 0x2),             # -> (151, 7, 1, 0xC61)
], _E)
HAND_EVENTS_EVT21 = [(7, 20, 1, 0x440), (9, 20, 1, 0x440)] + [(x, 5, 0, 0x47F) for x in range(288, 304)] + [
    (300, 239, 1, 0x902), (303, 239, 1, 0x902), (2, 0, 0, 0x681), (95, 0, 0, 0xC3F), (302, 239, 1, 0xC00), (303, 239, 1, 0xC00),
    (0, 0, 0, 0xC05), (16, 0, 0, 0xC05), (100, 100, 1, 0xC60), (101, 100, 1, 0xC60), (100, 100, 0, 0xC60), (151, 7, 1, 0xC61),
]
HAND_COUNTERS_EVT21 = {"events": 30, "before_sync": 3, "out_of_frame": 53, "triggers": 2, "other_words": 5, "time_loops": 0, "unsorted": 2,
                       "first_t": 0x440, "last_t": 0xC61}

HAND_WORDS = {"EVT2": HAND_WORDS_EVT2, "EVT21": HAND_WORDS_EVT21}
HAND_EVENTS = {"EVT2": HAND_EVENTS_EVT2, "EVT21": HAND_EVENTS_EVT21}
HAND_COUNTERS = {"EVT2": HAND_COUNTERS_EVT2, "EVT21": HAND_COUNTERS_EVT21}


def records_of(events, shift=0):
    """[(x, y, p, t)] -> DAT8 records with t - shift."""
    a = np.array(events, dtype=np.int64).reshape(-1, 4)
    return synth.to_dat8({"x": a[:, 0], "y": a[:, 1], "p": a[:, 2], "t": a[:, 3] - shift})


def shifted(counters, shift):
    out = dict(counters)
    out["first_t"], out["last_t"] = counters["first_t"] - shift, counters["last_t"] - shift
    return out


# ---- the three literal streams that pin the clock (one event per word in both encodings) ------------------------------------
def clock_streams(enc):
    """name -> words.  'wrap': t = 63, 64 and one time loop with the shift; 'beyond': refused; 'edge': t = 0, 2^32 - 1."""
    return {
        "wrap": words_of([th((1 << 28) - 1, enc), cd(1, 1, 0, 63, enc), th(0, enc), cd(2, 1, 1, 0, enc)], enc),
        "beyond": words_of([th(0, enc), cd(1, 1, 0, 0, enc), th(1 << 26, enc), cd(2, 1, 1, 0, enc)], enc),
        "edge": words_of([th(0, enc), cd(1, 1, 0, 0, enc), th((1 << 26) - 1, enc), cd(2, 1, 1, 63, enc)], enc),
    }


# ---- the burst recording of the round trips: 304 x 240, about 20 000 events in time order -----------------------------------
BURST_SIZE = (240, 304)


def burst_events(seed=77, n=20_000, size=BURST_SIZE, t_span=400_000):
    return synth.synth_burst_events(seed, n, size[1], size[0], t_span)


# ---- filler and fuzz -------------------------------------------------------------------------------------------------------
def _assemble(kind, x, y, p, low, mask, payload, enc):
    """Arrays -> words.  kind: the type nibble; event fields are used where kind is 0 / 1, payload (28 bits) elsewhere."""
    hi = np.where(kind <= 1, (p << 28) | (low << 22) | (x << 11) | y, (kind << 28) | payload).astype(np.uint64)
    if enc == "EVT2":
        return hi.astype(np.uint32)
    lo = np.where(kind <= 1, mask, payload).astype(np.uint64)
    return (hi << np.uint64(32)) | lo


def random_masks(rng, n):
    """A mix of the AND of two random words, all ones and single bits."""
    how = rng.integers(0, 10, size=n)
    m = rng.integers(0, 1 << 32, size=n, dtype=np.uint64) & rng.integers(0, 1 << 32, size=n, dtype=np.uint64)
    m = np.where(how == 0, np.uint64(0xFFFFFFFF), m)
    return np.where(how >= 7, np.uint64(1) << rng.integers(0, 32, size=n).astype(np.uint64), m).astype(np.int64)


def filler(n, seed, enc, x_max=300, y_max=240):
    """n words that set nothing: events (random masks for EVT 2.1), OTHERS, EXT_TRIGGER and CONTINUED words."""
    rng = np.random.default_rng(seed)
    r = rng.integers(0, 100, size=n)
    kind = np.where(r < 6, 0xE, np.where(r < 10, 0xA, np.where(r < 12, 0xF, rng.integers(0, 2, size=n))))
    mask = random_masks(rng, n) if enc == "EVT21" else np.ones(n, np.int64)
    return _assemble(kind, rng.integers(0, x_max, size=n), rng.integers(0, y_max, size=n), kind & 1, rng.integers(0, 64, size=n), mask,
                     rng.integers(0, 1 << 28, size=n), enc)


def fuzz(n, seed, enc, width=304):
    """The fuzz stream of the GPU tests.  Per word 8 % EVT_TIME_HIGH, 6 % OTHERS, 4 % EXT_TRIGGER, 2 % another type, the rest
    events with x in [0, width + 12), y in [0, 250) and random low bits.  The first EVT_TIME_HIGH sits at a random word in 3..40
    (none before it); its value walks by steps in -3..+5 and never goes below the stream's first value."""
    rng = np.random.default_rng(seed)
    r = rng.integers(0, 100, size=n)
    kind = np.where(r < 8, 0x8, np.where(r < 14, 0xE, np.where(r < 18, 0xA, np.where(r < 20, rng.choice([0x2, 0x5, 0x7, 0xF], size=n),
                                                                                   rng.integers(0, 2, size=n)))))
    first = int(rng.integers(3, 41))
    kind[:first] = np.where(kind[:first] == 0x8, 0xE, kind[:first])
    kind[first] = 0x8
    payload = rng.integers(0, 1 << 28, size=n)
    at = np.flatnonzero(kind == 0x8)
    v0 = int(rng.integers(0, 1000))
    v, values = v0, []
    for step in rng.integers(-3, 6, size=len(at)).tolist():
        values.append(v)
        v = max(v0, v + step)
    payload[at] = values
    mask = random_masks(rng, n) if enc == "EVT21" else np.ones(n, np.int64)
    return _assemble(kind, rng.integers(0, width + 12, size=n), rng.integers(0, 250, size=n), kind & 1, rng.integers(0, 64, size=n), mask,
                     payload, enc)
