"""Streams the EVT 3.0 tests share: the hand-assembled stream with its decode written out literally, the burst recording for the
round trips, and small builders of words."""
import numpy as np

from frlw_evd_amd import synth

# ---- the hand-assembled stream: every word type of DESIGN.md's table, on a 304 x 240 frame ------------------------------------
HAND_SIZE = (240, 304)
HAND_WORDS = np.array([
    0x2005,  # EVT_ADDR_X x=5 p=0            before the first TIME_HIGH and ADDR_Y: before_sync
    0x4003,  # VECT_12 bits 0, 1             before the first VECT_BASE_X: 2 x before_sync, base stays unset
    0xA001,  # EXT_TRIGGER
    0x8110,  # EVT_TIME_HIGH 0x110           the stream's first: the shift is 0x110000
    0x2806,  # EVT_ADDR_X x=6 p=1            before the first ADDR_Y: before_sync
    0x0814,  # EVT_ADDR_Y y=20, bit 11 set   (camera origin bit, ignored)
    0x2807,  # EVT_ADDR_X x=7 p=1            -> (7, 20, 1, 0x110000): low is 0 before the first TIME_LOW
    0x6ABC,  # EVT_TIME_LOW 0xABC
    0x200A,  # EVT_ADDR_X x=10 p=0           -> (10, 20, 0, 0x110ABC)
    0x3864,  # VECT_BASE_X x=100 p=1
    0x4805,  # VECT_12 bits 0, 2, 11         -> x = 100, 102, 111; base = 112
    0x5F81,  # VECT_8 payload 0xF81          bits above 7 ignored: bits 0, 7 -> x = 112, 119; base = 120
    0x7123,  # CONTINUED_4                   other
    0xE000,  # OTHERS                        other
    0xF456,  # CONTINUED_12                  other
    0x1000,  # type 0x1 (unknown)            other
    0x8124,  # EVT_TIME_HIGH 0x124
    0x6001,  # EVT_TIME_LOW 1
    0x0005,  # EVT_ADDR_Y y=5
    0x2130,  # EVT_ADDR_X x=304              out_of_frame (x == width)
    0x212F,  # EVT_ADDR_X x=303 p=0          -> (303, 5, 0, 0x124001)
    0x312A,  # VECT_BASE_X x=298 p=0
    0x4FFF,  # VECT_12 all bits              -> x = 298 .. 303; 304 .. 309: 6 x out_of_frame; base = 310
    0x5003,  # VECT_8 bits 0, 1              x = 310, 311: 2 x out_of_frame; base = 318
    0x00F0,  # EVT_ADDR_Y y=240
    0x2001,  # EVT_ADDR_X x=1                out_of_frame (y == height)
    0x0000,  # EVT_ADDR_Y y=0
    0x811A,  # EVT_TIME_HIGH 0x11A           10 below 0x124: taken as it is, no wrap
    0x2002,  # EVT_ADDR_X x=2 p=0            -> (2, 0, 0, 0x11A001): earlier than its predecessor: unsorted
    0x8FFF,  # EVT_TIME_HIGH 4095
    0x2003,  # EVT_ADDR_X x=3 p=0            -> (3, 0, 0, 0xFFF001)
    0x8000,  # EVT_TIME_HIGH 0               a wrap: loops = 1
    0x6000,  # EVT_TIME_LOW 0
    0x2804,  # EVT_ADDR_X x=4 p=1            -> (4, 0, 1, 0x1000000)
    0xA801,  # EXT_TRIGGER
    0x3000,  # VECT_BASE_X x=0 p=0
    0x4000,  # VECT_12 no bit                nothing; base = 12
    0x5010,  # VECT_8 bit 4                  -> (16, 0, 0, 0x1000000)
], dtype=np.uint16)
# (x, y, p, t) with time_shift: t - 0x110000
HAND_EVENTS = [
    (7, 20, 1, 0x000000), (10, 20, 0, 0x000ABC), (100, 20, 1, 0x000ABC), (102, 20, 1, 0x000ABC), (111, 20, 1, 0x000ABC),
    (112, 20, 1, 0x000ABC), (119, 20, 1, 0x000ABC), (303, 5, 0, 0x014001), (298, 5, 0, 0x014001), (299, 5, 0, 0x014001),
    (300, 5, 0, 0x014001), (301, 5, 0, 0x014001), (302, 5, 0, 0x014001), (303, 5, 0, 0x014001), (2, 0, 0, 0x00A001),
    (3, 0, 0, 0xEEF001), (4, 0, 1, 0xEF0000), (16, 0, 0, 0xEF0000),
]
HAND_COUNTERS = {"events": 18, "before_sync": 4, "out_of_frame": 10, "triggers": 2, "other_words": 4, "time_loops": 1, "unsorted": 1,
                 "first_t": 0, "last_t": 0xEF0000}


def records_of(events):
    """[(x, y, p, t)] -> DAT8 records."""
    a = np.array(events, dtype=np.int64).reshape(-1, 4)
    return synth.to_dat8({"x": a[:, 0], "y": a[:, 1], "p": a[:, 2], "t": a[:, 3]})


# ---- the burst recording of the round trips: 304 x 240, about 20 000 events, half of them in vector runs ------------------------
BURST_SIZE = (240, 304)


def burst_events(seed=77, n=20_000, size=BURST_SIZE, t_span=400_000):
    return synth.synth_burst_events(seed, n, size[1], size[0], t_span)


# ---- word builders ---------------------------------------------------------------------------------------------------
def th(v):
    return 0x8000 | v


def tl(v):
    return 0x6000 | v


def ay(y):
    return 0x0000 | y


def ax(x, p=0):
    return 0x2000 | (p << 11) | x


def vb(x, p=0):
    return 0x3000 | (p << 11) | x


def v12(mask):
    return 0x4000 | mask


def v8(mask):
    return 0x5000 | mask


OTHERS, CONTINUED_12, TRIGGER = 0xE000, 0xF000, 0xA000


def filler(n, seed, x_max=64):
    """n words that set nothing: EVT_ADDR_X with random x below x_max, OTHERS and CONTINUED_12."""
    rng = np.random.default_rng(seed)
    kind = rng.integers(0, 4, size=n)
    w = np.where(kind == 0, OTHERS, np.where(kind == 1, CONTINUED_12 | rng.integers(0, 4096, size=n),
                                              0x2000 | (rng.integers(0, 2, size=n) << 11) | rng.integers(0, x_max, size=n)))
    return w.astype(np.uint16)
