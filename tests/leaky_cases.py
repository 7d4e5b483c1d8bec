"""uint8(leaky_transform(v)) at every level edge, bucket and special: the value list and the references of
tests/test_leaky_cases_cpu.py, tests/test_leaky_forms_gpu.py and tests/test_elementwise_gpu.py.  numpy only.

The transform (generate_taf.py:69-76) of a state slot ``v`` is ``255 * max(0, 1 - log1p(-v) / 8.7)``; the byte the detector is
fed is its uint8 truncation.  With x = -v >= 0 that byte is a non-increasing step function of x with 256 levels, which three of
the library's four forms evaluate through tables (csrc/leaky.h).  Everything here is stated without those tables:

    level64(x)          the transform in float64
    u8_rule(f32)        float32 -> uint8 as csrc/frlw_common.h documents f32_to_u8, in integer arithmetic
    thresholds(exact)   the 255 level edges of ANY exact routine float32 -> uint8, by bisection over bit patterns
    values(thr)         the list: 17 bit patterns around every edge (A), both ends of every bucket of the bucket table and
                        what lies outside the table (B), the specials (C), a log-spaced sweep (D)
"""
import numpy as np

DEN = 8.7  # generate_taf.py:73

# The bucket table of leaky_u8_bucket_n, restated from csrc/leaky.h (kLeakyBucketShift, kLeakyBucket0, kLeakyBuckets): the
# bucket of x is its float32 bit pattern >> 18 (the exponent and five mantissa bits), counted from the one of 2^-6 and
# clamped to [0, 607]; the last bucket ends in front of 2^13.
BUCKET_SHIFT = 18
BUCKET0 = (127 - 6) << 5
BUCKETS = ((127 + 13) << 5) - BUCKET0
assert BUCKETS == 608

BISECT_HI = 0x7F000000  # leaky_threshold_bits: f(0) = 255 >= k always, f(2^127) = 0
BISECT_ROUNDS = 31      # 0x7f000000 < 2^31: the interval is one pattern wide after 31 halvings
D_COUNT = 16384
D_LOG2 = (-6.0, 13.0)
A_REACH = 8             # bit patterns on either side of an edge


def bits_f32(b):
    """uint32 bit patterns -> float32."""
    return np.ascontiguousarray(b, dtype=np.uint32).view(np.float32)


def f32_bits(v):
    """float32 -> uint32 bit patterns."""
    return np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)


def level64(x):
    """255 * max(0, 1 - log1p(x) / 8.7) in float64, x = -v >= 0."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):  # (x = inf: 1 - inf = -inf, clamped)
        return 255.0 * np.maximum(0.0, 1.0 - np.log1p(x) / DEN)


def edge64(k):
    """The x at which level64 crosses the integer k (1..254) coming from above: level64(x) >= k exactly for x <= edge64(k)."""
    k = np.asarray(k, dtype=np.float64)
    return np.expm1(DEN * (1.0 - k / 255.0))


def u8_rule(v):
    """float32 -> uint8 the way f32_to_u8 states it (csrc/frlw_common.h:88): the x86 cvttss2si conversion to int32 -- truncate
    toward zero where -2^31 <= v < 2^31, INT_MIN otherwise (out of range, infinite, NaN) -- then the low byte.  The float never
    meets a uint8 conversion here: truncation happens in float64 (exact for a float32), the byte is cut from an int64."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        ok = (v >= np.float32(-2147483648.0)) & (v < np.float32(2147483648.0))  # NaN compares false
    t = np.trunc(np.where(ok, v, np.float32(0)).astype(np.float64)).astype(np.int64)
    i32 = np.where(ok, t, np.int64(-2147483648))
    return (i32 & 0xFF).astype(np.uint8)  # an integer in 0..255: nothing to round or wrap


def thresholds(exact_u8):
    """thr[k], k = 1..255: the bit pattern of the largest x in [0, 2^127) with ``exact_u8(-x) >= k``; thr[0] = the one of +inf.
    ``exact_u8``: float32 array of v -> uint8 array.  255 lanes bisect at once, one call on 255 values per round
    (leaky_threshold_bits of csrc/leaky.h, through any exact routine instead of the device's table)."""
    k = np.arange(1, 256, dtype=np.int64)
    lo = np.zeros(255, dtype=np.int64)
    hi = np.full(255, BISECT_HI, dtype=np.int64)
    for _ in range(BISECT_ROUNDS):
        mid = lo + (hi - lo) // 2
        ge = np.asarray(exact_u8(-bits_f32(mid.astype(np.uint32)))).astype(np.int64) >= k
        lo = np.where(ge, mid, lo)
        hi = np.where(ge, hi, mid)
    assert np.all(hi - lo <= 1)
    return np.concatenate([[0x7F800000], lo]).astype(np.uint32)


def bucket_of(xb):
    """The bucket leaky_u8_bucket_n reads for the bit pattern ``xb`` of x."""
    b = (np.asarray(xb, dtype=np.int64) >> BUCKET_SHIFT) - BUCKET0
    return np.clip(b, 0, BUCKETS - 1)


def bucket_bounds():
    """(first, last) bit pattern of every bucket as the (x >> 18) rule cuts them (without the clamp at either end)."""
    b = np.arange(BUCKETS, dtype=np.int64)
    first = (b + BUCKET0) << BUCKET_SHIFT
    return first, first + (1 << BUCKET_SHIFT) - 1


FLT_MIN_BITS = 0x00800000
FLT_MAX_BITS = 0x7F7FFFFF
INF_BITS = 0x7F800000

# C, the specials, as v (not -x): (name, bit pattern)
SPECIALS = [
    ("+0", 0x00000000), ("-0", 0x80000000), ("+denormal", 0x00000001), ("-denormal", 0x80000001),
    ("0.5", int(f32_bits(np.float32(0.5))[0])), ("0.999", int(f32_bits(np.float32(0.999))[0])),
    ("nextafter(1,0)", 0x3F7FFFFF), ("1.0", 0x3F800000), ("1.5", 0x3FC00000),
    ("+inf", 0x7F800000), ("-inf", 0xFF800000), ("+nan", 0x7FC12345), ("-nan", 0xFFC54321),
    ("-5800.5566", int(f32_bits(np.float32(-5800.5566))[0])), ("-6000", int(f32_bits(np.float32(-6000.0))[0])),
    ("-6001.9", int(f32_bits(np.float32(-6001.9))[0])), ("-6002", int(f32_bits(np.float32(-6002.0))[0])),
    ("-6002.5", int(f32_bits(np.float32(-6002.5))[0])),
]
# the bytes that do not depend on whose log1pf ran: name -> uint8(leaky_transform(v))
#   +-0, +-denormal  log1p(-v) = -v exactly (or 0): 1 - (tiny / 8.7) rounds to 1, 255
#   0.5              255 * (1 + 0.693147 / 8.7) = 275.3, low byte of 275 = 19
#   0.999            255 * (1 + 6.907755 / 8.7) = 457.47, low byte of 457 = 201
#   1.0              log1p(-1) = -inf, the level +inf: out of the int32 range, INT_MIN, 0
#   1.5, +inf, NaN   log1p gives NaN (NaN < 0 is false, so the clamp keeps it): INT_MIN, 0
#   -inf             log1p(+inf) = +inf, 1 - inf = -inf, clamped to 0
#   -6002.5, -1e30   the level is negative before the clamp from x = 6001.91 on, 0
SPECIAL_BYTES = {"+0": 255, "-0": 255, "+denormal": 255, "-denormal": 255, "0.5": 19, "0.999": 201, "1.0": 0, "1.5": 0,
                 "+inf": 0, "-inf": 0, "+nan": 0, "-nan": 0, "-6002.5": 0}


def values(thr):
    """The list as a dict of float32 arrays of v: "A" (255 x 17 = 4 335), "B" (608 x 4 + 12 = 2 444), "C" (18), "D" (16 384).
    ``thr``: thresholds() of the routine under test (A sits on ITS edges); None: A is left empty.  Deterministic."""
    a_bits = np.zeros(0, dtype=np.int64)
    if thr is not None:
        thr = np.asarray(thr, dtype=np.uint32).astype(np.int64)
        assert thr.shape == (256,)
        d = np.arange(-A_REACH, A_REACH + 1, dtype=np.int64)
        a_bits = (thr[1:, None] + d[None, :]).reshape(-1)
        assert a_bits.min() >= 0 and a_bits.max() < INF_BITS
    first, last = bucket_bounds()
    b_bits = np.stack([first - 1, first, last, last + 1], axis=1).reshape(-1)
    one = lambda x: int(f32_bits(np.float32(x))[0])  # noqa: E731
    below = [one(2.0 ** -6) - 1, one(2.0 ** -7), one(1e-7), 0x00000001, FLT_MIN_BITS - 1, FLT_MIN_BITS]
    above = [one(2.0 ** 13) - 1, one(2.0 ** 13), one(2.0 ** 14), one(1e30), FLT_MAX_BITS, INF_BITS]
    b_bits = np.concatenate([b_bits, below, above])
    sweep = np.exp2(np.linspace(D_LOG2[0], D_LOG2[1], D_COUNT)).astype(np.float32)
    return {
        "A": -bits_f32(a_bits.astype(np.uint32)),
        "B": -bits_f32(b_bits.astype(np.uint32)),
        "C": bits_f32(np.array([b for _, b in SPECIALS], dtype=np.uint32)),
        "D": -sweep,
    }


def flat(vals, groups="ABCD"):
    return np.concatenate([vals[g] for g in groups])


def margin(f32_level, x):
    """The one tolerance of these tests: 4 x the largest distance of a float32 restatement of the transform from level64 on
    the points ``x`` (A and D) -- the factor the TV-L1 and motion tests give float32 arithmetic over its own restatement."""
    return 4.0 * float(np.max(np.abs(np.asarray(f32_level, dtype=np.float64) - level64(x))))


def undecided(x, m):
    """Where float64 does not decide the byte: level64 within ``m`` of an integer, strictly between 0 and 255."""
    lv = level64(x)
    return (np.abs(lv - np.round(lv)) < m) & (lv > 0.0) & (lv < 255.0)


def edge_ulps(thr, m):
    """For k = 1..254: (distance of thr[k] from the float64 edge, the distance that ``m`` levels amount to there), both in ulp
    of thr[k].  d level / dx = 255 / (8.7 (1 + x)), so m levels are m * 8.7 * (1 + x) / 255 in x; one more ulp because the
    threshold is the last float32 in front of the edge of a routine that may be off by m, not the edge itself."""
    k = np.arange(1, 255)
    x = bits_f32(np.asarray(thr, dtype=np.uint32)[1:255]).astype(np.float64)
    ulp = np.spacing(x.astype(np.float32)).astype(np.float64)
    got = np.abs(x - edge64(k)) / ulp
    allowed = m * DEN * (1.0 + x) / 255.0 / ulp + 1.0
    return got, allowed
