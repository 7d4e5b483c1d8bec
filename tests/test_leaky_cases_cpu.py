"""tests/leaky_cases.py on the CPU: the builder run with the oracle's orc_leaky_transform + u8_rule as the exact routine.

Pins what does not depend on a GPU: the list's size, the thresholds' order, one threshold per bucket at most, the bytes of the
specials, and the condition on the sweep D that tests/test_leaky_forms_gpu.py relies on (float64 decides all but a handful of
its bytes).  Measured with the oracle on an x86 host (glibc's log1pf): margin m = 1.04e-4 levels (4 x 2.6e-5), 2 undecided
values on D, thresholds within 37 ulp of the float64 edge for k <= 253 (71 ulp for k = 254, where an ulp is 3.7e-9),
thr[255] = 2.5928e-7, thr[254] = 0.034707, thr[1] = 5800.56.
"""
import numpy as np
import pytest

import leaky_cases as lc


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def cpu(orc):
    def exact(v):
        return lc.u8_rule(orc.leaky_transform(v))
    thr = lc.thresholds(exact)
    vals = lc.values(thr)
    x = -lc.flat(vals, "AD")
    m = lc.margin(orc.leaky_transform(-x), x)
    return {"exact": exact, "thr": thr, "vals": vals, "m": m}


def test_u8_rule():
    """The conversion itself, at the values where a saturating or a rounding conversion would differ."""
    two31 = np.float32(2147483648.0)
    v = np.array([0.0, -0.0, 0.999, -0.999, -1.5, 254.999, 255.0, 255.99998, 256.0, 300.7, -300.7, 1e9, two31,
                  np.nextafter(two31, np.float32(0)), -two31, np.nextafter(-two31, np.float32(-np.inf)), np.inf, -np.inf, np.nan],
                 dtype=np.float32)
    want = [0, 0, 0, 0, 255, 254, 255, 255, 0, 44, 256 - 44, 0, 0, 0x80, 0, 0, 0, 0, 0]  # 1e9 = 0x3b9aca00; 2^31 - 128 = 0x7fffff80
    assert lc.u8_rule(v).tolist() == want
    assert lc.u8_rule(v).dtype == np.uint8


def test_list_size_and_groups(cpu):
    vals = cpu["vals"]
    assert {g: len(v) for g, v in vals.items()} == {"A": 255 * 17, "B": 608 * 4 + 12, "C": 18, "D": 16384}
    assert len(lc.flat(vals)) == 23181
    assert all(v.dtype == np.float32 for v in vals.values())
    a = lc.f32_bits(vals["A"])
    assert len(np.unique(a)) == len(a), "neighbourhoods of two edges overlap"
    assert np.all(a >> 31 == 1), "A is v = -x"
    # B touches every bucket at both ends, and the clamps on either side
    bb = lc.f32_bits(-vals["B"])
    first, last = lc.bucket_bounds()
    assert set(first.tolist()) <= set(bb.tolist()) and set(last.tolist()) <= set(bb.tolist())
    assert bb.min() == 1 and bb.max() == lc.INF_BITS
    d = -vals["D"].astype(np.float64)
    assert d[0] == 2.0 ** -6 and d[-1] == 2.0 ** 13 and np.all(np.diff(d) > 0)
    # the list is a function of the thresholds alone
    again = lc.values(cpu["thr"])
    assert all(lc.f32_bits(again[g]).tobytes() == lc.f32_bits(vals[g]).tobytes() for g in "ABCD")


def test_thresholds_are_the_edges_of_the_routine(cpu):
    thr, exact = cpu["thr"], cpu["exact"]
    assert thr[0] == lc.INF_BITS
    x = thr[1:].astype(np.int64)
    assert np.all(np.diff(x) < 0), "thresholds strictly decreasing in k"
    k = np.arange(1, 256)
    assert np.all(exact(-lc.bits_f32(thr[1:])) >= k) and np.all(exact(-lc.bits_f32(thr[1:] + 1)) < k)
    got, allowed = lc.edge_ulps(thr, cpu["m"])
    print(f"cpu: m = {cpu['m']:.3e} levels; thr[255] = {lc.bits_f32(thr[255:])[0]:.5e}, thr[254] = {lc.bits_f32(thr[254:255])[0]:.6f}, "
          f"thr[1] = {lc.bits_f32(thr[1:2])[0]:.2f}; worst edge distance {got[:253].max():.1f} ulp (k <= 253), {got[253]:.1f} ulp (k = 254)")
    assert np.all(got <= allowed), (np.flatnonzero(got > allowed) + 1, got.max())
    assert 0.0 <= lc.bits_f32(thr[255:])[0] <= 1e-6  # 1 - l / 8.7 rounds to 1 below it: no float64 edge to compare with


def test_one_threshold_per_bucket_at_most(cpu):
    b = lc.bucket_of(cpu["thr"][1:])
    n = np.bincount(b, minlength=lc.BUCKETS)
    # bucket 0 takes everything below 2^-6 with it: thr[255] lies there, thr[254] (0.0347) in a bucket of its own
    assert n.max() == 1, np.flatnonzero(n > 1)
    assert b[254] == 0 and b[253] > 0


def test_step_function_on_the_neighbourhoods(cpu):
    """The assumption the tables rest on, for the CPU routine: its byte does not step back within 8 ulp of an edge."""
    u = cpu["exact"](cpu["vals"]["A"]).reshape(255, 17).astype(np.int64)  # x ascending along a row
    assert np.all(np.diff(u, axis=1) <= 0)
    k = np.arange(1, 256)[:, None]
    assert np.all(u[:, :9] == k) and np.all(u[:, 9:] == k - 1)


def test_special_bytes(cpu):
    got = dict(zip([n for n, _ in lc.SPECIALS], cpu["exact"](cpu["vals"]["C"]).tolist()))
    for name, want in lc.SPECIAL_BYTES.items():
        assert got[name] == want, (name, got[name], want)
    assert int(cpu["exact"](np.array([-1e30], np.float32))[0]) == 0
    assert got["-6000"] == 0 and got["-5800.5566"] in (0, 1)  # (the production initial state; thr[1] itself)


def test_float64_decides_the_sweep(cpu):
    """D is usable as a float64 judgement: at most 16 of its 16 384 values lie within m of an integer level, and the CPU routine
    agrees with floor(level64) everywhere else."""
    m = cpu["m"]
    assert 5e-5 < m < 2e-4, m  # 4 x (a few ulp of log1pf at l = 8.7, 2.8e-5 levels each)
    x = -cpu["vals"]["D"]
    und = lc.undecided(x, m)
    print(f"cpu: {int(und.sum())} undecided values on D at m = {m:.3e}")
    assert und.sum() <= 16
    u = cpu["exact"](cpu["vals"]["D"]).astype(np.int64)
    lv = lc.level64(x)
    assert np.array_equal(u[~und], np.floor(lv[~und]).astype(np.int64))
    r = np.round(lv[und]).astype(np.int64)
    assert np.all((u[und] == r) | (u[und] == r - 1))
