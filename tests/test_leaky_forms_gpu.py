"""The four forms of uint8(leaky_transform(.)) at every level edge, bucket and special (tests/leaky_cases.py).

    F0  f32_to_u8(leaky_f(v)), a log1pf per value      k_leaky, csrc/elementwise.hip      frlw_leaky_transform
    F1  leaky_u8_lookup_n<kMaxK>                        the write-out of taf_tile_body     frlw_taf_encode
    F2  leaky_u8_lookup_n<4>                            close_window of taf_tile_body      frlw_taf_encode_chain
    F3  leaky_u8_bucket_n<kMaxK>                        the write-out of kf_taf_walk       frlw_taf_encode_batch

Which call reaches which site, from the code: ``encode_taf_dat(fast=False)`` calls frlw_taf_encode, which launches k_taf_tile =
taf_tile_body<.., SNAP = false> -- the <4> site is under ``if constexpr (SNAP)`` and not compiled into it -- and hands it
out_u8, so every byte comes from the <kMaxK> call in the write-out (csrc/enc_taf.h).  ``encode_taf_chain`` calls
frlw_taf_encode_chain, which launches k_taf_tile_snap (SNAP = true) with out_u8 = NULL: the write-out's look-up is skipped and
every snapshot byte comes from the <4> call in close_window.  ``encode_taf_batch``, and ``encode_taf_dat(fast=True)`` through
it, call frlw_taf_encode_batch, whose only uint8 producer is leaky_u8_bucket_n in kf_taf_walk (csrc/taf_walk.h); the Python
fall-back of ``encode_taf_dat`` to the general path is ruled out here by watching ``encode_taf_batch`` return.

The proof that each call reaches the site named: five builds with one defect each, this file and tests/test_elementwise_gpu.py
(89 tests) run against each on an MI355X.
    (a)  ``xb < t1`` for ``xb <= t1`` in leaky_u8_bucket_n                    12 failed: every F3 case, no F1 / F2 case
    (b)  lut[520] (x from 1 280 to 1 312) one too high in k_leaky_fill        13 failed: every F3 case and F3 after a FIFO step
    (c)  both fabsf dropped in leaky_u8_lookup_n                               0 failed, and no value can make one fail: see below
    (c') fabsf dropped in leaky_u8_lookup, the exact routine behind it        12 failed: every F1 and F2 case and both after a step
    (d)  ``v <= 0`` removed in a copy of leaky_u8_lookup_n for the <4> call    5 failed: every F2 case and F2 after a step
(c): with the sign bit left in ``xb`` the test ``xb > t1 && xb <= t0`` fails for every negative v (also for k = 0, where t0 is the
pattern of +inf), so every value takes leaky_u8_exact, which has its own fabsf: the bytes are F0's for every float, only slower.
The fabsf that carries the -0.0 case is the one in leaky_u8_lookup, which both sites of leaky_u8_lookup_n reach and the bucket
routine reaches for positive v only (where it returns before the fabsf): that is defect (c').

F0 is judged against float64 within m = 4 x the distance of the CPU float32 restatement from float64 on A and D; F1..F3 are
judged against F0 bit for bit on all 23 181 values: a TAF call without events leaves the state alone (fifo_step with
has == false), so each byte is the look-up of the float planted in its slot.  The 5 610 slots of the 17 x 33, K = 5 frame hold
A + B + C (6 797 values) in two plants.

Measured on an MI355X (gfx950), printed by the tests below with ``-s``:
    thr[255] = 2.59280e-07 (bits 0x348b3334), thr[254] = 0.034707, thr[1] = 5800.56; every threshold within 36.4 ulp of the
    float64 edge for k <= 253, 70.6 ulp for k = 254 (allowed: what m levels amount to at that x and one more, 31 to 988 ulp)
    m = 1.041e-04 levels; worst |F0 float32 - level64| on A + B + D = 2.858e-05 levels = 0.27 m
    undecided values on D: 2 of 16 384 (16 allowed); F0's byte is floor(level64) on all others
    no neighbourhood of A where F0's byte steps back; no bucket with two thresholds
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import leaky_cases as lc  # noqa: E402
from frlw_evd_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

WINDOW_US, N_WINDOWS = 10_000, 4
FRAMES = {"32x48_K8": ((32, 48), 8, "ABCD"), "17x33_K5": ((17, 33), 5, "ABC"), "4x640_K8": ((4, 640), 8, "ABCD")}


@pytest.fixture(scope="module")
def er():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from frlw_evd_amd import event_representation
    return event_representation


def host(t):
    return t.cpu().numpy()


def f0(v, want_f32=True, want_u8=True):
    """frlw_leaky_transform on the float32 array ``v`` -> (float32 or None, uint8 or None)."""
    from frlw_evd_amd import _lib
    src = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32).reshape(-1).copy()).cuda()
    f = torch.empty_like(src) if want_f32 else None
    u = torch.empty(src.shape, dtype=torch.uint8, device="cuda") if want_u8 else None
    rc = _lib.load().frlw_leaky_transform(C.c_void_p(src.data_ptr()), src.numel(), C.c_void_p(f.data_ptr()) if want_f32 else None,
                                          C.c_void_p(u.data_ptr()) if want_u8 else None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "frlw_leaky_transform")
    torch.cuda.synchronize()
    return (host(f) if want_f32 else None), (host(u) if want_u8 else None)


@pytest.fixture(scope="module")
def dev(er):
    """The device's thresholds through the public exact entry, the list built on them, F0 on the list once."""
    from oracle import oracle as orc
    thr = lc.thresholds(lambda v: f0(v, want_f32=False)[1])
    vals = lc.values(thr)
    out = {"thr": thr, "vals": vals}
    for g in "ABCD":
        out["f32_" + g], out["u8_" + g] = f0(vals[g])
    x = -lc.flat(vals, "AD")
    out["m"] = lc.margin(orc.leaky_transform(-x), x)
    return out


# ---- F0 against float64 ---------------------------------------------------------------------------------------------------
def test_f0_float32_within_the_margin_of_float64(dev):
    m = dev["m"]
    worst = 0.0
    for g in "ABD":
        d = np.abs(dev["f32_" + g].astype(np.float64) - lc.level64(-dev["vals"][g].astype(np.float64)))
        assert not np.isnan(d).any(), g
        worst = max(worst, float(d.max()))
        assert d.max() <= m, (g, float(d.max()), m, dev["vals"][g][np.argmax(d)])
    t = lc.bits_f32(dev["thr"])
    print(f"device: thr[255] = {t[255]:.5e} ({int(dev['thr'][255]):#010x}), thr[254] = {t[254]:.6f}, thr[1] = {t[1]:.2f}; "
          f"m = {m:.3e} levels; worst |F0 - level64| = {worst:.3e} = {worst / m:.2f} m")


def test_f0_byte_is_the_floor_of_float64_on_the_sweep(dev):
    m = dev["m"]
    x = -dev["vals"]["D"].astype(np.float64)
    und = lc.undecided(x, m)
    print(f"device: {int(und.sum())} undecided values on D at m = {m:.3e}")
    assert und.sum() <= 16
    u = dev["u8_D"].astype(np.int64)
    lv = lc.level64(x)
    bad = np.flatnonzero(u[~und] != np.floor(lv[~und]).astype(np.int64))
    assert bad.size == 0, (x[~und][bad[:5]], u[~und][bad[:5]], lv[~und][bad[:5]])
    r = np.round(lv[und]).astype(np.int64)
    assert np.all((u[und] == r) | (u[und] == r - 1)), (x[und], u[und], lv[und])


def test_f0_u8_is_the_truncation_of_its_float32(dev):
    for g in "ABCD":
        assert np.array_equal(dev["u8_" + g], lc.u8_rule(dev["f32_" + g])), g


# ---- the step-function assumption ------------------------------------------------------------------------------------------
def test_f0_is_a_step_function_around_every_edge(dev):
    """Non-increasing in x over the 17 bit patterns around each of the 255 edges; the bisection's answer is the only step."""
    u = dev["u8_A"].reshape(255, 17).astype(np.int64)  # x ascending along a row
    back = np.argwhere(np.diff(u, axis=1) > 0)
    assert back.size == 0, [(int(k) + 1, lc.f32_bits(dev["vals"]["A"].reshape(255, 17)[k]).tolist(), u[k].tolist()) for k, _ in back[:3]]
    k = np.arange(1, 256)[:, None]
    assert np.all(u[:, :9] == k) and np.all(u[:, 9:] == k - 1)


def test_device_thresholds(dev):
    thr = dev["thr"]
    assert thr[0] == lc.INF_BITS
    assert np.all(np.diff(thr[1:].astype(np.int64)) < 0), "thresholds strictly decreasing in k"
    got, allowed = lc.edge_ulps(thr, dev["m"])
    print(f"device: worst edge distance {got[:253].max():.1f} ulp (k <= 253), {got[253]:.1f} ulp (k = 254)")
    assert np.all(got <= allowed), (np.flatnonzero(got > allowed) + 1, got.max())
    assert 0.0 <= lc.bits_f32(thr[255:])[0] <= 1e-6
    n = np.bincount(lc.bucket_of(thr[1:]), minlength=lc.BUCKETS)
    assert n.max() == 1, "a bucket with two thresholds: the library would (rightly) leave the bucket table unused"


def test_f0_specials(dev):
    got = dict(zip([n for n, _ in lc.SPECIALS], dev["u8_C"].tolist()))
    for name, want in lc.SPECIAL_BYTES.items():
        assert got[name] == want, (name, got[name], want)
    b = dict(zip(lc.f32_bits(dev["vals"]["B"]).tolist(), dev["u8_B"].tolist()))
    assert b[int(lc.f32_bits(np.float32(-1e30))[0])] == 0 and b[0x80000000 | lc.INF_BITS] == 0
    assert b[0x80000001] == 255 and b[0x80000000 | lc.FLT_MIN_BITS] == 255


# ---- F1, F2, F3 against F0, bit for bit ------------------------------------------------------------------------------------
def plants(dev, frame, n_seq=1):
    """The frame's share of the list, padded by repetition, as state tensors (n_seq, H, W, 2, K) with the F0 byte of every slot:
    as many plants as it takes to send every value through."""
    (H, W), K, groups = FRAMES[frame]
    v = lc.flat(dev["vals"], groups)
    u = np.concatenate([dev["u8_" + g] for g in groups])
    slots = n_seq * H * W * 2 * K
    out = []
    for at in range(0, len(v), slots):
        idx = np.resize(np.arange(at, min(at + slots, len(v))), slots)
        out.append((v[idx].reshape(n_seq, H, W, 2, K).copy(), u[idx].reshape(n_seq, H, W, 2, K).copy()))
    assert sum(min(slots, len(v) - at) for at in range(0, len(v), slots)) == len(v)
    return out


def as_view(st):
    """(H, W, 2, K) -> (2K, H, W), generate_taf.py:55."""
    H, W, _, K = st.shape
    return np.ascontiguousarray(st.transpose(3, 2, 0, 1)).reshape(2 * K, H, W)


def as_volume(by_slot, flip_k):
    """Per-slot bytes (H, W, 2, K) -> the uint8 volume (K, 2, H, W), newest slot first with flip_k."""
    vol = np.ascontiguousarray(by_slot.transpose(3, 2, 0, 1))
    return np.ascontiguousarray(vol[::-1]) if flip_k else vol


def same_bytes(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if got.tobytes() != want.tobytes():
        g, w = got.reshape(-1).view(np.uint8 if got.dtype == np.uint8 else np.uint32), want.reshape(-1).view(np.uint8 if got.dtype == np.uint8 else np.uint32)
        bad = np.flatnonzero(g != w)
        raise AssertionError(f"{what}: {bad.size} of {g.size} differ, first at {bad[:6]}: {g[bad[:6]]} vs {w[bad[:6]]}")


def no_events():
    return torch.empty((0, 8), dtype=torch.uint8, device="cuda")


def check_volume(u8, planted, f0_bytes, flip_k, what):
    """Every byte is F0 of the float in its slot; on a mismatch name the floats."""
    want = as_volume(f0_bytes, flip_k)
    if u8.tobytes() != want.tobytes():
        src = as_volume(planted.view(np.uint32), flip_k)
        bad = np.flatnonzero(u8.reshape(-1) != want.reshape(-1))
        vb = np.unique(src.reshape(-1)[bad])
        raise AssertionError(f"{what}: {bad.size} bytes differ from F0 at {vb.size} distinct floats, e.g. bits {[hex(int(b)) for b in vb[:6]]}: "
                             f"{u8.reshape(-1)[bad[:6]]} vs F0 {want.reshape(-1)[bad[:6]]}")


@pytest.fixture
def fast_calls(er, monkeypatch):
    """Counts the encode_taf_batch calls that RETURNED: encode_taf_dat(fast=True) falls back to the general path when that call
    raises, and a test of F3 must not pass on F1's bytes."""
    served = []
    inner = er.encode_taf_batch

    def spy(*a, **kw):
        out = inner(*a, **kw)
        served.append(1)
        return out
    monkeypatch.setattr(er, "encode_taf_batch", spy)
    return served


@pytest.mark.parametrize("flip_k", [True, False])
@pytest.mark.parametrize("frame", list(FRAMES))
def test_f1_general_path(er, dev, frame, flip_k):
    (H, W), K, _ = FRAMES[frame]
    for i, (planted, want) in enumerate(plants(dev, frame)):
        st = torch.from_numpy(planted[0]).cuda()
        u8, view = er.encode_taf_dat(no_events(), (H, W), st, 0, WINDOW_US, N_WINDOWS, K, want_view=True, flip_k=flip_k, fast=False)
        same_bytes(host(st), planted[0], f"state, plant {i}")
        same_bytes(host(view), as_view(planted[0]), f"view, plant {i}")
        check_volume(host(u8), planted[0], want[0], flip_k, f"F1 {frame} flip_k={flip_k} plant {i}")


@pytest.mark.parametrize("flip_k", [True, False])
@pytest.mark.parametrize("frame", ["32x48_K8", "17x33_K5"])
def test_f2_chain_snapshots(er, dev, frame, flip_k):
    (H, W), K, _ = FRAMES[frame]
    for i, (planted, want) in enumerate(plants(dev, frame)):
        st = torch.from_numpy(planted[0]).cuda()
        snaps = host(er.encode_taf_chain(no_events(), (H, W), st, 0, WINDOW_US, [1, 2, 1], K, flip_k=flip_k))
        same_bytes(host(st), planted[0], f"state, plant {i}")
        assert snaps.shape == (3, K, 2, H, W)
        for s in range(3):
            check_volume(snaps[s], planted[0], want[0], flip_k, f"F2 {frame} flip_k={flip_k} plant {i} step {s}")


@pytest.mark.parametrize("flip_k", [True, False])
@pytest.mark.parametrize("frame", list(FRAMES))
def test_f3_fast_walk(er, dev, fast_calls, frame, flip_k):
    (H, W), K, _ = FRAMES[frame]
    n = 0
    for i, (planted, want) in enumerate(plants(dev, frame)):
        st = torch.from_numpy(planted[0]).cuda()
        u8, view = er.encode_taf_dat(no_events(), (H, W), st, 0, WINDOW_US, N_WINDOWS, K, want_view=True, flip_k=flip_k, fast=True)
        n += 1
        assert len(fast_calls) == n, "encode_taf_dat(fast=True) was not served by the fast path"
        same_bytes(host(st), planted[0], f"state, plant {i}")
        same_bytes(host(view), as_view(planted[0]), f"view, plant {i}")
        check_volume(host(u8), planted[0], want[0], flip_k, f"F3 {frame} flip_k={flip_k} plant {i}")


@pytest.mark.parametrize("flip_k", [True, False])
@pytest.mark.parametrize("frame", list(FRAMES))
def test_f3_batch_of_two_sequences(er, dev, frame, flip_k):
    """Two sequences that hold halves of the list (the plant runs through both states back to back)."""
    (H, W), K, _ = FRAMES[frame]
    for i, (planted, want) in enumerate(plants(dev, frame, n_seq=2)):
        st = torch.from_numpy(planted).cuda()
        u8, view = er.encode_taf_batch(no_events(), [0, 0, 0], (H, W), st, 0, WINDOW_US, N_WINDOWS, K, want_view=True, flip_k=flip_k)
        same_bytes(host(st), planted, f"state, plant {i}")
        for s in range(2):
            same_bytes(host(view[s]), as_view(planted[s]), f"view, plant {i}, sequence {s}")
            check_volume(host(u8[s]), planted[s], want[s], flip_k, f"F3 batch {frame} flip_k={flip_k} plant {i} sequence {s}")


# ---- with events: the look-up on what a FIFO step produced ------------------------------------------------------------------
EV_FRAME = "32x48_K8"
EV_CORNER = (8, 16)  # rows, columns that take events


def corner_events():
    return synth.to_dat8(synth.synth_events(707, 300, EV_CORNER[1], EV_CORNER[0], WINDOW_US))


def check_stepped(planted, after):
    """Cells outside the corner took no event in a window that has events: every slot is st - 1.0f."""
    want = (planted - np.float32(1.0))[:, EV_CORNER[1]:]
    got = after[:, EV_CORNER[1]:]
    ok = ~np.isnan(want)
    assert np.array_equal(got.view(np.uint32)[ok], want.view(np.uint32)[ok]) and np.isnan(got[~ok]).all()
    assert not np.array_equal(after[:EV_CORNER[0], :EV_CORNER[1]].view(np.uint32),
                              (planted - np.float32(1.0))[:EV_CORNER[0], :EV_CORNER[1]].view(np.uint32)), "no cell took an event"


@pytest.mark.parametrize("form", ["F1", "F2", "F3"])
def test_forms_after_a_fifo_step(er, dev, fast_calls, form):
    """300 events in the corner tile, one window: the judge is F0 applied to the floats the call left (the view it returned,
    which is held bit-exact to the oracle elsewhere)."""
    (H, W), K, _ = FRAMES[EV_FRAME]
    planted = plants(dev, EV_FRAME)[0][0][0]
    rec = corner_events()
    d = torch.from_numpy(rec.view(np.uint8).reshape(-1, 8).copy()).cuda()
    st = torch.from_numpy(planted).cuda()
    if form == "F2":
        u8 = host(er.encode_taf_chain(d, (H, W), st, 0, WINDOW_US, [1], K))[0]
        after = host(st)
    else:
        u8, view = er.encode_taf_dat(d, (H, W), st, 0, WINDOW_US, 1, K, want_view=True, fast=(form == "F3"))
        assert len(fast_calls) == (1 if form == "F3" else 0)
        u8, after = host(u8), host(st)
        same_bytes(host(view), as_view(after), "the returned view is the state the call left")
    check_stepped(planted, after)
    want = f0(after, want_f32=False)[1].reshape(after.shape)
    check_volume(u8, after, want, True, f"{form} after a FIFO step")
