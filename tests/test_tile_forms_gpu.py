"""Every form of the general path's tile kernels (csrc/enc_*.h, launched by csrc/encoders.hip) alone, against the CPU oracle.

The tile kernels exist for NT = 256, 512 and 1024 threads (``tile_width_log2`` 6, 7, 8) and, for Event Volume and TAF, in
three launch modes: every tile as four one-cell-per-thread quarters (small frames), whole tiles (four cells per thread), and
whole tiles with the listed hot tiles as quarters in the same launch.  The frames of the other tests pick a few of these by
their size; here ``frlw_tuning_t`` forces each one on ONE small stream whose frame is ragged on both edges at every width
and whose busiest tile needs more than one counting-sort slice.  The scatter's staged form and the TAF partition without
its value table, which the sizes of the suite never select, get a row each.

Bars as in tests/test_encoders_gpu.py: bit-exact f32; after expf / log1pf 2 ulp and the uint8 1-LSB budget of the small samples.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from frlw_evd_amd import synth  # noqa: E402
from golden_util import LAMDAS, assert_bitexact, assert_u8_budget  # noqa: E402

pytestmark = pytest.mark.gpu

H, W, N, SPAN = 20, 300, 60_000, 80_000
WINDOW_US, N_WINDOWS = 10_000, 8
SLICE_MULT, TILE_H, MAX_HOT = 16, 8, 32  # kSliceMult, kTileH, kMaxHot (csrc/frlw_consts.h)
HOT_RECORDS = 2000
SAE_NOW, SAE_WINDOW = 80_000, 1_000_000  # now - window lies in front of the stream: the time filter runs and drops nothing
MODES = {"quarter": {}, "whole": dict(quarter_below=0, hot_tile_records=2 ** 30),
         "hot": dict(quarter_below=0, hot_tile_records=HOT_RECORDS)}


@pytest.fixture(scope="module")
def er():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from frlw_evd_amd import event_representation
    return event_representation


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def to_dev(rec):
    return torch.from_numpy(rec.view(np.uint8).reshape(-1, 8).copy()).cuda()


def host(t):
    return t.cpu().numpy()


def assert_ulp(got, want, ulps, what):
    a = np.ascontiguousarray(got).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(want).view(np.int32).astype(np.int64)
    assert np.abs(a - b).max() <= ulps, f"{what}: {np.abs(a - b).max()} ulp"


def tile_counts(ev, twl):
    """Records per tile ((1 << twl) x 8 pixels) of the stream, as the partition counts them."""
    tiles_x = (W + (1 << twl) - 1) >> twl
    tiles_y = (H + TILE_H - 1) // TILE_H
    tile = (ev["y"] // TILE_H) * tiles_x + (ev["x"] >> twl)
    return np.bincount(tile, minlength=tiles_x * tiles_y)


@pytest.fixture(scope="module")
def stream():
    """The one stream of this module, time-sorted and under a fixed permutation (windows interleave: the tile kernel's
    general, one-pass-per-window path)."""
    ev = synth.synth_events(41, N, W, H, SPAN, hotspot=True)
    perm = np.random.default_rng(5).permutation(N)
    return {"ev": ev, "sorted": synth.to_dat8(ev), "shuffled": synth.to_dat8({k: v[perm] for k, v in ev.items()})}


def test_stream_has_the_shape_the_forms_need(stream):
    """What makes the cases below mean something, recomputed: ragged right column and bottom row at every width, the
    busiest tile longer than one slice, tiles on both sides of the hot threshold, and few enough wavefronts for the default
    mode to be all-quarters."""
    want = {6: (15, 9568, 3), 7: (9, 13420, 2), 8: (6, 21224, 2)}
    for twl in (6, 7, 8):
        nt, c = 4 << twl, tile_counts(stream["ev"], twl)
        assert W % (1 << twl) == 44 and H % TILE_H == 4
        assert c.max() > SLICE_MULT * nt, (twl, c.max())
        assert c.min() < HOT_RECORDS < c.max(), (twl, c.min(), c.max())
        assert 0 < (c > HOT_RECORDS).sum() <= MAX_HOT and (c <= HOT_RECORDS).sum() > 0
        assert len(c) * (nt // 64) <= 1024
        assert (len(c), int(c.max()), -(-int(c.max()) // (SLICE_MULT * nt))) == want[twl]
        assert int(c.min()) == 1258


def header_words(er):
    """pad (tiles of the last TAF launch that took the window-interleaved loop), n_hot and hot_thr of the cached workspace's header
    (csrc/frlw_common.h WsHeader: status, pad, wmask, n_hot, hot_thr), which every partition resets and the tile kernels read."""
    w = er._workspace(N, H, W, torch.device("cuda", torch.cuda.current_device()))[:24].cpu().numpy().view(np.uint32)
    return int(w[1]), int(w[4]), int(w[5])


def state0(K):
    return np.random.default_rng(K).uniform(-50, 0, size=(H, W, 2, K)).astype(np.float32)


@pytest.fixture(scope="module")
def want(orc, stream):
    """The oracle's results, computed once for all the cases (none of them is modified)."""
    out = {}
    dat = stream["sorted"]
    for bins in (5, 8):
        out["ev", bins] = orc.ev_stream_dat8(dat, (H, W), (H, W), bins, SPAN, SPAN)
    for K in (8, 5):
        for order in ("sorted", "shuffled"):
            view, st = orc.taf_stream_dat8(stream[order], (H, W), (H, W), K, 0, WINDOW_US, N_WINDOWS, state0(K))
            u8 = orc.quantize_u8(orc.leaky_transform(view.reshape(K, 2, H, W)))
            out["taf", K, order] = (view, st, np.ascontiguousarray(u8[::-1]))  # flip_k: newest slot first
    out["eci"] = orc.eci_stream_dat8(dat, (H, W), (H, W))
    out["eci_u8"] = orc.quantize_u8(out["eci"])
    out["sae"] = orc.sae_stream_dat8(dat, (H, W), (H, W), LAMDAS, None, SAE_NOW, SAE_WINDOW)
    out["sae_u8"] = orc.quantize_u8(out["sae"][0])
    return out


ROWS = [pytest.param(twl, mode, {}, id=f"w{twl}-{mode}") for twl in (6, 7, 8) for mode in MODES] + \
       [pytest.param(7, "whole", dict(staged_scatter=1), id="w7-whole-staged_scatter"),
        pytest.param(7, "whole", dict(no_value_table=1), id="w7-whole-no_value_table")]


@pytest.mark.parametrize("twl,mode,extra", ROWS)
def test_ev_and_taf_tile_forms(er, stream, want, monkeypatch, twl, mode, extra):
    """k_ev_tile5 / k_ev_tile / k_taf_tile at one width in one launch mode: Event Volume with 5 and 8 bins, TAF with K = 8
    and K = 5 (state, f32 view, flipped uint8) on the sorted stream and on the shuffled one."""
    from frlw_evd_amd import _lib
    monkeypatch.setattr(er, "TUNING", _lib.FrlwTuning(tile_width_log2=twl, **MODES[mode], **extra))
    what = f"width {twl} {mode} {extra}"
    d = {order: to_dev(stream[order]) for order in ("sorted", "shuffled")}
    n_listed = int((tile_counts(stream["ev"], twl) > HOT_RECORDS).sum())
    for bins in (5, 8):
        out, _ = er.encode_ev_dat(d["sorted"], (H, W), SPAN, SPAN, volume_bins=bins, fast=False)
        assert_bitexact(host(out), want["ev", bins], f"ev bins={bins}, {what}")
        # WHICH form ran: the hot list holds exactly the tiles above the threshold in "hot" mode and nothing in "whole" mode
        _, n_hot, hot_thr = header_words(er)
        if mode == "hot":
            assert (n_hot, hot_thr) == (n_listed, HOT_RECORDS), (n_hot, hot_thr)
        elif mode == "whole":
            assert n_hot == 0, n_hot
    for K in (8, 5):
        for order in ("sorted", "shuffled"):
            oview, ost, ou8 = want["taf", K, order]
            st = torch.from_numpy(state0(K)).cuda()
            u8, view = er.encode_taf_dat(d[order], (H, W), st, 0, WINDOW_US, N_WINDOWS, K, want_view=True, want_u8=True,
                                         fast=False)
            assert_bitexact(host(st), ost, f"taf state K={K} {order}, {what}")
            assert_bitexact(host(view), oview, f"taf view K={K} {order}, {what}")
            assert_u8_budget(host(u8), ou8, 1e-4, f"taf u8 K={K} {order}, {what}")
            # the sorted stream stays on the window-sorted loop in every tile, the shuffled one leaves it
            pad, n_hot, _ = header_words(er)
            assert (pad > 0) == (order == "shuffled"), (order, pad)
            assert n_hot == (n_listed if mode == "hot" else n_hot if mode == "quarter" else 0), (mode, n_hot)


@pytest.mark.parametrize("twl", [6, 7, 8])
def test_eci_and_sae_tile_forms(er, stream, want, monkeypatch, twl):
    """k_eci_tile / k_sae_tile at one width (they have no quarter or hot form); staged_scatter = 0 keeps both calls on the
    general path."""
    from frlw_evd_amd import _lib
    monkeypatch.setattr(er, "TUNING", _lib.FrlwTuning(tile_width_log2=twl, staged_scatter=0))
    d = to_dev(stream["sorted"])
    out, u8 = er.encode_eci_dat(d, (H, W), want_u8=True)
    assert_bitexact(host(out), want["eci"], f"eci, width {twl}")
    assert_bitexact(host(u8), want["eci_u8"], f"eci u8, width {twl}")
    oo, omem = want["sae"]
    o, su8, mem = er.encode_sae_dat(d, (H, W), LAMDAS, None, SAE_NOW, SAE_WINDOW, want_u8=True)
    assert_bitexact(host(mem), omem, f"sae memory, width {twl}")
    assert_ulp(host(o), oo, 2, f"sae out, width {twl}")
    assert_u8_budget(host(er.quantize_u8(o)), want["sae_u8"], 1e-4, f"sae u8, width {twl}")
    assert_u8_budget(host(su8), want["sae_u8"], 1e-4, f"sae u8 written by the kernel, width {twl}")

