"""The cell means of kf_taf_walk (csrc/taf_walk.h, phase 2) on both sides of the reciprocal table's end, against the CPU oracle,
bit for bit: a wavefront whose counts all lie below kMeanTab = 64 takes mean_by_recip (csrc/taf_mean.h; the arithmetic itself is
checked for every reachable sum by tests/test_walk_mean_cpu.py), one with a larger count divides.

The stream is a few thousand time-sorted events on a 64 x 32 frame: ONE tile whose sub-tile 0 is the frame's rows 0 and 1; the
wavefronts of phase 2 own 32 pixels x 2 polarities each (row 0: x < 32 and x >= 32).  Row 0 carries only hand-placed records:

  window 1       x <  32: cells with exactly 1, 2, 3, 7, 62, 63 records (table);  x >= 32: 64, 65, 300 next to 1, 2, 63 (division)
  window 0       a cell whose only record has r = 0 (value -1 exactly)
  window 2       empty in the whole sequence (generate_taf.py:40-41: no step)
  window 3       events in other sub-tiles only
  last window    a cell whose only record has r = window_us (value +0: the sum is +0 with n = 1); x >= 32: 1, 2, 63 records;
                 with 9 windows it is the second round of windows, and x < 32 gets a cell with 64 records there: each of the two
                 wavefronts takes the table in one round and the division in the other
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from frlw_evd_amd import synth  # noqa: E402
from golden_util import assert_bitexact  # noqa: E402

pytestmark = pytest.mark.gpu

H, W, WIN, T0 = 32, 64, 10_000, 1_000


def _stream(n_win):
    rng = np.random.default_rng(640)
    ev = []  # (t, x, y, p)

    def cell(window, x, p, n):  # n records of cell (x, row 0, p) inside `window`, at distinct random times
        for r in rng.choice(np.arange(1, WIN), size=n, replace=False):
            ev.append((T0 + window * WIN + int(r), x, 0, p))

    last = n_win - 1
    for x, p, n in ((0, 0, 1), (0, 1, 2), (1, 0, 3), (2, 1, 7), (3, 0, 62), (4, 1, 63),                # wavefront 0: all below 64
                    (32, 0, 64), (33, 1, 65), (34, 0, 300), (35, 0, 1), (36, 1, 2), (37, 0, 63)):     # wavefront 1: 64 and more
        cell(1, x, p, n)
    ev.append((T0, 10, 0, 0))                      # r = 0
    ev.append((T0 + n_win * WIN, 11, 0, 1))        # r = window_us: the end of the last window belongs to it (generate_taf.py:197-203)
    for x, p, n in ((35, 0, 1), (36, 1, 2), (37, 0, 63)):
        cell(last, x, p, n)
    if n_win > 8:
        cell(last, 5, 0, 64)
        cell(last, 0, 0, 3)
    # the other rows (row 1 belongs to sub-tile 0 as well): a few thousand random events, none in window 2, in window 3 none in sub-tile 0
    n_bg = 2500
    bt = rng.integers(0, n_win * WIN, size=n_bg)
    by = rng.integers(1, H, size=n_bg)
    bx = rng.integers(0, W, size=n_bg)
    bp = rng.integers(0, 2, size=n_bg)
    bw = bt // WIN
    keep = (bw != 2) & ~((bw == 3) & (by < 2))
    ev += [(T0 + int(t), int(x), int(y), int(p)) for t, x, y, p in zip(bt[keep], bx[keep], by[keep], bp[keep])]
    ev.sort(key=lambda e: e[0])  # (stable: window-sorted time order)
    a = np.array(ev, dtype=np.int64)
    rec = synth.to_dat8({"t": a[:, 0], "x": a[:, 1], "y": a[:, 2], "p": a[:, 3]})
    # the stream is what the docstring says
    w = np.minimum((a[:, 0] - T0) // WIN, n_win - 1)
    row0 = a[:, 2] == 0
    counts = sorted(np.unique(a[row0 & (w == 1)][:, [1, 3]], axis=0, return_counts=True)[1].tolist())
    assert counts == [1, 1, 2, 2, 3, 7, 62, 63, 63, 64, 65, 300]
    assert not (w == 2).any() and (w == 3).any() and not ((w == 3) & (a[:, 2] < 2)).any()
    return rec


@pytest.fixture(scope="module")
def cases():
    """Stream, prior state and the oracle's results per (K, windows): computed once, shared by the forms."""
    from oracle import oracle as orc
    out = {}
    for K in (8, 4):
        for n_win in (8, 9):
            rec = _stream(n_win)
            state0 = np.random.default_rng(7 * K + n_win).uniform(-50, 0, (H, W, 2, K)).astype(np.float32)
            view, st = orc.taf_stream_dat8(rec, (H, W), (H, W), K, T0, WIN, n_win, state0)
            u8 = np.ascontiguousarray(orc.quantize_u8(orc.leaky_transform(view.reshape(K, 2, H, W)))[::-1])
            out[(K, n_win)] = (rec, state0, view, st, u8)
    return out


@pytest.mark.parametrize("n_win", [8, 9])
@pytest.mark.parametrize("K", [8, 4])
@pytest.mark.parametrize("form", ["tile_bins", "direct"])
def test_counts_on_both_sides_of_the_table_against_the_oracle(cases, monkeypatch, form, K, n_win):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from frlw_evd_amd import _lib, event_representation as er
    rec, state0, oview, ost, ou8 = cases[(K, n_win)]
    # tile bins + kf_split_whole<true> + kf_taf_walk<., false> / sub-tile bins + kf_taf_walk<., true> (it gathers its own list)
    monkeypatch.setattr(er, "TUNING", _lib.FrlwTuning(chunk_major=1, direct_bins=0 if form == "tile_bins" else 1))
    dat = torch.from_numpy(np.ascontiguousarray(rec).view(np.uint8).reshape(-1, 8).copy()).cuda()
    st = torch.from_numpy(state0.copy()).cuda().view(1, H, W, 2, K)
    u8, view = er.encode_taf_batch(dat, [0, len(rec)], (H, W), st, T0, WIN, n_win, K, want_view=True)
    assert_bitexact(st[0].cpu().numpy(), ost, "state")
    assert_bitexact(view[0].cpu().numpy(), oview, "view")
    assert_bitexact(u8[0].cpu().numpy(), ou8, "uint8")
    assert not np.array_equal(ost, state0)
