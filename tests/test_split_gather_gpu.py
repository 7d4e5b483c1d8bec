"""kf_split_whole<true> finds rec[]'s index of a list position through the block address table (csrc/taf_blocktab.h; the arithmetic
itself: tests/test_blocktab_cpu.py), and kf_taf_walk<., false> takes its row of the window table with the header words, whatever
the tile's flag says.  The check is the CPU oracle, bit for bit, on streams BUILT so that the table meets the shapes at which it
can go wrong.  A run is what one (sequence, tile) has inside one chunk of the stream; these calls (chunk-major partition, fewer than
512 * 8192 events) are cut into chunks of 8192 events (csrc/taf_plan.h: `cm && k == 1`), so a stream is laid out here chunk by
chunk, with a chosen number of events per tile in every chunk:
  1. runs shorter than 16 records, several boundaries inside one block of 16 positions (the fallback), next to a skewed tile;
  2. chunks in which a tile has no record (empty runs between non-empty ones, at the front and at the end), a tile without any;
  3. run boundaries exactly on multiples of 16; lists of exactly 16 k, of 8192 and of 8193 records (the staging-chunk edge);
  4. a tile just below and just above whole_max_of(pairs) (8192 with fewer than 256 pairs): the one above goes through the
     segment kernels and must come out the same;
  5. a batch of sequences with different chunk counts, one of them empty;
  6. a time-reversed sequence (TileP::wst_flag 2), a sequence whose first and last windows are empty (flag 1, rows with "none" at
     both ends), an empty and a skewed tile (flag 0: the row is read and ignored).
Frames of 3 to 9 tiles (a tile is 256 x 8 pixels on these frames), at most 150 000 events per case."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from frlw_evd_amd import synth  # noqa: E402
from golden_util import assert_bitexact, assert_u8_budget  # noqa: E402

pytestmark = pytest.mark.gpu

CHUNK = 8192
W = 250


def frame(tiles):
    return 8 * tiles - 3, W  # ragged at the lower edge


def stream(counts, tiles, seed, t_lo, t_hi, reverse=False):
    """One sequence: counts[c][t] events of tile t in chunk c, shuffled inside the chunk; every chunk but the last holds CHUNK
    events.  Times ascend over the stream (descend with `reverse`) inside [t_lo, t_hi)."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1, tiles)
    assert (counts >= 0).all() and (counts[:-1].sum(axis=1) == CHUNK).all() and counts[-1].sum() <= CHUNK, counts.sum(axis=1)
    H, _ = frame(tiles)
    rng = np.random.default_rng(seed)
    tile = np.concatenate([rng.permutation(np.repeat(np.arange(tiles), row)) for row in counts]) if counts.sum() else np.zeros(0, np.int64)
    n = len(tile)
    rows = np.minimum(8, H - 8 * tile)
    t = np.sort(rng.integers(t_lo, t_hi, n))
    ev = {"x": rng.integers(0, W, n), "y": 8 * tile + rng.integers(0, 1 << 30, n) % np.maximum(rows, 1), "p": rng.integers(0, 2, n),
          "t": t[::-1].copy() if reverse else t}
    return synth.to_dat8(ev), counts.sum(axis=0)


def filled(part, tiles, n_chunks, last=CHUNK):
    """part: {tile: per-chunk counts}; the last tile takes what is left of every chunk (`last` events in the last chunk)."""
    c = np.zeros((n_chunks, tiles), dtype=np.int64)
    for t, v in part.items():
        c[:, t] = v
    room = np.full(n_chunks, CHUNK)
    room[-1] = last
    c[:, tiles - 1] = room - c.sum(axis=1)
    return c


def spread(total, n_chunks, rng):
    """`total` events over n_chunks chunks, unevenly."""
    return rng.multinomial(total, rng.dirichlet(np.full(n_chunks, 2.0)))


def case_short_runs():
    tiles, nc, rng = 9, 18, np.random.default_rng(101)
    part = {t: rng.integers(1, 16, nc) for t in range(7)}  # 1 .. 15 records per run: up to a dozen boundaries in a block
    part[2] = np.full(nc, 1)                                # 16 boundaries in every block
    part[7] = rng.integers(0, 41, nc)                       # runs around the block size, some of them empty
    rec, per_tile = stream(filled(part, tiles, nc), tiles, 1, 0, 80_000)
    assert per_tile[:8].max() < 1000 and per_tile[8] > CHUNK  # few events per tile, next to a skewed one
    return tiles, [rec]


def case_empty_runs():
    tiles, nc = 5, 12
    part = {0: [0, 0, 7, 0, 0, 20, 3, 0, 0, 0, 300, 0],      # empty at both ends and in between
            1: np.zeros(nc, dtype=np.int64),                  # a tile without any record
            2: [25, 0] * 6,
            3: [0] * 11 + [5000]}                             # one run only, in the last chunk
    rec, per_tile = stream(filled(part, tiles, nc, last=6000), tiles, 2, 0, 80_000)
    assert per_tile[1] == 0 and per_tile[3] == 5000
    return tiles, [rec]


def case_multiples_of_16():
    tiles, nc = 5, 17
    part = {0: [16, 32, 16, 48, 16, 16, 64, 16, 32, 16, 16, 16, 80, 16, 16, 32, 16],  # every boundary on a multiple of 16; a list of 16 k
            1: [512] * 16 + [0],                                                          # 8192 records: a whole staging chunk, no more
            2: [512] * 16 + [1],                                                          # 8193
            3: [16, 16, 16, 0, 32, 16, 5, 11, 16, 16, 16, 16, 16, 16, 16, 16, 9]}        # on and off the multiples
    rec, per_tile = stream(filled(part, tiles, nc, last=3000), tiles, 3, 0, 80_000)
    assert per_tile[0] % 16 == 0 and per_tile[1] == 8192 and per_tile[2] == 8193
    return tiles, [rec]


def case_whole_tile_limit():
    tiles, nc, rng = 3, 16, np.random.default_rng(104)
    part = {0: spread(8191, nc, rng), 1: spread(8193, nc, rng)}  # whole_max_of(3 pairs) = 8192
    rec, per_tile = stream(filled(part, tiles, nc, last=7000), tiles, 4, 0, 80_000)
    assert per_tile[0] == 8191 and per_tile[1] == 8193
    return tiles, [rec]


def case_batch():
    tiles, rng = 9, np.random.default_rng(105)

    def even(nc, last, tiny=None):
        part = {t: rng.integers(700, 1000, nc) for t in range(tiles - 1)}
        if tiny is not None:
            part[tiny] = np.full(nc, 3)
        c = filled(part, tiles, nc, last)
        c[-1, :tiles - 1] = c[-1, :tiles - 1] * last // CHUNK
        c[-1, tiles - 1] = last - c[-1, :tiles - 1].sum()
        return c
    recs = [stream(even(6, CHUNK), tiles, 5, 0, 2931)[0], stream(np.zeros((1, tiles)), tiles, 6, 0, 2931)[0],
            stream(even(3, 3616), tiles, 7, 0, 2931)[0], stream(even(7, 8000, tiny=4), tiles, 8, 0, 2931)[0]]
    assert [len(r) for r in recs] == [6 * CHUNK, 0, 2 * CHUNK + 3616, 6 * CHUNK + 8000]  # 6, 1 (empty), 3 and 7 chunks
    return tiles, recs


def case_window_flags():
    tiles, rng = 3, np.random.default_rng(106)
    c0 = [[2700, 2692, 2800], [2600, 2808, 2784], [2600, 2300, 2416]]  # 7900, 7800 and 8000 records: all three tiles whole
    rev = stream(c0, tiles, 9, 0, 80_000, reverse=True)[0]                                            # every list runs backwards: flag 2
    c1 = filled({0: spread(7000, 3, rng), 1: np.zeros(3, dtype=np.int64)}, tiles, 3, last=7300)      # tile 1 empty, tile 2 skewed: flag 0
    mid = stream(c1, tiles, 10, 10_000, 70_000)[0]                                                   # windows 0 and 7 of 8 are empty
    return tiles, [rev, mid]


CASES = {"short_runs": (case_short_runs, 8, 8, 10_000), "empty_runs": (case_empty_runs, 8, 8, 10_000),
         "multiples_of_16": (case_multiples_of_16, 8, 8, 10_000), "whole_tile_limit": (case_whole_tile_limit, 8, 8, 10_000),
         "batch": (case_batch, 4, 3, 977), "window_flags": (case_window_flags, 8, 8, 10_000)}


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


@pytest.mark.parametrize("name", sorted(CASES))
def test_tile_form_through_the_block_table_vs_oracle(er, orc, monkeypatch, name):
    from frlw_evd_amd import _lib
    make, K, n_win, win = CASES[name]
    tiles, recs = make()
    H, Wd = frame(tiles)
    B, span = len(recs), n_win * win
    assert 3 <= tiles <= 9 and sum(len(r) for r in recs) <= 150_000
    state0 = np.random.default_rng(17).uniform(-50, 0, (B, H, Wd, 2, K)).astype(np.float32)
    # the inputs are valid, by the oracle and numpy alone: every event inside the frame and the span (a refused call would fall back
    # to the general path and pass without the kernels under test), the oracle's own status 0 (it raises otherwise)
    want = []
    for j, r in enumerate(recs):
        ev = synth.from_dat8(r)
        assert len(r) == 0 or (ev["t"].min() >= 0 and ev["t"].max() < span and ev["x"].max() < Wd and ev["y"].max() < H), (name, j)
        view, st = orc.taf_stream_dat8(r, (H, Wd), (H, Wd), K, 0, win, n_win, state0[j])
        u8 = orc.quantize_u8(orc.leaky_transform(view.reshape(K, 2, H, Wd)))
        want.append((view, st, np.ascontiguousarray(u8[::-1])))
    dat = torch.from_numpy(np.ascontiguousarray(np.concatenate(recs)).view(np.uint8).reshape(-1, 8).copy()).cuda()
    offs = np.concatenate([[0], np.cumsum([len(r) for r in recs])])
    for wtab in (0, 1):
        monkeypatch.setattr(er, "TUNING", _lib.FrlwTuning(chunk_major=1, direct_bins=0, walk_window_table=wtab))
        st = torch.from_numpy(state0).cuda()
        u8, view = er.encode_taf_batch(dat, offs, (H, Wd), st, 0, win, n_win, K, want_view=True)
        for j in range(B):
            what = f"{name}, walk_window_table={wtab}, sequence {j}"
            assert_bitexact(st[j].cpu().numpy(), want[j][1], "state, " + what)
            assert_bitexact(view[j].cpu().numpy(), want[j][0], "view, " + what)
            assert_u8_budget(u8[j].cpu().numpy(), want[j][2], 1e-4, "uint8, " + what)
