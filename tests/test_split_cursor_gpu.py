"""kf_split_whole<true> books a tile's space in rec2[] with one returning add on the header's cursor and no longer waits for it in
front of its gather: the value stays in thread 0's register until the last gather address is out and reaches the other wavefronts
through the barrier behind the tickets.  What can go wrong is a start read before it is published, or a booking that is
skipped or made twice -- lists that overlap or leave holes in rec2[], which the CPU oracle sees as lost or duplicated events.  So:
bit for bit against the oracle (FIFO state, float32 view, uint8 volume, Event Volume), on streams BUILT chunk by chunk (chunks of
8192 events, csrc/taf_plan.h: `cm && k == 1`) so that the lists have the lengths at which the kernel takes another path:
  1. lists of 1, 63, 64 and 65 records (only wavefront 0 has a record: the other fifteen run ahead to the barrier), in one chunk
     and as short runs over three chunks next to an empty tile and a hot one (more than 8192 records with fewer than 256 pairs:
     booked here, placed by the segment kernels);
  2. lists of 8192, 8193, 16 385 and 28 673 records -- the staging-chunk edges and the first position of the fourth chunk -- as
     ORDINARY tiles, which takes 256 pairs or more: sequence 0 of a call of 64, the other 63 tiny (576 workgroups book at once);
  3. two sequences in one call;
  4. the mixed call captured into a HIP graph and replayed three times with different records;
  5. an Event Volume batch whose lists end on and just behind a staging-chunk edge.
frlw_tuning_t(chunk_major=1, direct_bins=0) sends every call through kf_split_whole<true>.  Frames of 6 to 9 tiles (a tile is
256 x 8 pixels on these frames), at most 80 000 events per case."""
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


def stream(counts, tiles, seed, t_lo, t_hi):
    """One sequence: counts[c][t] events of tile t in chunk c, shuffled inside the chunk; every chunk but the last holds CHUNK
    events.  Times ascend over the stream inside [t_lo, t_hi)."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1, tiles)
    assert (counts >= 0).all() and (counts[:-1].sum(axis=1) == CHUNK).all() and counts[-1].sum() <= CHUNK, counts.sum(axis=1)
    H, _ = frame(tiles)
    rng = np.random.default_rng(seed)
    tile = np.concatenate([rng.permutation(np.repeat(np.arange(tiles), row)) for row in counts]) if counts.sum() else np.zeros(0, np.int64)
    n = len(tile)
    rows = np.minimum(8, H - 8 * tile)
    ev = {"x": rng.integers(0, W, n), "y": 8 * tile + rng.integers(0, 1 << 30, n) % np.maximum(rows, 1), "p": rng.integers(0, 2, n),
          "t": np.sort(rng.integers(t_lo, t_hi, n))}
    return synth.to_dat8(ev), counts.sum(axis=0)


def filled(part, tiles, n_chunks, last):
    """part: {tile: per-chunk counts}; the last tile takes what is left of every chunk (`last` events in the last chunk)."""
    c = np.zeros((n_chunks, tiles), dtype=np.int64)
    for t, v in part.items():
        c[:, t] = v
    room = np.full(n_chunks, CHUNK)
    room[-1] = last
    c[:, tiles - 1] = room - c.sum(axis=1)
    return c


def spread(total, n_chunks, rng, evenness=2.0):
    """`total` events over n_chunks chunks, unevenly."""
    return rng.multinomial(total, rng.dirichlet(np.full(n_chunks, evenness)))


def tiny_counts():
    """6 tiles, one chunk of 200 events: lists of 1, 63, 64 and 65 records, an empty tile, 7 records in the last."""
    return 6, np.array([[1, 63, 64, 65, 0, 7]])


def mixed_counts():
    """7 tiles over three chunks: the tiny lists as short runs, an empty tile, an ordinary tile of 4000 records and a hot one."""
    tiles, nc = 7, 3
    c = filled({0: [1, 0, 0], 1: [20, 43, 0], 2: [0, 64, 0], 3: [30, 30, 5], 4: [0, 0, 0], 5: [1500, 1200, 1300]}, tiles, nc, last=6000)
    assert c[:, 6].sum() > CHUNK and c[:, 5].sum() == 4000  # 7 pairs: the last tile is over the one-segment limit
    return tiles, c


def case_tiny(seed=0):
    tiles, c = tiny_counts()
    return tiles, [stream(c, tiles, 11 + seed, 0, 80_000)[0]]


def case_mixed(seed=0):
    tiles, c = mixed_counts()
    return tiles, [stream(c, tiles, 21 + seed, 0, 80_000)[0]]


def case_chunk_edges():
    """64 sequences on 9 tiles = 576 pairs (whole-tile limit 32 768): sequence 0 holds lists of 8192, 8193, 16 385 and 28 673
    records over nine chunks, the other 63 sequences a few dozen events each (one of them none)."""
    tiles, nc, rng = 9, 9, np.random.default_rng(31)
    while True:  # (runs of uneven length; a draw that overfills a chunk is drawn again)
        c = filled({t: spread(n, nc, rng, 20.0) for t, n in enumerate((8192, 8193, 16385, 28673))}, tiles, nc, last=CHUNK)
        if (c >= 0).all():
            break
    rec0, per_tile = stream(c, tiles, 32, 0, 80_000)
    assert list(per_tile[:4]) == [8192, 8193, 16385, 28673]
    recs = [rec0]
    for j in range(1, 64):
        n_j = 0 if j == 5 else 9 + 3 * (j % 11)
        recs.append(stream(rng.multinomial(n_j, np.full(tiles, 1.0 / tiles))[None, :], tiles, 100 + j, 0, 80_000)[0])
    return tiles, recs


def case_two_sequences():
    tiles, rng = 7, np.random.default_rng(41)
    _, c0 = mixed_counts()
    c1 = filled({t: rng.integers(900, 1300, 2) for t in range(tiles - 1)}, tiles, 2, last=7000)  # every tile ordinary, two chunks
    c1[-1, :tiles - 1] = c1[-1, :tiles - 1] * 7000 // CHUNK
    c1[-1, tiles - 1] = 7000 - c1[-1, :tiles - 1].sum()
    assert (c1 >= 0).all() and c1.sum(axis=0).max() <= CHUNK
    return tiles, [stream(c0, tiles, 42, 0, 80_000)[0], stream(c1, tiles, 43, 0, 80_000)[0]]


CASES = {"tiny_lists": case_tiny, "mixed_empty_ordinary_hot": case_mixed, "chunk_edges_64_sequences": case_chunk_edges,
         "two_sequences": case_two_sequences}
K, N_WIN, WIN = 4, 8, 10_000


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


def to_dev(recs):
    return torch.from_numpy(np.ascontiguousarray(np.concatenate(recs)).view(np.uint8).reshape(-1, 8).copy()).cuda()


def oracle_taf(orc, rec, shape, state):
    view, st = orc.taf_stream_dat8(rec, shape, shape, K, 0, WIN, N_WIN, state)
    u8 = orc.quantize_u8(orc.leaky_transform(view.reshape(K, 2, *shape)))
    return view, st, np.ascontiguousarray(u8[::-1])


@pytest.mark.parametrize("name", sorted(CASES))
def test_lists_are_placed_once_and_whole(er, orc, monkeypatch, name):
    from frlw_evd_amd import _lib
    tiles, recs = CASES[name]()
    H, Wd = frame(tiles)
    B = len(recs)
    assert sum(len(r) for r in recs) <= 80_000
    state0 = np.random.default_rng(17).uniform(-50, 0, (B, H, Wd, 2, K)).astype(np.float32)
    # (valid by the oracle and numpy alone: a refused call would fall back to the general path and pass without the kernel under test)
    for r in recs:
        ev = synth.from_dat8(r)
        assert len(r) == 0 or (ev["t"].min() >= 0 and ev["t"].max() < N_WIN * WIN and ev["x"].max() < Wd and ev["y"].max() < H)
    want = [oracle_taf(orc, r, (H, Wd), state0[j]) for j, r in enumerate(recs)]
    offs = np.concatenate([[0], np.cumsum([len(r) for r in recs])])
    monkeypatch.setattr(er, "TUNING", _lib.FrlwTuning(chunk_major=1, direct_bins=0))
    st = torch.from_numpy(state0).cuda()
    u8, view = er.encode_taf_batch(to_dev(recs), offs, (H, Wd), st, 0, WIN, N_WIN, K, want_view=True)
    for j in range(B):
        what = f"{name}, sequence {j} ({len(recs[j])} events)"
        assert_bitexact(st[j].cpu().numpy(), want[j][1], "state, " + what)
        assert_bitexact(view[j].cpu().numpy(), want[j][0], "view, " + what)
        assert_u8_budget(u8[j].cpu().numpy(), want[j][2], 1e-4, "uint8, " + what)


def test_captured_encode_books_afresh_on_every_replay(er, orc, monkeypatch):
    """The cursor is a header word: a replay that found the previous replay's bookings in it would place its lists behind them.
    One frlw_taf_encode_batch captured into a HIP graph (tests/test_taf_fast_gpu.py: test_captured_encode_replays_against_the_oracle),
    replayed three times with different records of the same counts; the carried state and the uint8 volume after every replay."""
    from frlw_evd_amd import _lib
    monkeypatch.setattr(er, "TUNING", _lib.FrlwTuning(chunk_major=1, direct_bins=0))
    variants = [case_mixed(seed)[1] for seed in (0, 100, 200)]
    tiles = mixed_counts()[0]
    H, Wd = frame(tiles)
    offs = np.array([0, len(variants[0][0])])
    assert all(len(v[0]) == offs[1] for v in variants)
    side = torch.cuda.Stream()
    dat = to_dev(variants[0])
    state = torch.full((1, H, Wd, 2, K), -6000.0, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        warm = state.clone()  # (eager call on the capture stream first: workspace, self-test and threshold table exist before the capture)
        er.encode_taf_batch(dat, offs, (H, Wd), warm, 0, WIN, N_WIN, K)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            u8, _ = er.encode_taf_batch(dat, offs, (H, Wd), state, 0, WIN, N_WIN, K, check=False)
    want = np.full((H, Wd, 2, K), -6000, np.float32)
    for i, v in enumerate(variants):
        dat.copy_(to_dev(v))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        _view, want, ou8 = oracle_taf(orc, v[0], (H, Wd), want)
        assert_bitexact(state[0].cpu().numpy(), want, f"state after replay {i}")
        assert_u8_budget(u8[0].cpu().numpy(), ou8, 1e-4, f"uint8 after replay {i}")
    with torch.cuda.stream(side):
        er.raise_deferred()


def test_event_volume_batch_at_a_chunk_edge(er, orc, monkeypatch):
    """frlw_ev_encode_batch takes the same second level: 64 label windows on 9 tiles (576 pairs), the first with lists of 8192 and
    8193 records, the others a few dozen events each."""
    from frlw_evd_amd import _lib
    tiles, nc, bins, win, rng = 9, 3, 5, 50_000, np.random.default_rng(51)
    c = filled({0: [3000, 3000, 2192], 1: [3000, 3000, 2193]}, tiles, nc, last=5000)
    c[:, 2:tiles - 1] = c[:, [tiles - 1]] // (tiles - 2)  # the rest of every chunk over the other tiles
    c[:, tiles - 1] -= c[:, 2:tiles - 1].sum(axis=1)
    rec0, per_tile = stream(c, tiles, 52, 1, win + 1)
    assert list(per_tile[:2]) == [8192, 8193] and per_tile.max() == 8193
    recs = [rec0] + [stream(rng.multinomial(7 + j % 13, np.full(tiles, 1.0 / tiles))[None, :], tiles, 200 + j, 1, win + 1)[0] for j in range(1, 64)]
    H, Wd = frame(tiles)
    offs = np.concatenate([[0], np.cumsum([len(r) for r in recs])])
    monkeypatch.setattr(er, "TUNING", _lib.FrlwTuning(chunk_major=1, direct_bins=0))
    out, _ = er.encode_ev_batch(to_dev(recs), offs, (H, Wd), win, win, bins)
    for j, r in enumerate(recs):
        assert_bitexact(out[j].cpu().numpy(), orc.ev_stream_dat8(r, (H, Wd), (H, Wd), bins, win, win), f"sequence {j}")
