"""The consumers of the chunk-major partition take their bin through csrc/xcd_map.h (xcd_owned_index), not from the block index:
kf_split_whole<true>, kf_taf_walk<., true>, kf_ev_sub<., true>, kf_ev_fadd, kf_sae_sub (kf_taf_walk<., false>, kf_segcount_cm and
kf_split_place<true> keep the block index; they run in the same calls).  A relabelling that were not a bijection
would leave a bin unwritten, one that did not lead back to its own bin would write another bin's output -- so the check is the CPU
oracle, bit for bit, on the smallest calls where a relabelling can go wrong: grids below 8 and grids that are no multiple of 8
(frames of 1, 3, 7, 9 and 17 tiles x batches of 1, 3 and 5 sequences), every partition form frlw_tuning_t can force, tiles above
and below the segment limit (fewer than 256 pairs: 8192 records), a hot spot, an empty tile, a sparse sequence.
tests/test_xcd_map_cpu.py checks the arithmetic itself for every grid size."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from frlw_evd_amd import synth  # noqa: E402
from golden_util import LAMDAS, assert_bitexact, assert_u8_budget  # noqa: E402

pytestmark = pytest.mark.gpu

# frames of 1, 3, 7, 9 and 17 tiles (a tile is 2048 pixels: 256 x 8 on these frames), ragged at the right and lower edges
FRAMES = {1: (5, 250), 3: (21, 250), 7: (53, 250), 9: (69, 250), 17: (133, 250)}
EVENTS = [200_000, 20_000, 77_000, 120_000, 33_000]  # per sequence: tiles of these frames land on both sides of the segment limit
# (chunk_major, direct_bins, walk_window_table); -1 = the library's choice
TUNINGS = [(1, -1, -1), (1, 1, -1), (1, 0, 1), (1, 0, 0), (0, -1, -1), (0, 1, -1), (0, 0, -1)]


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
    return torch.from_numpy(np.ascontiguousarray(rec).view(np.uint8).reshape(-1, 8).copy()).cuda()


def host(t):
    return t.cpu().numpy()


def path_counts():
    """frlw_encoder_path_counts: [SAE two-launch, SAE general, ECI two-launch, ECI scan / general] launches of this process."""
    from frlw_evd_amd import _lib
    c = (C.c_uint64 * 4)()
    _lib.check(_lib.load().frlw_encoder_path_counts(c), "frlw_encoder_path_counts")
    return np.array(list(c), dtype=np.int64)


def _sequences(tiles, B, span, t_offset=0):
    """B sequences on the frame of `tiles` tiles: sequence 1 (the only one of a 17-tile single: a skewed tile next to ordinary
    ones) has a hot spot, sequence 2 (the only one of a 9-tile single) no event in tile 1 (rows 8 .. 15)."""
    H, W = FRAMES[tiles]
    recs = []
    for j in range(B):
        hot = j == 1 or (B == 1 and tiles == 17)
        ev = synth.synth_events(7000 + 31 * tiles + j, EVENTS[(j + tiles) % len(EVENTS)], W, H, span, hotspot=hot, t_offset=t_offset)
        if tiles >= 3 and (j == 2 or (B == 1 and tiles == 9)):
            keep = (ev["y"] < 8) | (ev["y"] >= 16)
            ev = {k: v[keep] for k, v in ev.items()}
        recs.append(synth.to_dat8(ev))
    return recs, np.concatenate([[0], np.cumsum([len(r) for r in recs])])


@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("tiles", sorted(FRAMES))
def test_taf_every_partition_form_vs_oracle(er, orc, monkeypatch, tiles, B):
    from frlw_evd_amd import _lib
    H, W = FRAMES[tiles]
    K, n_win, win = (4, 3, 977) if B == 3 else (8, 8, 10_000)  # kf_taf_walk<false, .> and <true, .>
    recs, offs = _sequences(tiles, B, n_win * win)
    dat = to_dev(np.concatenate(recs))
    state0 = np.random.default_rng(3 + tiles).uniform(-50, 0, (B, H, W, 2, K)).astype(np.float32)
    want = []  # one oracle run per sequence, shared by the tunings
    for j in range(B):
        view, st = orc.taf_stream_dat8(recs[j], (H, W), (H, W), K, 0, win, n_win, state0[j])
        u8 = orc.quantize_u8(orc.leaky_transform(view.reshape(K, 2, H, W)))
        want.append((view, st, np.ascontiguousarray(u8[::-1])))
    for cmaj, direct, wtab in TUNINGS:
        monkeypatch.setattr(er, "TUNING", _lib.FrlwTuning(chunk_major=cmaj, direct_bins=direct, walk_window_table=wtab))
        st = torch.from_numpy(state0).cuda()
        u8, view = er.encode_taf_batch(dat, offs, (H, W), st, 0, win, n_win, K, want_view=True)
        for j in range(B):
            what = f"chunk_major={cmaj} direct_bins={direct} walk_window_table={wtab}, sequence {j}"
            assert_bitexact(host(st[j]), want[j][1], "state, " + what)
            assert_bitexact(host(view[j]), want[j][0], "view, " + what)
            assert_u8_budget(host(u8[j]), want[j][2], 1e-4, "uint8, " + what)


@pytest.mark.parametrize("bins", [5, 8])
def test_event_volume_batch_every_consumer_vs_oracle(er, orc, monkeypatch, bins):
    """kf_ev_fadd (the default of a small direct-mode call), kf_ev_sub<., true> (ev_lds_float_atomics = 0), kf_split_whole<true> +
    kf_ev_sub<., false> (direct_bins = 0) and the histogram partition: 21 pairs, 336 bins, 84 workgroups of four bins."""
    from frlw_evd_amd import _lib
    tiles, B, win = 7, 3, 80_000
    H, W = FRAMES[tiles]
    recs, offs = _sequences(tiles, B, win, t_offset=1)
    dat = to_dev(np.concatenate(recs))
    want = [orc.ev_stream_dat8(r, (H, W), (H, W), bins, win, win) for r in recs]
    for tuning in (dict(), dict(direct_bins=1, ev_lds_float_atomics=0), dict(direct_bins=1, ev_lds_float_atomics=1),
                   dict(direct_bins=0), dict(chunk_major=0)):
        monkeypatch.setattr(er, "TUNING", _lib.FrlwTuning(**tuning))
        out, _ = er.encode_ev_batch(dat, offs, (H, W), win, win, bins)
        for j in range(B):
            assert_bitexact(host(out[j]), want[j], f"{tuning}, sequence {j}")


@pytest.mark.parametrize("tiles", [3, 7])
def test_sae_and_eci_two_launch_forms_vs_oracle(er, orc, tiles):
    """kf_sae_sub<false> and <true>: one workgroup per sub-tile bin, straight from the runs; the counters say that the two-launch
    form ran (the general path would give the same bits)."""
    H, W = FRAMES[tiles]
    ev = synth.synth_events(7100 + tiles, 60_000, W, H, 3_000_000, hotspot=True, t_offset=10_000_000)
    rec = synth.to_dat8(ev)
    dat = to_dev(rec)
    now = 13_000_000
    c0 = path_counts()
    out, _, mem = er.encode_sae_dat(dat, (H, W), LAMDAS, None, now, 1_000_000)
    c1 = path_counts()
    eci, _ = er.encode_eci_dat(dat, (H, W))
    c2 = path_counts()
    assert list(c1 - c0) == [1, 0, 0, 0] and list(c2 - c1) == [0, 0, 1, 0], (c0, c1, c2)
    want, wmem = orc.sae_stream_dat8(rec, (H, W), (H, W), LAMDAS, None, now, 1_000_000)
    assert_bitexact(host(mem), wmem, "sae memory")
    a = np.ascontiguousarray(host(out)).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(want).view(np.int32).astype(np.int64)
    assert np.abs(a - b).max() <= 2, f"sae out: {np.abs(a - b).max()} ulp (expf: 2 ulp, SURVEY.md 8c)"
    assert_bitexact(host(eci), orc.eci_stream_dat8(rec, (H, W), (H, W)), "eci")
