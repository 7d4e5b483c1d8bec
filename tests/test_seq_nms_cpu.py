"""Seq-NMS without a GPU: the restatement the kernels are held to (tests/seqnms_restated.py) against the answers of the reference
(tests/golden/seqnms.npz, made by tests/golden/make_golden_seqnms.py), and the host side of the product: the workspace query, the
wrapper's argument checks, the grouping of a detection file and the new flags of detect_recording.py."""
import os
import sys

import numpy as np
import pytest

import seqnms_data
import seqnms_restated

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = seqnms_data.cases()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "seqnms.npz"))


@pytest.mark.parametrize("metric", ["avg", "max"])
@pytest.mark.parametrize("name", list(CASES))
def test_restatement_equals_the_reference(golden, name, metric):
    """``stop`` mode: the same sequences in the same order with the same sums, and the final scores equal bit for bit."""
    res, selections, truncated = seqnms_restated.seq_nms(CASES[name], metric=metric, isolated="stop")
    sel = golden[f"{name}_{metric}_sel"]
    assert not truncated and len(selections) == len(sel)
    for (start, path, total), row, want in zip(selections, sel, golden[f"{name}_{metric}_sum"]):
        assert start == row[0] and len(path) == row[1] and path == row[2:2 + row[1]].tolist()
        assert total == want
    scores = np.concatenate([s for s, _, _ in res]) if res else np.zeros(0)
    want = golden[f"{name}_{metric}_scores"]
    assert scores.shape == want.shape and (scores == want).all()


def test_cases_hold_what_they_are_named_for(golden):
    """The goldens exercise the rules: sequences exist, a path crosses frame 64, ties are broken by index and frame, the exact
    thresholds link and suppress, ``skip`` goes on where ``stop`` ends."""
    n_sel = {name: len(golden[f"{name}_avg_sel"]) for name in CASES}
    assert n_sel["one_frame"] == 0 and n_sel["two_frames"] == 1 and n_sel["single_box_frames"] == 1
    assert n_sel["random_a"] >= 3 and n_sel["random_b"] >= 2 and n_sel["empty_frames"] >= 2
    assert max(len(f) for f in CASES["wide64"]) == 64 and [63] in [r[2:2 + r[1]].tolist()[1:2] for r in golden["wide64_avg_sel"]]
    assert any(r[0] < 64 <= r[0] + r[1] - 1 for r in golden["long130_avg_sel"]) and any(r[0] >= 64 for r in golden["long130_avg_sel"])
    assert golden["exact_half_avg_sel"].tolist() == [[0, 3, 0, 1, 0]]                  # IoU 0.5 links twice; 1/3 does not
    assert golden["exact_three_tenths_avg_sel"].tolist() == [[0, 3, 0, 0, 0]]          # B (IoU 3/10) is suppressed: no second sequence
    assert golden["ties_avg_sel"].tolist() == [[0, 2, 0, 0], [0, 2, 1, 2], [1, 2, 3, 0]]
    assert golden["cross_class_avg_sel"].tolist() == [[0, 3, 0, 0, 0]]
    res, _, _ = seqnms_restated.seq_nms(CASES["cross_class"])
    assert res[1][2].tolist() == [False, True] and res[2][2].tolist() == [False, True]
    stop = seqnms_restated.seq_nms(CASES["stop_vs_skip"], isolated="stop")[1]
    skip = seqnms_restated.seq_nms(CASES["stop_vs_skip"], isolated="skip")[1]
    assert len(stop) == 1 and len(skip) == 2 and skip[0] == stop[0] and len(skip[1][1]) == 4
    assert all(len(f) <= 12 for n, c in CASES.items() if n != "wide64" for f in c)
    assert all(len(c) <= 40 for n, c in CASES.items() if n != "long130")


def test_restatement_bounds_and_ids():
    res, selections, truncated = seqnms_restated.seq_nms(CASES["random_a"], isolated="skip", max_sequences=2)
    assert truncated and len(selections) == 2
    ids = np.concatenate([q for _, q, _ in res])
    assert sorted(set(ids.tolist())) == [0, 1, 2]
    for k, (start, path, _) in enumerate(selections, 1):
        assert all(res[start + j][1][i] == k for j, i in enumerate(path)) and int((ids == k).sum()) == len(path)


def test_workspace_query_is_host_only():
    from frlw_evd_amd import _lib
    lib = _lib.load()
    small, big = lib.frlw_seq_nms_workspace_bytes(100, 20, 1), lib.frlw_seq_nms_workspace_bytes(64 * 4096 * 64, 64 * 4096, 64)
    assert 25 * 100 <= small < 8192 and big >= 25 * 64 * 4096 * 64
    assert lib.frlw_seq_nms_workspace_bytes(0, 0, 1) > 0
    assert lib.frlw_seq_nms_workspace_bytes(10, 5, 65) == 0          # more than 64 recordings
    assert lib.frlw_seq_nms_workspace_bytes(10, 4097, 1) == 0        # more than 4096 frames in one recording
    assert lib.frlw_seq_nms_workspace_bytes(65, 1, 1) == 0           # more than 64 boxes in the one frame
    assert lib.frlw_seq_nms_workspace_bytes(-1, 1, 1) == 0 and lib.frlw_seq_nms_workspace_bytes(1, 1, 0) == 0


def test_entry_point_checks_arguments_on_the_host():
    """Null pointers and offsets over the limits are answered before anything is enqueued: no GPU needed."""
    import ctypes as C
    from frlw_evd_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(0x1000)   # never dereferenced

    def call(fs, vs, boxes=p, status=p, ws=p, ws_bytes=1 << 20, metric=0, isolated=0, max_sequences=1):
        fs, vs = (C.c_int32 * len(fs))(*fs), (C.c_int32 * len(vs))(*vs)
        return lib.frlw_seq_nms(boxes, p, p, fs, vs, len(vs) - 1, 0.5, 0.3, metric, isolated, max_sequences, p, p, p, status, ws, ws_bytes, None)
    assert call([0, 65], [0, 1]) == _lib.FRLW_ERR_ARG                       # 65 boxes in a frame
    assert call([0] * 4098, [0, 4097]) == _lib.FRLW_ERR_ARG                 # 4097 frames in a recording
    assert call([0, 3, 2], [0, 2]) == _lib.FRLW_ERR_ARG                     # offsets running backwards
    assert call([0, 3], [0, 1], boxes=None) == _lib.FRLW_ERR_ARG
    assert call([0, 3], [0, 1], status=None) == _lib.FRLW_ERR_ARG
    assert call([0, 3], [0, 1], metric=2) == _lib.FRLW_ERR_ARG and call([0, 3], [0, 1], isolated=2) == _lib.FRLW_ERR_ARG
    assert call([0, 3], [0, 1], max_sequences=0) == _lib.FRLW_ERR_ARG
    assert call([0, 3], [0, 1], ws=None) == _lib.FRLW_ERR_WORKSPACE
    assert call([0, 3], [0, 1], ws_bytes=lib.frlw_seq_nms_workspace_bytes(3, 1, 1) - 1) == _lib.FRLW_ERR_WORKSPACE


def test_wrapper_argument_errors():
    from frlw_evd_amd import seq_nms as sn
    box = [0.0, 0.0, 10.0, 10.0, 0.5, 0.0]
    with pytest.raises(ValueError, match="at most 64"):
        sn.seq_nms([np.tile(box, (65, 1))])
    with pytest.raises(ValueError, match="at most 4096"):
        sn.seq_nms([np.array([box])] * 4097)
    bad = np.array([box])
    bad[0, 4] = np.nan
    with pytest.raises(ValueError, match="finite"):
        sn.seq_nms([bad])
    bad[0, 4] = -0.1
    with pytest.raises(ValueError, match=">= 0"):
        sn.seq_nms([bad])
    with pytest.raises(ValueError):
        sn.seq_nms([np.array([box])], metric="median")
    with pytest.raises(ValueError):
        sn.seq_nms([np.array([box])], isolated="keep")
    with pytest.raises(ValueError):
        sn.seq_nms([np.array([box])], max_sequences=0)
    with pytest.raises(ValueError):
        sn.seq_nms([[np.array([box])]] * 65)
    assert sn.seq_nms([]) == [] and sn.seq_nms([np.zeros((0, 6))] * 3)[2][1].shape == (0,)   # nothing to do: no device call


def _restated_rows(rows, **options):
    """What ``rescore_frames`` must return, by the restatement (no drop)."""
    from frlw_evd_amd import seq_nms as sn
    frames, picks = sn.rows_to_frames(rows)
    res, selections, _ = seqnms_restated.seq_nms(frames, **options)
    return sn.apply_to_rows(rows, picks, res), len(selections)


def test_rows_conversion_and_the_64_box_cut():
    """xywh -> corners in the rows' float32; of a frame with more than 64 boxes the 64 most confident are sent (ties: the lower
    index) and the rest pass through with track 0."""
    from frlw_evd_amd import seq_nms as sn
    rng = np.random.default_rng(5)
    r = np.zeros((70, 8), np.float32)
    r[:, 1:5] = rng.uniform(1, 50, (70, 4))
    r[:, 6] = np.repeat(np.linspace(0.9, 0.1, 35), 2)          # pairs of equal confidence: rows 64, 65 tie
    r[:, 7] = 9
    frames, picks = sn.rows_to_frames([r, r[:3]])
    assert picks[0].tolist() == list(range(64)) and picks[1].tolist() == [0, 1, 2]
    assert (frames[0][:, 2] == (r[:64, 1] + r[:64, 3]).astype(np.float64)).all() and (frames[1][:, 4] == r[:3, 6]).all()
    res = [(f[:, 4] * 0.5, np.arange(len(f)) % 3, np.arange(len(f)) % 2 == 1) for f in frames]
    out = sn.apply_to_rows([r, r[:3]], picks, res, seq_offset=10)
    assert (out[0][64:, 6] == r[64:, 6]).all() and (out[0][64:, 7] == 0).all()
    assert (out[0][:64, 6] == (r[:64, 6].astype(np.float64) * 0.5).astype(np.float32)).all()
    assert out[0][:6, 7].tolist() == [0, 11, 12, 0, 11, 12]
    dropped = sn.apply_to_rows([r, r[:3]], picks, res, drop_suppressed=True)
    assert len(dropped[0]) == 32 + 6 and len(dropped[1]) == 2


def test_rescore_records_grouping_and_round_trip(monkeypatch):
    """``rescore_records`` groups a structured array by ``t`` (any record order), hands the frames over in time order and writes the
    answers back to the records they came from; with ``stamps`` an empty frame of the grid breaks the links.  The device call is
    replaced by the restatement here; tests/test_seq_nms_gpu.py runs the real one."""
    from frlw_evd_amd import seq_nms as sn
    from frlw_evd_amd.stream import BBOX_DTYPE, to_bbox_records

    def by_restatement(frames, link_thr=0.5, nms_thr=0.3, metric="avg", isolated="stop", max_sequences=65536):
        return seqnms_restated.seq_nms(frames, link_thr, nms_thr, metric, isolated, max_sequences)[0]
    monkeypatch.setattr(sn, "seq_nms", by_restatement)
    case = CASES["stop_vs_skip"]
    stamps = [1_000_000 + 50_000 * k for k in range(len(case))]
    rows = []
    for ts, fr in zip(stamps, case):
        r = np.zeros((len(fr), 8), np.float32)
        r[:, 0], r[:, 1], r[:, 2], r[:, 3], r[:, 4] = ts, fr[:, 0], fr[:, 1], fr[:, 2] - fr[:, 0], fr[:, 3] - fr[:, 1]
        r[:, 5], r[:, 6] = fr[:, 5], fr[:, 4]
        rows.append(r)
    rec = to_bbox_records(rows, stamps)
    assert rec.dtype == BBOX_DTYPE
    want_rows, want_n = _restated_rows(rows, isolated="skip")
    want = to_bbox_records(want_rows, stamps)
    got, n = sn.rescore_records(rec, stamps=stamps, isolated="skip")
    assert n == want_n == 2 and got.tobytes() == want.tobytes() and set(got["track_id"].tolist()) == {0, 1, 2}
    perm = np.random.default_rng(3).permutation(len(rec))
    shuffled, _ = sn.rescore_records(rec[perm], stamps=stamps, isolated="skip")
    assert shuffled.tobytes() == want[perm].tobytes()
    # frame 0 of the case is empty: without the grid the file's own timestamps are the frames, and the answer is the same here
    assert sn.rescore_records(rec, isolated="skip")[0].tobytes() == want.tobytes()
    kept, _ = sn.rescore_records(rec, stamps=stamps, isolated="skip", drop_suppressed=True)
    assert len(kept) == len(rec)      # nothing overlaps in this case
    with pytest.raises(ValueError):
        sn.rescore_records(rec, stamps=stamps[1:5])


def test_detect_recording_flags():
    sys.path.insert(0, ROOT)
    import detect_recording
    p = detect_recording.build_parser()
    a = p.parse_args(["--dat", "x_td.dat", "--out", "y"])
    assert a.seq_nms == "off" and a.seq_nms_metric == "avg" and a.seq_nms_drop is False
    assert detect_recording.seq_nms_options(a) is None
    a = p.parse_args(["--dat", "x_td.dat", "--out", "y", "--seq_nms", "skip", "--seq_nms_metric", "max", "--seq_nms_drop"])
    assert detect_recording.seq_nms_options(a) == {"isolated": "skip", "metric": "max", "drop_suppressed": True}
    with pytest.raises(SystemExit):
        p.parse_args(["--dat", "x_td.dat", "--out", "y", "--seq_nms", "on"])
