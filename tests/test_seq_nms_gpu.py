"""Seq-NMS on the GPU (frlw_seq_nms, csrc/seq_nms.hip) against the plain restatement (tests/seqnms_restated.py, itself held to the
reference's answers in tests/test_seq_nms_cpu.py): scores equal bit for bit (``==`` on float64), sequence ids and suppression
flags identical.  The kernel recomputes only the frames a selection touched; the restatement recomputes everything."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import seqnms_data  # noqa: E402
import seqnms_restated  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = seqnms_data.cases()
ALL = dict(CASES, **seqnms_data.more_seeds(20))
_WANT = {}


def want(name, metric, isolated, **kw):
    """The restatement's answer, computed once per (case, options)."""
    key = (name, metric, isolated, tuple(sorted(kw.items())))
    if key not in _WANT:
        _WANT[key] = seqnms_restated.seq_nms(ALL[name], metric=metric, isolated=isolated, **kw)
    return _WANT[key]


def same(got, res):
    assert len(got) == len(res)
    for f, ((gs, gq, gf), (ws, wq, wf)) in enumerate(zip(got, res)):
        assert gs.dtype == np.float64 and gq.dtype == np.int32 and gf.dtype == bool
        assert (gs == ws).all(), f"scores of frame {f}: {gs} != {ws}"
        assert (gq == wq).all(), f"sequence ids of frame {f}: {gq} != {wq}"
        assert (gf == wf).all(), f"flags of frame {f}: {gf} != {wf}"


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.mark.parametrize("isolated", ["stop", "skip"])
@pytest.mark.parametrize("metric", ["avg", "max"])
def test_kernel_equals_the_restatement(metric, isolated):
    """Every golden case and 20 further seeds, all in ONE call (33 recordings), and the first three once more alone."""
    need_gpu()
    from frlw_evd_amd import seq_nms as sn
    names = list(ALL)
    got, status = sn.seq_nms([ALL[n] for n in names], metric=metric, isolated=isolated, return_status=True)
    assert (status == 0).all()
    n_seq = 0
    for name, g in zip(names, got):
        res, selections, _ = want(name, metric, isolated)
        same(g, res)
        n_seq += len(selections)
    assert n_seq > 100
    for name in ("empty_frames", "wide64", "long130"):
        same(sn.seq_nms(CASES[name], metric=metric, isolated=isolated), want(name, metric, isolated)[0])


def test_three_recordings_batched_equal_the_three_alone():
    need_gpu()
    from frlw_evd_amd import seq_nms as sn
    names = ["random_a", "long130", "random_b"]
    batched = sn.seq_nms([CASES[n] for n in names], isolated="skip")
    for name, b in zip(names, batched):
        alone = sn.seq_nms(CASES[name], isolated="skip")
        assert len(alone) == len(b)
        for (a0, a1, a2), (b0, b1, b2) in zip(alone, b):
            assert a0.tobytes() == b0.tobytes() and a1.tobytes() == b1.tobytes() and a2.tobytes() == b2.tobytes()
    assert max(int(q.max()) for _, q, _ in batched[0] if len(q)) >= 3


def test_max_sequences_truncates():
    """``max_sequences = 1``: exactly the first sequence, and the status word says so; a bound nobody reaches leaves it clear."""
    need_gpu()
    from frlw_evd_amd import _lib, seq_nms as sn
    got, status = sn.seq_nms(CASES["random_a"], max_sequences=1, return_status=True)
    res, selections, truncated = want("random_a", "avg", "stop", max_sequences=1)
    assert truncated and len(selections) == 1 and status.tolist() == [_lib.SEQ_NMS_TRUNCATED]
    same(got, res)
    assert sorted(set(np.concatenate([q for _, q, _ in got]).tolist())) == [0, 1]
    start, path, _ = want("random_a", "avg", "stop")[1][0]
    assert all(got[start + k][1][i] == 1 for k, i in enumerate(path))
    _, status = sn.seq_nms(CASES["random_a"], max_sequences=1000, return_status=True)
    assert status.tolist() == [0]


def test_short_workspace_is_refused():
    need_gpu()
    from frlw_evd_amd import _lib, seq_nms as sn
    packed = sn.pack([CASES["random_b"]])
    need = _lib.load().frlw_seq_nms_workspace_bytes(len(packed[1]), len(packed[3]) - 1, 1)
    with pytest.raises(RuntimeError, match="workspace too small"):
        sn.run_packed(*packed, 0.5, 0.3, 0, 0, 65536, workspace_bytes=need - 1)
    out = sn.run_packed(*packed, 0.5, 0.3, 0, 0, 65536, workspace_bytes=need)
    want_scores = np.concatenate([s for s, _, _ in want("random_b", "avg", "stop")[0]])
    assert (out[0] == want_scores).all()


def test_thresholds_cross_as_doubles():
    """IoU exactly 3/10 suppresses at nms_thr = 0.3 and exactly 1/2 links at link_thr = 0.5; one ulp above, neither does."""
    need_gpu()
    from frlw_evd_amd import seq_nms as sn
    got = sn.seq_nms(CASES["exact_three_tenths"])
    assert got[1][2].tolist() == [False, True] and got[2][2].tolist() == [False, True]
    up = float(np.nextafter(0.3, 1.0))
    got = sn.seq_nms(CASES["exact_three_tenths"], nms_thr=up, isolated="skip")
    assert not got[1][2].any() and got[1][1].tolist() == [1, 2]
    same(got, seqnms_restated.seq_nms(CASES["exact_three_tenths"], nms_thr=up, isolated="skip")[0])
    assert [q.tolist() for _, q, _ in sn.seq_nms(CASES["exact_half"])] == [[1, 0], [0, 1], [1]]
    got = sn.seq_nms(CASES["exact_half"], link_thr=float(np.nextafter(0.5, 1.0)))
    assert all(not q.any() for _, q, _ in got)


def test_rescore_records_on_the_device():
    """The structured-array route through the real call equals the restatement applied to the same rows."""
    need_gpu()
    from frlw_evd_amd import seq_nms as sn
    from frlw_evd_amd.stream import to_bbox_records
    case = CASES["random_b"]
    stamps = [1_000_000 + 50_000 * k for k in range(len(case))]
    rows = []
    for ts, fr in zip(stamps, case):
        r = np.zeros((len(fr), 8), np.float32)
        r[:, 0], r[:, 1], r[:, 2], r[:, 3], r[:, 4] = ts, fr[:, 0], fr[:, 1], fr[:, 2] - fr[:, 0], fr[:, 3] - fr[:, 1]
        r[:, 5], r[:, 6] = fr[:, 5], fr[:, 4]
        rows.append(r)
    frames, picks = sn.rows_to_frames(rows)
    res, selections, _ = seqnms_restated.seq_nms(frames, isolated="skip")
    want_rec = to_bbox_records(sn.apply_to_rows(rows, picks, res), stamps)
    got, n = sn.rescore_records(to_bbox_records(rows, stamps), stamps=stamps, isolated="skip")
    assert n == len(selections) >= 2 and got.tobytes() == want_rec.tobytes()
    kept, _ = sn.rescore_records(to_bbox_records(rows, stamps), stamps=stamps, isolated="skip", drop_suppressed=True)
    n_sup = int(sum(s.sum() for _, _, s in res))
    assert n_sup > 0 and len(kept) == len(got) - n_sup
