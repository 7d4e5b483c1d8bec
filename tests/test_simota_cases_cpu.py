"""What tests/simota_cases.py claims, checked with the reference's per-image procedure on the CPU (``losses.get_assignments`` /
``dynamic_k_matching``): every case reaches the regime it exists for, and no decision of the reference is a near-tie, so
that tests/test_simota_regimes_gpu.py can demand the kernels' assignment to be exactly the reference's.  Without this
file an edit to the generator could drift back to k = 1 everywhere and the GPU tests would go on passing.

Decision margins: the kernels and the reference compute the class cost in float32 with different exp / log / sqrt
routines (a few 1e-7 relative); everything else of a cost and every IoU is float64 on both sides.  A relative gap of 1e-5
between the costs that decide, and a distance of 1e-5 between a top-10 IoU sum and the next integer, are about a hundred
times that.  A seed that falls short is replaced; the bound stays.
"""
import pytest

torch = pytest.importorskip("torch")

import simota_cases as sc  # noqa: E402

MARGIN = 1e-5


def _images(name):
    case, res = sc.cached(name)
    return case, [a for a in res if a.n_cand > 0]


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_case_shapes_and_types(name):
    case, res = sc.cached(name)
    spec = sc.CASES[name]
    B = len(spec["boxes"])
    assert [tuple(t.shape) for t in case.levels] == [(B, 5 + case.nc, h, w) for h, w in spec["shapes"]]
    assert all(t.dtype == torch.float32 and bool(torch.isfinite(t).all()) for t in case.levels)
    assert case.labels.shape == (B, 80, 5) and case.labels.dtype == torch.float64
    assert [a.n for a in res] == list(spec["boxes"])  # every box counts as a label (its five fields sum to > 0)
    assert 1 <= len(case.levels) <= 4 and len(case.strides) == len(case.levels)
    again = sc.make(name)
    assert all(torch.equal(a, b) for a, b in zip(again.levels, case.levels)) and torch.equal(again.labels, case.labels)


def test_anchor_counts():
    anchors = {n: sum(h * w for h, w in s["shapes"]) for n, s in sc.CASES.items()}
    assert anchors["crowded-1mpx"] == 6720 and anchors["near-limit"] == 9576 and anchors["exact-limit"] == 9600
    assert anchors["small-crowded"] == 1680
    assert all(anchors[n] <= 3072 for n in ("levels-1", "levels-2", "levels-4"))  # within the default dynamic LDS
    assert [len(sc.CASES[n]["shapes"]) for n in ("levels-1", "levels-2", "levels-4")] == [1, 2, 4]
    assert sc.CASES["nc-1"]["nc"] == 1 and sc.CASES["nc-20"]["nc"] == 20
    from frlw_evd_amd.yolox import losses
    assert anchors["exact-limit"] == losses.NATIVE_MAX_ANCHORS


@pytest.mark.parametrize("name", sc.CROWDED)
def test_crowded_cases_spread_k_and_contest_anchors(name):
    case, imgs = _images(name)
    ks = torch.cat([a.ks for a in imgs])
    contested = sum(sc.decision_margins(a)[2] for a in imgs)
    print(f"{name}: k histogram {sorted((int(k), int((ks == k).sum())) for k in ks.unique())}, {contested} contested anchors")
    assert int(ks.max()) >= 8 and int(ks.min()) <= 2
    assert contested >= 5
    assert imgs[0].n == 80 and imgs[0].cost.shape[0] == 80  # the full label tensor


@pytest.mark.parametrize("name", ["near-limit", "levels-1", "levels-2", "levels-4", "nc-1", "nc-20", "saturated"])
def test_other_cases_are_not_the_k_equals_1_corner(name):
    case, imgs = _images(name)
    ks = torch.cat([a.ks for a in imgs])
    assert int(ks.max()) >= 8 and int(ks.min()) <= 2
    assert sum(sc.decision_margins(a)[2] for a in imgs) >= 1


def test_few_candidates():
    case, res = sc.cached("few-candidates")
    assert 1 <= res[0].n_cand <= 9  # image 0: fewer candidates than the ten of the top-10 IoU sum
    assert int(res[0].ks[0]) == 2 and res[0].num_fg == 2  # and more than one round of the k cheapest among them
    # image 1: the second box has no candidate of its own -- not one cost of its row is free of the 1e5 penalty, and
    # every IoU of the row is 0 -- next to a box that has
    a = res[1]
    assert a.n == 2 and float(a.cost[1].min()) >= 100000.0 and float(a.ious[1].max()) == 0.0
    assert float(a.cost[0].min()) < 100.0 and int(a.ks[0]) > 1 and int(a.ks[1]) == 1
    assert res[2].n == 12 and res[2].n_cand > 100


def test_no_candidate():
    case, res = sc.cached("no-candidate")
    b = case.meta["empty_image"]
    assert res[b].n == 1 and res[b].n_cand == 0  # one label, not one candidate anchor
    assert res[1 - b].n_cand > 100 and res[1 - b].num_fg > 0
    from frlw_evd_amd.yolox import losses
    with pytest.raises(RuntimeError):  # the reference's procedure has no answer here (topk with k = 1 on an empty row)
        losses.yolox_losses([t[b:b + 1] for t in case.levels], case.strides, case.labels[b:b + 1], case.nc, case.radius)


def test_saturated_reaches_the_clamp():
    case, imgs = _images("saturated")
    on_clamp = sum(int((a.bce == 100.0).sum()) for a in imgs)
    print(f"saturated: {on_clamp} elements of the class cost on the -100 clamp")
    assert on_clamp >= 1
    assert max(float(t[:, 4:].abs().max()) for t in case.levels) == 30.0
    # costs that the clamp decided, on anchors inside their box's centre square (no 1e5 penalty)
    costs = torch.cat([a.cost.flatten() for a in imgs])
    assert bool(((costs >= 100.0) & (costs < 100000.0)).any())


def test_tied_corners():
    case, res = sc.cached("tied-corners")
    a = res[0]
    outputs = sc.decode(case.levels, case.strides)[0]
    for g, (lvl, y, x) in enumerate(case.meta["tied"]):
        i = sc.anchor_index(case, lvl, y, x)
        assert bool(a.fg[i]), "the crafted anchor is foreground"
        j = int(a.fg[:i].sum())  # its position among the foreground anchors
        assert int(a.matched_gt[j]) == g
        pred, box = outputs[0, i, :4].double(), case.labels[0, g, 1:5]
        tl = torch.stack([pred[:2] - pred[2:] / 2, box[:2] - box[2:] / 2])
        br = torch.stack([pred[:2] + pred[2:] / 2, box[:2] + box[2:] / 2])
        ties = int((tl[0] == tl[1]).sum()) + int((br[0] == br[1]).sum())
        assert ties == (4, 2, 2)[g]
        if g == 0:
            assert float(a.matched_iou[j]) == 1.0  # exactly
        else:
            assert 0.7 < float(a.matched_iou[j]) < 0.8
    assert a.num_fg == 3


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_decision_margins(name):
    case, imgs = _images(name)
    assert imgs
    for a in imgs:
        gap_k, gap_contested, n_contested, dist_int = sc.decision_margins(a)
        print(f"{name}: k-th vs (k+1)-th cost {gap_k:.2e}, contested ({n_contested}) {gap_contested:.2e}, "
              f"IoU sum to integer {dist_int:.2e}")
        assert gap_k >= MARGIN
        assert gap_contested >= MARGIN
        assert dist_int >= MARGIN
