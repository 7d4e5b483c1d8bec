"""tests/conv_edge_cases.py on the CPU: every claim a case makes about its shape (rows of the last M-tile, valid columns of the
last column tile, a split count that does not divide the k-tiles, pixels in the last k-tile of the weight gradient) is
recomputed from the shape and checked against the tile size its form name implies.  An edit that makes a shape whole again,
or drops the only ragged case of a big tile, fails here without a GPU."""
import pytest

import conv_edge_cases as ec


def _launch_dims(case, table):
    """(M, N, K, (Ho, Wo)) of the GEMM the claims of a case speak about: the forward convolution, or for the data-gradient table
    the gradient's own launch (a parity class: M = B Ho Wo; else M = B H W), N = Cin, K = taps x Cout."""
    B, Cin, H, W, Cout, k, s = case.shape
    g = ec.geometry(case.shape)
    if table != "dgrad":
        return g.M, Cout, g.K, (g.Ho, g.Wo)
    if s == 2 and k == 3 and H % 2 == 0 and W % 2 == 0:
        return g.M, Cin, 4 * Cout, (g.Ho, g.Wo)
    return B * H * W, Cin, k * k * Cout, (H, W)


TABLES = [("fwd", ec.FWD), ("train", ec.TRAIN), ("dgrad", ec.DGRAD), ("wgrad", ec.WGRAD), ("dx_add", [ec.DX_ADD])]
CASES = [(t, c) for t, tab in TABLES for c in tab]


def test_names_are_unique_and_twins_exist():
    for t, tab in TABLES:
        names = [c.name for c in tab]
        assert len(set(names)) == len(names), t
    fwd = {c.name: c for c in ec.FWD}
    train = {c.name: c for c in ec.TRAIN}
    for a, b in ec.TWIN.items():
        assert train[a].shape == fwd[b].shape


def test_form_names_are_the_librarys():
    known = set(ec.TILE) | set(ec.WGRAD_TILE) | {"gathered", "parity", "wgrad_group_sum", "wgrad_scratch_limited"}
    for _, c in CASES:
        assert ec.forms_of(c) <= known, (c.name, ec.forms_of(c) - known)


@pytest.mark.parametrize("table,case", CASES, ids=[f"{t}: {c.name}" for t, c in CASES])
def test_claims(table, case):
    B, Cin, H, W, Cout, k, s = case.shape
    assert Cin % 4 == 0 and Cin >= 4 and Cout >= 1 and k % 2 == 1 and s in (1, 2)
    g = ec.geometry(case.shape)
    assert (g.M, g.K, g.R, g.Npad, g.nk) == (B * g.Ho * g.Wo, k * k * Cin, k * k * Cin, (Cout + 31) // 32 * 32, (k * k * Cin + 15) // 16)
    M, N, K, (oh, ow) = _launch_dims(case, table)
    forms = ec.forms_of(case)
    assert case.claims, "a case without an edge"
    for claim in case.claims:
        kind = claim[0]
        if kind == "last_m":
            _, form, r = claim
            assert form in forms, claim
            bm = ec.TILE[form][0]
            assert M % bm == r and 0 < r < bm, (claim, M, M % bm)
        elif kind == "valid_n":
            _, form, c = claim
            assert form in forms, claim
            if form in ec.WGRAD_TILE:
                bn, n = ec.WGRAD_TILE[form][1], Cout
            else:
                bn, n = ec.TILE[form][1], N
            assert n % bn == c and 0 < c < bn, (claim, n, n % bn)
        elif kind in ("splits", "dgrad_splits"):
            _, n, counters = claim
            nk = ec.cdiv(K, ec.BK)
            assert ec.conv_splits(M, ec.npad32(N), nk, counters) == n, (claim, ec.conv_splits(M, ec.npad32(N), nk, counters))
            assert n > 1 and (kind == "dgrad_splits" or nk % n != 0), (claim, nk)
        elif kind == "whole":
            assert ec.conv_splits(M, ec.npad32(N), ec.cdiv(K, ec.BK), claim[1]) == 1, claim
        elif kind == "pix16":
            assert g.M % 16 == claim[1] and claim[1] != 0, (claim, g.M % 16)
        elif kind == "short_image":
            assert g.Ho * g.Wo < 16
        elif kind == "wgrad_splits":
            form = next(f for f in forms if f in ec.WGRAD_TILE)
            assert ec.wgrad_splits(g.R, Cout, g.M, form) == claim[1] and claim[1] > 1, (claim, ec.wgrad_splits(g.R, Cout, g.M, form))
        elif kind == "last_r":
            _, form, r = claim
            assert form in forms, claim
            bm = ec.WGRAD_TILE[form][0]
            assert g.R % bm == r and 0 < r < bm, (claim, g.R % bm)
        elif kind == "odd":
            assert oh % 2 == 1 and ow % 2 == 1, (claim, oh, ow)
        else:
            raise AssertionError(f"unknown claim {claim}")


def test_44_k_tiles_split_only_with_counters():
    """The one shape whose split depends on the arrival counters alone: both sides are in the table."""
    sh = (2, 704, 8, 10, 256, 1, 1)
    g = ec.geometry(sh)
    assert g.nk == 44
    assert ec.conv_splits(g.M, g.Npad, g.nk, True) == 5 and ec.conv_splits(g.M, g.Npad, g.nk, False) == 1
    assert any(c.shape == sh and ("whole", False) in c.claims for c in ec.FWD)
    assert any(c.shape == sh and ("splits", 5, True) in c.claims for c in ec.TRAIN)


def _has(form, kind, tables):
    return [c for t in tables for c in t if form in ec.forms_of(c) and any(cl[0] == kind and (len(cl) < 2 or cl[1] == form) for cl in c.claims)]


@pytest.mark.parametrize("form", ec.BIG_TILES)
def test_every_big_forward_tile_is_ragged_somewhere(form):
    tables = (ec.FWD, ec.TRAIN)
    assert _has(form, "last_m", tables), f"{form}: no case with a ragged last M-tile"
    assert _has(form, "valid_n", tables), f"{form}: no case with a ragged last column tile"
    odd = [c for t in tables for c in t if form in ec.forms_of(c) and ("odd",) in c.claims]
    assert odd, f"{form}: no case with odd Ho and Wo"
    # through both entries: the plain forward and the train forward with its statistics slabs
    assert any(form in ec.forms_of(c) for c in ec.FWD) and any(form in ec.forms_of(c) for c in ec.TRAIN)


def test_the_wide_wgrad_tile_is_ragged_somewhere():
    form = "wgrad_128x128"
    assert _has(form, "valid_n", (ec.WGRAD,)) and _has(form, "last_r", (ec.WGRAD,))
    ragged_pixels = [c for c in ec.WGRAD if form in c.forms and any(cl[0] == "pix16" for cl in c.claims)]
    assert ragged_pixels and any(("odd",) in c.claims for c in ragged_pixels)


def test_every_forward_and_wgrad_tile_has_a_ragged_m_case():
    for form in ("128x32", "128x128_2x2", "128x128_4x1", "64x128", "64x64", "split_vec", "split_inkernel", "split_inkernel_stats"):
        assert _has(form, "last_m", (ec.FWD, ec.TRAIN, ec.DGRAD, [ec.DX_ADD])), form
    for form in ec.WGRAD_TILE:
        assert any(form in ec.forms_of(c) and any(cl[0] == "pix16" for cl in c.claims) for c in ec.WGRAD + ec.TRAIN), form


def test_dx_add_rows_are_wider_than_cin():
    Cin = ec.DX_ADD.shape[1]
    assert ec.DX_ADD_PITCH > Cin and ec.DX_ADD_PITCH % 4 == 0 and ec.DX_ADD_OFFSET % 4 == 0
    assert ec.DX_ADD_OFFSET + Cin <= ec.DX_ADD_PITCH and ec.DX_ADD.shape[-1] == 1
