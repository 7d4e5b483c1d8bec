"""frlw_taf_batch_workspace_bytes against values recorded BEFORE the workspace layout became one function shared by the size
query and the call (tests/golden/workspace_bytes.json, made by tests/golden/make_golden_workspace.py from that earlier build):
the query is host arithmetic, the library loads without a GPU."""
import json
import os

from frlw_evd_amd import _lib


def test_batch_workspace_query_equals_the_recorded_values(golden_dir):
    g = json.load(open(os.path.join(golden_dir, "workspace_bytes.json")))
    lib = _lib.load()
    grid = [(n, s, h, w, win) for n in g["events"] for s in g["sequences"] for h, w in g["frames_h_w"] for win in g["windows_us"]]
    assert len(grid) == len(g["bytes"]) == 640
    assert any(b == 0 for b in g["bytes"]) and any(b > 0 for b in g["bytes"])  # refused shapes and planned ones
    bad = [(a, int(lib.frlw_taf_batch_workspace_bytes(*a)), want) for a, want in zip(grid, g["bytes"])
           if int(lib.frlw_taf_batch_workspace_bytes(*a)) != want]
    assert not bad, f"{len(bad)} of {len(grid)} differ, first: {bad[:3]}"
    for a, want in list(zip(grid, g["bytes"]))[::37]:
        assert int(lib.frlw_ev_batch_workspace_bytes(*a)) == want


def test_encoder_workspace_query_equals_the_recorded_values(golden_dir):
    """frlw_encoder_workspace_bytes = the larger of the general path's plan (csrc/enc_plan.h make_plan) and the two-launch form's,
    pinned over 8 event counts x 12 frames (tests/golden/encoder_workspace_bytes.json): a change of the planner or of the layout
    that moves a caller's allocation shows here."""
    g = json.load(open(os.path.join(golden_dir, "encoder_workspace_bytes.json")))
    lib = _lib.load()
    grid = [(n, h, w) for n in g["events"] for h, w in g["frames_h_w"]]
    assert len(grid) == len(g["bytes"]) == 96
    assert sum(1 for b in g["bytes"] if b == 0) == 16  # 4000 x 4000 and the stack of 64 GEN1 frames: too many tiles at width 8
    bad = [(a, int(lib.frlw_encoder_workspace_bytes(*a)), want) for a, want in zip(grid, g["bytes"])
           if int(lib.frlw_encoder_workspace_bytes(*a)) != want]
    assert not bad, f"{len(bad)} of {len(grid)} differ, first: {bad[:3]}"
