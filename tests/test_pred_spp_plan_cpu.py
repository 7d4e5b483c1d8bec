"""The host arithmetic of the train head level and the SPP pools (csrc/pred_ops.hip) through the C ABI on a machine without a GPU.

frlw_pred_plan and frlw_spp_train_plan name the form a call takes -- the template arguments and the grid of k_pred_fwd / k_pred_bwd,
the channel width and the dynamic LDS of k_spp_train_fwd / k_spp_train_bwd.  The launchers take their form from the function the
queries call, so the table below pins the launches themselves; tests/test_pred_spp_forms_gpu.py asserts the plan of every case it
runs with the same queries.  The table holds the values the rules gave when the queries were added; a sweep against the rules
restated here covers the sizes in between.

The refusals are calls the entries turn down before any HIP runtime call: nothing is dereferenced, nothing is launched."""
import ctypes as C

import pytest

from frlw_evd_amd import _lib

OK, ARG, UNSUPPORTED, WORKSPACE = _lib.FRLW_OK, _lib.FRLW_ERR_ARG, _lib.FRLW_ERR_UNSUPPORTED, _lib.FRLW_ERR_WORKSPACE
SPP_MAX_LDS = 144 * 1024


def pred_plan(M, C_, nc):
    out = (C.c_int32 * 3)(-7, -7, -7)
    return _lib.load().frlw_pred_plan(M, C_, nc, out), tuple(out)


def spp_plan(B, H, W, C_):
    out = (C.c_int32 * 3)(-7, -7, -7)
    return _lib.load().frlw_spp_train_plan(B, H, W, C_, out), tuple(out)


# ---- the plan table -------------------------------------------------------------------------------------------------------------
PRED_TABLE = [  # (M, C, nc), {CPL, NG, n_wg} (None: not pinned by the table)
    ((1, 4, 1), (1, 1, 1)),
    ((64, 256, 3), (1, 1, 1)),
    ((65, 260, 3), (2, 1, 2)),
    ((1024, 256, 4), (1, 2, 16)),
    ((1025, 512, 11), (2, 2, 17)),
    ((65536, 8, 1), (None, None, 1024)),
    ((81920, 8, 1), (None, None, 1024)),
]

SPP_TABLE = [  # (B, H, W, C), ch, backward LDS bytes (None: only the formula below)
    ((256, 2, 3, 256), 64, None),
    ((512, 2, 3, 72), 64, None),
    ((512, 2, 3, 64), 32, None),
    ((1024, 8, 16, 64), 64, None),
    ((1024, 3, 43, 64), 32, None),
    ((1024, 16, 16, 32), 32, None),
    ((1024, 1, 257, 32), 16, None),
    ((64, 8, 10, 256), 16, None),
    ((2, 16, 32, 40), 16, 147456),
]


@pytest.mark.parametrize("args,want", PRED_TABLE, ids=[str(a) for a, _ in PRED_TABLE])
def test_pred_plan_table(args, want):
    rc, got = pred_plan(*args)
    assert rc == OK
    assert all(w is None or g == w for g, w in zip(got, want)), (got, want)
    assert got[0] in (1, 2) and got[1] in (1, 2)


@pytest.mark.parametrize("args,ch,lds_bwd", SPP_TABLE, ids=[str(a) for a, _, _ in SPP_TABLE])
def test_spp_plan_table(args, ch, lds_bwd):
    B, H, W, C_ = args
    rc, got = spp_plan(*args)
    assert rc == OK
    assert got[0] == ch, got
    assert got[1] == H * W * ch * 4 and got[2] == 3 * H * W * ch * 6 <= SPP_MAX_LDS, got
    if lds_bwd is not None:
        assert got[2] == lds_bwd


def test_spp_plan_refuses_a_map_of_513_pixels():
    for H, W in ((1, 513), (513, 1), (19, 27)):
        rc, got = spp_plan(1, H, W, 16)
        assert rc == UNSUPPORTED and got == (-7, -7, -7), (H, W, rc, got)
    assert spp_plan(1, 1, 512, 16)[0] == OK


# ---- the rules, restated, over the sizes in between ---------------------------------------------------------------------------------

def pred_rule(M, C_, nc):
    return (2 if C_ > 256 else 1, 2 if 5 + nc > 8 else 1, max(1, min(1024, -(-M // 64))))


def spp_rule(B, HW, C_):
    fit = 0
    for ch in (64, 32, 16):
        if HW * ch * 18 > SPP_MAX_LDS:
            continue
        fit = ch
        if -(-C_ // ch) * B >= 1024:
            return ch
    return fit


PRED_GRID = [(M, C_, nc) for M in (1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 5120, 65535, 65536, 65537, 65600, 81920, 1 << 33)
             for C_ in (4, 8, 64, 252, 256, 260, 508, 512) for nc in (1, 2, 3, 4, 10, 11)]


def test_pred_plan_equals_the_restated_rule_and_sizes_the_scratch():
    """frlw_pred_bwd_scratch_floats == n_wg ((5 + nc) C + 16) with the plan's n_wg, over the table and the grid."""
    lib = _lib.load()
    for M, C_, nc in [a for a, _ in PRED_TABLE] + PRED_GRID:
        rc, got = pred_plan(M, C_, nc)
        assert rc == OK and got == pred_rule(M, C_, nc), (M, C_, nc, rc, got)
        assert lib.frlw_pred_bwd_scratch_floats(M, C_, nc) == got[2] * ((5 + nc) * C_ + 16), (M, C_, nc)


def test_spp_plan_equals_the_restated_rule():
    shapes = [(1, 1), (1, 5), (2, 3), (8, 10), (8, 16), (3, 43), (10, 13), (16, 16), (1, 257), (16, 20), (16, 32), (1, 512)]
    for H, W in shapes:
        for B in (1, 2, 3, 15, 16, 17, 64, 255, 256, 511, 512, 1023, 1024, 4096):
            for C_ in (1, 16, 20, 24, 32, 40, 63, 64, 65, 72, 128, 256, 1024):
                rc, got = spp_plan(B, H, W, C_)
                ch = spp_rule(B, H * W, C_)
                assert rc == OK and got == (ch, H * W * ch * 4, H * W * ch * 18), (B, H, W, C_, rc, got)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
M, CC, NC = 130, 64, 3
B, H, W = 2, 8, 10


def P(i):
    """dummy device pointer number i: 16-byte aligned, never dereferenced"""
    return C.c_void_p(0x10000 * (i + 1))


PRED_FWD_PTRS = ("reg_feat", "cls_feat", "w_reg", "b_reg", "w_obj", "b_obj", "w_cls", "b_cls", "out")
PRED_BWD_PTRS = ("reg_feat", "cls_feat", "dout", "w_reg", "w_obj", "w_cls", "d_reg_feat", "d_cls_feat", "dw_reg", "db_reg", "dw_obj",
                 "db_obj", "dw_cls", "db_cls", "scratch")
SPP_FWD_PTRS = ("x", "out", "argmax")
SPP_BWD_PTRS = ("dout", "argmax", "dx")


def _ptrs(names, null):
    assert set(null) <= set(names)
    return {n: (None if n in null else P(i)) for i, n in enumerate(names)}


def pred_fwd(M_=M, C_=CC, nc=NC, null=()):
    a = _ptrs(PRED_FWD_PTRS, null)
    return _lib.load().frlw_pred_fwd(a["reg_feat"], a["cls_feat"], M_, C_, nc, a["w_reg"], a["b_reg"], a["w_obj"], a["b_obj"], a["w_cls"],
                                     a["b_cls"], a["out"], None)


def pred_bwd(M_=M, C_=CC, nc=NC, short=0, null=()):
    lib = _lib.load()
    a = _ptrs(PRED_BWD_PTRS, null)
    n = lib.frlw_pred_bwd_scratch_floats(M_, C_, nc) - short
    return lib.frlw_pred_bwd(a["reg_feat"], a["cls_feat"], a["dout"], M_, C_, nc, a["w_reg"], a["w_obj"], a["w_cls"], a["d_reg_feat"],
                             a["d_cls_feat"], a["dw_reg"], a["db_reg"], a["dw_obj"], a["db_obj"], a["dw_cls"], a["db_cls"], a["scratch"], n, None)


def spp_fwd(B_=B, H_=H, W_=W, C_=CC, null=()):
    a = _ptrs(SPP_FWD_PTRS, null)
    return _lib.load().frlw_spp_train_fwd(a["x"], B_, H_, W_, C_, a["out"], a["argmax"], None)


def spp_bwd(B_=B, H_=H, W_=W, C_=CC, null=()):
    a = _ptrs(SPP_BWD_PTRS, null)
    return _lib.load().frlw_spp_train_bwd(a["dout"], a["argmax"], B_, H_, W_, C_, a["dx"], None)


def plan_only_pred(**kw):
    return pred_plan(kw.get("M_", M), kw.get("C_", CC), kw.get("nc", NC))[0]


def plan_only_spp(**kw):
    return spp_plan(kw.get("B_", B), kw.get("H_", H), kw.get("W_", W), kw.get("C_", CC))[0]


# One fault per call, so the order of an entry's checks cannot decide the code.
REFUSALS = (
    [(f"pred_fwd: {n} NULL", lambda n=n: pred_fwd(null=(n,)), ARG) for n in PRED_FWD_PTRS]
    + [(f"pred_bwd: {n} NULL", lambda n=n: pred_bwd(null=(n,)), ARG) for n in PRED_BWD_PTRS]
    + [(f"spp_train_fwd: {n} NULL", lambda n=n: spp_fwd(null=(n,)), ARG) for n in SPP_FWD_PTRS]
    + [(f"spp_train_bwd: {n} NULL", lambda n=n: spp_bwd(null=(n,)), ARG) for n in SPP_BWD_PTRS]
    + [(f"{f.__name__}: M = {m}", lambda f=f, m=m: f(M_=m), ARG) for f in (pred_fwd, pred_bwd, plan_only_pred) for m in (0, -1)]
    + [(f"{f.__name__}: {k} = {v}", lambda f=f, k=k, v=v: f(**{k: v}), ARG)
       for f in (spp_fwd, spp_bwd, plan_only_spp) for k in ("B_", "H_", "W_", "C_") for v in (0, -1)]
    + [(f"{f.__name__}: C = {c}", lambda f=f, c=c: f(C_=c), UNSUPPORTED) for f in (pred_fwd, pred_bwd, plan_only_pred) for c in (0, 2, 6, 516)]
    + [(f"{f.__name__}: nc = {n}", lambda f=f, n=n: f(nc=n), UNSUPPORTED) for f in (pred_fwd, pred_bwd, plan_only_pred) for n in (0, 12)]
    + [("pred_bwd: scratch one float short", lambda: pred_bwd(short=1), WORKSPACE),
       ("pred_bwd: scratch one float short, capped grid", lambda: pred_bwd(M_=81920, C_=8, nc=1, short=1), WORKSPACE),
       ("pred_plan: out NULL", lambda: _lib.load().frlw_pred_plan(M, CC, NC, None), ARG),
       ("spp_train_plan: out NULL", lambda: _lib.load().frlw_spp_train_plan(B, H, W, CC, None), ARG)]
    + [(f"{f.__name__}: H W = 513", lambda f=f: f(B_=1, H_=19, W_=27, C_=16), UNSUPPORTED) for f in (spp_fwd, spp_bwd, plan_only_spp)]
    + [(f"{f.__name__}: H W = 70000", lambda f=f: f(B_=1, H_=250, W_=280, C_=16), UNSUPPORTED) for f in (spp_fwd, spp_bwd, plan_only_spp)]
)


@pytest.mark.parametrize("case", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_before_any_launch(case):
    _, call, want = case
    assert call() == want
