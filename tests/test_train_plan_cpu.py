"""The host arithmetic of the training operators (csrc/train_ops.hip and its train_*.h headers) through the C ABI on a machine
without a GPU.

The six integer queries -- operand sizes, the operand cache, the parity decision, the weight gradient's scratch, the statistics
scratch and the scratch of the block entries -- are held to the values the library gave BEFORE the unit was split and its
scratch layout, stacked-pair record and split arithmetic each became one function (tests/golden/train_plan.json, made by
tests/golden/make_golden_train_plan.py from that earlier build).  The Python side caches scratch by
frlw_baseconv_train_scratch_bytes and the form tests NaN-fill exactly that many bytes, so it must not move by a byte.

The refusals are calls the entries turn down before any HIP runtime call: nothing is dereferenced, nothing is launched."""
import ctypes as C
import json
import os

import pytest

from frlw_evd_amd import _lib


def test_queries_equal_the_recorded_values(golden_dir):
    g = json.load(open(os.path.join(golden_dir, "train_plan.json")))
    lib = _lib.load()
    assert sorted(g) == ["frlw_baseconv_train_scratch_bytes", "frlw_baseconv_weight_cache_floats", "frlw_bn_scratch_doubles",
                         "frlw_conv2d_dgrad_parity", "frlw_conv2d_wgrad_scratch_floats", "frlw_conv_operand_floats"]
    assert sum(len(q["values"]) for q in g.values()) == 4350
    assert set(g["frlw_conv2d_dgrad_parity"]["values"]) == {0, 1}
    for name, q in g.items():
        f = getattr(lib, name)
        assert len(q["args"]) == len(q["values"]) > 0
        bad = [(a, int(f(*a)), want) for a, want in zip(q["args"], q["values"]) if int(f(*a)) != want]
        assert not bad, f"{name}: {len(bad)} of {len(q['values'])} differ, first: {bad[:3]}"


# ---- refusals -------------------------------------------------------------------------------------------------------------------
ARG, UNSUPPORTED, WORKSPACE = _lib.FRLW_ERR_ARG, _lib.FRLW_ERR_UNSUPPORTED, _lib.FRLW_ERR_WORKSPACE
B, H, W, CIN, COUT, K = 2, 8, 8, 8, 36, 3
SPLIT = 16


def P(i):
    """dummy device pointer number i: 16-byte aligned, never dereferenced"""
    return C.c_void_p(0x10000 * (i + 1))


def pair(**kw):
    """a valid stacked pair (both directions' fields), then the fault"""
    f = dict(split=SPLIT, w2=P(40), gamma2=P(41), beta2=P(42), running_mean2=P(43), running_var2=P(44), y2=P(45), dy2=P(46))
    f.update(kw)
    return _lib.FrlwBaseconvFuse(**f)


def fwd(lib, stride=1, short=0, fuse=None, running=False, **null):
    """frlw_baseconv_train_fwd of a valid call with the named pointer arguments NULL"""
    a = dict(x=P(0), w=P(1), gamma=P(2), beta=P(3), z=P(4), y=P(5), mean=P(6), var=P(7), invstd=P(8), w_cache=None, scratch=P(9))
    a.update({k: None for k in null})
    n = lib.frlw_baseconv_train_scratch_bytes(B, H, W, CIN, COUT, K, stride) - short
    return lib.frlw_baseconv_train_fwd(a["x"], a["w"], a["gamma"], a["beta"], C.c_float(1e-3), B, H, W, CIN, COUT, K, stride, a["z"], a["y"],
                                       a["mean"], a["var"], a["invstd"], P(10) if running else None, P(11) if running else None,
                                       C.c_float(0.03), None, a["w_cache"], a["scratch"], n, None, C.byref(fuse) if fuse else None, 0, None)


def bwd(lib, stride=1, short=0, fuse=None, cache=True, **null):
    """frlw_baseconv_train_bwd of a valid call with the named pointer arguments NULL"""
    a = dict(dy=P(0), x=P(1), z=P(2), w=P(3), gamma=P(4), beta=P(5), mean=P(6), invstd=P(7), dz=P(8), dx=P(9), dw=P(10), dgamma=P(11),
             dbeta=P(12), scratch=P(13))
    a.update({k: None for k in null})
    n = lib.frlw_baseconv_train_scratch_bytes(B, H, W, CIN, COUT, K, stride) - short
    return lib.frlw_baseconv_train_bwd(a["dy"], 0, a["x"], a["z"], a["w"], a["gamma"], a["beta"], a["mean"], a["invstd"], B, H, W, CIN, COUT, K,
                                       stride, a["dz"], a["dx"], a["dw"], a["dgamma"], a["dbeta"], P(14) if cache else None, a["scratch"], n, None,
                                       C.byref(fuse) if fuse else None, 0, None)


def bad_size():
    f = pair()
    f.struct_size -= 8
    return f


# One fault per call, so the order of an entry's checks cannot decide the code.  Recorded from the library before the split of the
# unit, except the two marked "moved": there the entry used to refuse only after it had enqueued the weight layout (stride) or the
# convolution (running statistics), so before the change they could be observed on a GPU only; the codes are the ones it returned.
REFUSALS = [
    ("fwd: x NULL", lambda lib: fwd(lib, x=1), ARG),
    ("fwd: neither w nor w_cache", lambda lib: fwd(lib, w=1), ARG),
    ("fwd: gamma NULL", lambda lib: fwd(lib, gamma=1), ARG),
    ("fwd: z NULL", lambda lib: fwd(lib, z=1), ARG),
    ("fwd: invstd NULL", lambda lib: fwd(lib, invstd=1), ARG),
    ("fwd: scratch NULL", lambda lib: fwd(lib, scratch=1), ARG),
    ("fwd: struct_size", lambda lib: fwd(lib, fuse=bad_size()), ARG),
    ("fwd: split < 0", lambda lib: fwd(lib, fuse=pair(split=-4)), ARG),
    ("fwd: split % 4", lambda lib: fwd(lib, fuse=pair(split=SPLIT + 2)), ARG),
    ("fwd: split >= Cout", lambda lib: fwd(lib, fuse=pair(split=COUT)), ARG),
    ("fwd: gamma2 NULL", lambda lib: fwd(lib, fuse=pair(gamma2=None)), ARG),
    ("fwd: beta2 NULL", lambda lib: fwd(lib, fuse=pair(beta2=None)), ARG),
    ("fwd: y2 NULL", lambda lib: fwd(lib, fuse=pair(y2=None)), ARG),
    ("fwd: w without w2", lambda lib: fwd(lib, fuse=pair(w2=None)), ARG),
    ("fwd: residual with split", lambda lib: fwd(lib, fuse=pair(residual=P(50))), ARG),
    ("fwd: scratch one byte short", lambda lib: fwd(lib, short=1), WORKSPACE),
    ("fwd: stride 3 (moved)", lambda lib: fwd(lib, stride=3), UNSUPPORTED),
    ("fwd: running statistics without running_mean2 (moved)", lambda lib: fwd(lib, fuse=pair(running_mean2=None), running=True), ARG),
    ("fwd: running statistics without running_var2 (moved)", lambda lib: fwd(lib, fuse=pair(running_var2=None), running=True), ARG),
    ("bwd: dy NULL", lambda lib: bwd(lib, dy=1), ARG),
    ("bwd: w NULL", lambda lib: bwd(lib, w=1), ARG),
    ("bwd: dz NULL", lambda lib: bwd(lib, dz=1), ARG),
    ("bwd: dbeta NULL", lambda lib: bwd(lib, dbeta=1), ARG),
    ("bwd: scratch NULL", lambda lib: bwd(lib, scratch=1), ARG),
    ("bwd: struct_size", lambda lib: bwd(lib, fuse=bad_size()), ARG),
    ("bwd: dx_add with stride 2", lambda lib: bwd(lib, stride=2, fuse=_lib.FrlwBaseconvFuse(dx_add=P(50))), UNSUPPORTED),
    ("bwd: dx_add without dx", lambda lib: bwd(lib, fuse=_lib.FrlwBaseconvFuse(dx_add=P(50)), dx=1), UNSUPPORTED),
    ("bwd: split < 0", lambda lib: bwd(lib, fuse=pair(split=-4)), ARG),
    ("bwd: split % 4", lambda lib: bwd(lib, fuse=pair(split=SPLIT + 2)), ARG),
    ("bwd: split >= Cout", lambda lib: bwd(lib, fuse=pair(split=COUT)), ARG),
    ("bwd: gamma2 NULL", lambda lib: bwd(lib, fuse=pair(gamma2=None)), ARG),
    ("bwd: beta2 NULL", lambda lib: bwd(lib, fuse=pair(beta2=None)), ARG),
    ("bwd: dy2 NULL", lambda lib: bwd(lib, fuse=pair(dy2=None)), ARG),
    ("bwd: no w_cache and no w2", lambda lib: bwd(lib, fuse=pair(w2=None), cache=False), ARG),
    ("bwd: scratch one byte short", lambda lib: bwd(lib, short=1), WORKSPACE),
    ("conv2d_fwd: stride 3", lambda lib: lib.frlw_conv2d_fwd(P(0), B, H, W, CIN, P(1), COUT, K, 3, P(2), None, 0, 0, None), UNSUPPORTED),
    ("conv2d_fwd: precision 2", lambda lib: lib.frlw_conv2d_fwd(P(0), B, H, W, CIN, P(1), COUT, K, 1, P(2), None, 0, 2, None), ARG),
    ("conv2d_dgrad: precision 2", lambda lib: lib.frlw_conv2d_dgrad(P(0), B, H, W, COUT, P(1), CIN, K, 1, H, W, P(2), None, 0, 2, None), ARG),
    ("conv2d_dgrad: stride 3", lambda lib: lib.frlw_conv2d_dgrad(P(0), B, H, W, COUT, P(1), CIN, K, 3, H, W, P(2), None, 0, 0, None), UNSUPPORTED),
    ("conv2d_dgrad: even k", lambda lib: lib.frlw_conv2d_dgrad(P(0), B, H, W, COUT, P(1), CIN, 2, 1, H, W, P(2), None, 0, 0, None), UNSUPPORTED),
    ("conv2d_dgrad: parity classes, H != 2 Ho", lambda lib: lib.frlw_conv2d_dgrad(P(0), B, 5, 4, COUT, P(1), CIN, K, 2, H, W, P(2), None, 0, 0, None), ARG),
    ("conv2d_dgrad: parity classes, dz NULL", lambda lib: lib.frlw_conv2d_dgrad(None, B, 4, 4, COUT, P(1), CIN, K, 2, H, W, P(2), None, 0, 0, None), ARG),
    ("conv2d_dgrad: parity classes, bf16x3 with Cout % 16", lambda lib: lib.frlw_conv2d_dgrad(P(0), B, 4, 4, COUT, P(1), CIN, K, 2, H, W, P(2), None, 0, 1, None), UNSUPPORTED),
    ("conv_path_counts: NULL", lambda lib: lib.frlw_conv_path_counts(None, 4), ARG),
    ("bn_path_counts: n = 0", lambda lib: lib.frlw_bn_path_counts((C.c_uint64 * 4)(), 0), ARG),
]


@pytest.mark.parametrize("case", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_before_any_launch(case):
    _, call, want = case
    assert call(_lib.load()) == want
