"""Every form of the convolution family at its edges, behind guard bands: the cases of tests/conv_edge_cases.py (ragged last
M-tiles at odd Ho x Wo on every tile, column tiles that are mostly past Cout, splits that do not divide the k-tiles, the weight
gradient's pixel walk ending inside a k-tile or spanning images, the data gradient's parity classes of one pixel, dx_add
with rows wider than Cin) against float64 torch, through the C ABI.

The judgement is that of tests/test_conv_forms_gpu.py, unchanged and imported from it: (a) integers in {-3..3} bit-equal to
float64, (b) randn + 0.5 with |y - ref| <= TOL[prec] (|x| (*) |w|) element by element, outputs NaN before the call, the train
forward's mean and variance by the same per-channel bounds, BatchNorm + SiLU by test_bn_silu_forms_gpu.judge; the counters
of frlw_conv_path_counts must move exactly the forms the table names.

New here: every output and every scratch buffer handed to the library (z, y, dz, dx, dw, mean / var / invstd, dgamma / dbeta,
the weight-gradient scratch at exactly frlw_conv2d_wgrad_scratch_floats, the split-K scratch at exactly the floats passed, the
train scratch at exactly frlw_baseconv_train_scratch_bytes, the arrival counters) lies inside a larger allocation, between two
frames of max(4096, 128 rows of the buffer's pitch) words of the NaN 0x7FC0BEEF.  After the call every frame word must be
unchanged (compared as int32): the stores of the epilogues are plain 16-byte stores behind hand-written row and column guards,
and a store one row or one float4 past the end of a buffer of exactly its size would land where nothing looks.

Measured on an MI355X (112 tests, every case well under a second apart from its float64 references; the slowest 1.4 s):
  * worst |err| / bound of the (b) judgements of this file: 0.079 (float32), 0.138 (bf16x3); the forms file records
    0.16 / 0.088 for its own cases.  (Run in one session the forms file prints the larger of the two per arithmetic: the
    ratios go to its WORST as well.)
  * predicted forms that had to be corrected: one.  (3, 64, 31, 39, 64, 3, 1) is the unsplit 64x64 tile through
    frlw_conv2d_fwd only; through the train forward the arrival counters lower the split threshold to 32 k-tiles and its 36
    split 4 ways (split_inkernel_stats in float32, split_vec in bf16x3).  The case stays, as the in-kernel reduction with a
    43-row last slab, and (3, 32, 31, 39, 64, 3, 1) (18 k-tiles) was added for the unsplit 64x64 tile with epilogue statistics at
    the same 43 rows.  Every other shape landed on the form the thresholds predict.  One case was added beyond the list the
    table was drawn from: the weight gradient's 128x128 tile with a ragged last ROW tile (R = 2340, 36 of 128 rows).
  * defects found: none.  Every frame of every case was intact, the arrival counters were zero after every call that
    received them, two runs of every multi-split weight gradient gave the same bits, and in the integer mode the in-kernel and
    the two-launch reduction of the same operands agreed bit for bit.
  * negative control (a library built aside with three in-bounds value changes, run once): the remainder k-tiles of a split
    dropped in k_conv_mfma and in k_wgrad_mfma (kt0 = (nk / splits) z), and the in-kernel statistics counting 32 rows for a
    short wavefront -- 52 of these tests fail, the last change through the mean of the cases whose last slab is short only;
    of the forms file 8 fail, none of them for the statistics.
"""
import ctypes as C
import math
import time

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import conv_edge_cases as ec
import test_conv_forms_gpu as cf
from test_conv_forms_gpu import PREC, TOL, check_rc, conv_ref, counts, dgrad_ref, forms_moved, gen, ptr, run_dgrad, run_fwd, run_wgrad, seed, wgrad_ref

PATTERN = 0x7FC0BEEF  # a quiet NaN with a payload: a frame word read as a float poisons what it touches
WORST = {}            # precision -> worst |err| / bound of the (b) judgements of this file (also added to the forms file's WORST)


def judge(*args, **kw):
    """cf.judge; the ratios it records go to this file's WORST and stay in the forms file's."""
    saved = dict(cf.WORST)
    cf.WORST.clear()
    try:
        cf.judge(*args, **kw)
    finally:
        for p, v in cf.WORST.items():
            WORST[p] = max(WORST.get(p, 0.0), v)
        for p, v in saved.items():
            cf.WORST[p] = max(cf.WORST.get(p, 0.0), v)


@pytest.fixture(autouse=True)
def _case_time(request):
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    print(f"[{request.node.name}] {time.perf_counter() - t0:.2f} s")


# ---- guard bands -----------------------------------------------------------------------------------------------------------

class Frames:
    """Allocator for run_fwd / run_dgrad / run_wgrad and the train calls below: every buffer it hands out lies between two frames
    of PATTERN words, each at least 128 rows of the buffer's pitch and at least 4096 words; check() after the call."""

    def __init__(self):
        self.bufs = []

    def __call__(self, name, shape, pitch, dtype=torch.float32, fill=float("nan")):
        item = torch.empty((), dtype=dtype).element_size()
        nbytes = math.prod(shape) * item
        assert nbytes % 4 == 0, (name, nbytes)
        words = nbytes // 4
        frame = max(4096, 128 * ((pitch * item + 3) // 4))
        frame = (frame + 63) // 64 * 64  # the inner buffer keeps the allocation's alignment to 256 bytes
        raw = torch.full((2 * frame + words,), PATTERN, dtype=torch.int32, device="cuda")
        inner = raw[frame:frame + words].view(dtype).view(shape)
        assert inner.data_ptr() % 16 == 0 and inner.data_ptr() == raw.data_ptr() + 4 * frame
        inner.fill_(fill)
        self.bufs.append((name, raw, frame, words))
        return inner

    def check(self, what):
        torch.cuda.synchronize()
        for name, raw, frame, words in self.bufs:
            for side, fr, origin in (("before", raw[:frame], -frame), ("after", raw[frame + words:], 0)):
                bad = fr != PATTERN
                n = int(bad.sum())
                if n:
                    first = int(bad.nonzero()[0]) + origin
                    raise AssertionError(f"{what}: {name}: {n} words of the frame {side} the buffer were written, the first at word "
                                         f"{first} from the buffer's {'start' if side == 'before' else 'end'}")


def test_frames_catch_a_stray_store():
    """The frames themselves: sizes, alignment, and that one word written on either side of a buffer is reported by name."""
    fr = Frames()
    t = fr("z", (3, 5, 7, 132), 132)
    u = fr("bytes", (1028,), 640, dtype=torch.uint8, fill=0xFF)
    (_, raw, frame, words), (_, raw_u, frame_u, words_u) = fr.bufs
    assert frame >= 128 * 132 and frame >= 4096 and words == t.numel() and torch.isnan(t).all()
    assert frame_u >= 128 * 160 and words_u == 257 and int(u.min()) == 255
    assert raw.view(torch.float32)[:frame].isnan().all()
    fr.check("untouched")
    t.view(-1)[-1] = 1.0
    t.view(-1)[0] = 1.0
    fr.check("the buffer's own first and last word")
    raw[frame + words] = 0
    with pytest.raises(AssertionError, match=r"z: 1 words of the frame after the buffer were written, the first at word 0 "):
        fr.check("stray")
    raw[frame + words] = PATTERN
    raw_u[frame_u - 2] = 0
    with pytest.raises(AssertionError, match=r"bytes: 1 words of the frame before the buffer were written, the first at word -2 "):
        fr.check("stray")


# ---- forward / data gradient / weight gradient through their own entries -------------------------------------------------------

def _ids(table):
    return [c.name for c in table]


def _dims(shape):
    B, Cin, H, W, Cout, k, s = shape
    return B, Cin, H, W, Cout, k, s, ec.out_dim(H, k, s), ec.out_dim(W, k, s)


@pytest.mark.parametrize("mode", ["int", "randn"])
@pytest.mark.parametrize("case", ec.FWD, ids=_ids(ec.FWD))
def test_conv2d_fwd_edges(case, mode):
    B, Cin, H, W, Cout, k, s, Ho, Wo = _dims(case.shape)
    g = torch.Generator(device="cuda").manual_seed(seed(case.name, mode))
    x, w = gen((B, H, W, Cin), mode, g), gen((Cout, Cin, k, k), mode, g)
    ref, absref = conv_ref(x, w, s), conv_ref(x.abs(), w.abs(), s)
    for pname, fs in case.forms.items():
        fr = Frames()
        z, moved = run_fwd(x, w, s, PREC[pname], scratch=True, alloc=fr)
        fr.check(f"{case.name} {pname}")
        assert moved == fs, (pname, moved)
        judge(z, ref, absref, mode, PREC[pname], f"{case.name} {pname}")


@pytest.mark.parametrize("mode", ["int", "randn"])
@pytest.mark.parametrize("case", ec.DGRAD, ids=_ids(ec.DGRAD))
def test_conv2d_dgrad_edges(case, mode):
    B, Cin, H, W, Cout, k, s, Ho, Wo = _dims(case.shape)
    g = torch.Generator(device="cuda").manual_seed(seed(case.name, mode))
    dz, w = gen((B, Ho, Wo, Cout), mode, g), gen((Cout, Cin, k, k), mode, g)
    ref, absref = dgrad_ref(dz, w, s, H, W), dgrad_ref(dz.abs(), w.abs(), s, H, W)
    for pname, fs in case.forms.items():
        fr = Frames()
        dx, moved = run_dgrad(dz, w, s, H, W, PREC[pname], alloc=fr)
        fr.check(f"{case.name} {pname}")
        assert moved == fs, (pname, moved)
        judge(dx, ref, absref, mode, PREC[pname], f"{case.name} {pname}")


@pytest.mark.parametrize("mode", ["int", "randn"])
@pytest.mark.parametrize("case", ec.WGRAD, ids=_ids(ec.WGRAD))
def test_conv2d_wgrad_edges(case, mode):
    B, Cin, H, W, Cout, k, s, Ho, Wo = _dims(case.shape)
    g = torch.Generator(device="cuda").manual_seed(seed(case.name, mode))
    x, dz = gen((B, H, W, Cin), mode, g), gen((B, Ho, Wo, Cout), mode, g)
    shape = (Cout, Cin, k, k)
    ref, absref = wgrad_ref(x, dz, shape, s), wgrad_ref(x.abs(), dz.abs(), shape, s)
    several_splits = case.part < 1.0 or any(c[0] == "wgrad_splits" for c in case.claims)
    for pname, prec in PREC.items():
        fr = Frames()
        dw, moved = run_wgrad(x, dz, k, s, prec, case.part, alloc=fr)
        fr.check(f"{case.name} {pname}")
        assert moved == case.forms, (pname, moved)
        judge(dw, ref, absref, mode, prec, f"{case.name} {pname}")
        if several_splits:  # the reduction over the pixel splits has a fixed order: the same bits on every run
            fr = Frames()
            again, _ = run_wgrad(x, dz, k, s, prec, case.part, alloc=fr)
            fr.check(f"{case.name} {pname}, second run")
            assert torch.equal(again, dw), f"{case.name} {pname}: two runs differ in {int((again != dw).sum())} elements"


# ---- train-mode BaseConv: arrival counters handed over, no operand cache ----------------------------------------------------------

def _train(case, mode, pname, with_dx_add=False):
    import test_bn_silu_forms_gpu as bnf
    L, lib = cf._lib()
    B, Cin, H, W, Cout, k, s, Ho, Wo = _dims(case.shape)
    ffs, bfs = case.forms[pname]
    prec = PREC[pname]
    tol = TOL[prec]
    what = f"{case.name} {mode} {pname}"
    g = torch.Generator(device="cuda").manual_seed(seed(case.name, mode))
    x, w = gen((B, H, W, Cin), mode, g), gen((Cout, Cin, k, k), mode, g)
    gamma = torch.rand(Cout, generator=g, device="cuda") + 0.5
    beta = torch.randn(Cout, generator=g, device="cuda") * 0.2
    dy = torch.randn(B, Ho, Wo, Cout, generator=g, device="cuda")
    ref, absref = conv_ref(x, w, s), conv_ref(x.abs(), w.abs(), s)
    # per channel: mean and biased variance of z, and their bounds (|d mean| <= tol E A; |d var| <= 2 tol (E A^2 + (E A)^2))
    mean_ref, var_ref = ref.mean((0, 1, 2)), ref.var((0, 1, 2), unbiased=False)
    a1, a2 = absref.mean((0, 1, 2)), (absref * absref).mean((0, 1, 2))
    nbytes = lib.frlw_baseconv_train_scratch_bytes(B, H, W, Cin, Cout, k, s)
    npad = max(ec.npad32(Cin), ec.npad32(Cout))

    fr = Frames()
    scratch = fr("train scratch", (nbytes,), 4 * npad, dtype=torch.uint8, fill=0xFF)  # NaN wherever a float is read unwritten
    cnt = fr("arrival counters", (1024,), 1024, dtype=torch.int32, fill=0)
    z, y = fr("z", (B, Ho, Wo, Cout), Cout), fr("y", (B, Ho, Wo, Cout), Cout)
    mean, var, invstd = fr("mean", (Cout,), Cout), fr("var", (Cout,), Cout), fr("invstd", (Cout,), Cout)
    torch.cuda.synchronize()
    before = counts()
    check_rc(lib.frlw_baseconv_train_fwd(ptr(x), ptr(w), ptr(gamma), ptr(beta), C.c_float(1e-5), B, H, W, Cin, Cout, k, s,
                                         ptr(z), ptr(y), ptr(mean), ptr(var), ptr(invstd), None, None, C.c_float(0.1), None,
                                         None, ptr(scratch), nbytes, ptr(cnt), None, prec, None), "train_fwd")
    fr.check(what + " forward")
    assert forms_moved(before) == ffs, (pname, "forward", forms_moved(before))
    assert int(cnt.abs().sum()) == 0, "arrival counters not reset by the forward"
    judge(z, ref, absref, mode, prec, what + " z")
    assert ((mean.double() - mean_ref).abs() <= tol * a1 + 2.0 ** -23 * mean_ref.abs()).all(), what + " mean"
    assert ((var.double() - var_ref).abs() <= 2 * tol * (a2 + a1 * a1) + 2.0 ** -23 * var_ref).all(), what + " var"
    if mode == "int" and case.name in ec.TWIN:  # the two-launch reduction (no counters) of the same operands: the same bits
        fr2 = Frames()
        z2, _ = run_fwd(x, w, s, prec, scratch=True, alloc=fr2)
        fr2.check(what + " two-launch twin")
        assert torch.equal(z2, z), f"{what}: in-kernel and two-launch reductions differ in {int((z2 != z).sum())} elements"
    del ref, absref

    add = add_buf = None
    fuse = None
    if with_dx_add:  # rows of DX_ADD_PITCH floats, the addend at DX_ADD_OFFSET; every other column of the buffer is PATTERN
        frd = Frames()
        add_buf = frd("dx_add", (B, H, W, ec.DX_ADD_PITCH), ec.DX_ADD_PITCH)
        add_buf.view(torch.int32).fill_(PATTERN)
        add = add_buf[..., ec.DX_ADD_OFFSET:ec.DX_ADD_OFFSET + Cin]
        add.copy_(gen((B, H, W, Cin), mode, g))
        add_before = add_buf.view(torch.int32).clone()
        fuse = L.FrlwBaseconvFuse(dx_add=add.data_ptr(), dx_add_row_stride=ec.DX_ADD_PITCH)
    dz, dx, dw = fr("dz", (B, Ho, Wo, Cout), Cout), fr("dx", (B, H, W, Cin), Cin), fr("dw", (Cout, Cin, k, k), Cin * k * k)
    dgamma, dbeta = fr("dgamma", (Cout,), Cout), fr("dbeta", (Cout,), Cout)
    torch.cuda.synchronize()
    before = counts()
    check_rc(lib.frlw_baseconv_train_bwd(ptr(dy), 0, ptr(x), ptr(z), ptr(w), ptr(gamma), ptr(beta), ptr(mean), ptr(invstd),
                                         B, H, W, Cin, Cout, k, s, ptr(dz), ptr(dx), ptr(dw), ptr(dgamma), ptr(dbeta), None,
                                         ptr(scratch), nbytes, ptr(cnt), C.byref(fuse) if fuse else None, prec, None), "train_bwd")
    fr.check(what + " backward")
    assert forms_moved(before) == bfs, (pname, "backward", forms_moved(before))
    assert int(cnt.abs().sum()) == 0, "arrival counters not reset by the backward"
    assert torch.isfinite(dz).all()
    if with_dx_add:
        frd.check(what + " backward")
        assert torch.equal(add_buf.view(torch.int32), add_before), what + ": the addend buffer was written"
    # BatchNorm + SiLU per channel against float64 on the z the forward returned (bounds: test_bn_silu_forms_gpu.py)
    bn_ref = bnf.reference(z.reshape(-1, Cout), gamma, beta, dy.reshape(-1, Cout))
    bnf.assert_ok(bnf.judge(bn_ref, dict(mean=mean, var=var, invstd=invstd, y=y.reshape(-1, Cout), dz=dz.reshape(-1, Cout), dgamma=dgamma,
                                     dbeta=dbeta)), what + " BatchNorm + SiLU")
    del bn_ref
    # the data and weight gradients of the dz the BatchNorm backward produced: (b) in both data modes
    judge(dx, dgrad_ref(dz, w, s, H, W), dgrad_ref(dz.abs(), w.abs(), s, H, W), "randn", prec, what + " dx", res=add)
    judge(dw, wgrad_ref(x, dz, w.shape, s), wgrad_ref(x.abs(), dz.abs(), w.shape, s), "randn", prec, what + " dw")


@pytest.mark.parametrize("pname", list(PREC))
@pytest.mark.parametrize("mode", ["int", "randn"])
@pytest.mark.parametrize("case", ec.TRAIN, ids=_ids(ec.TRAIN))
def test_baseconv_train_edges(case, mode, pname):
    _train(case, mode, pname)


@pytest.mark.parametrize("pname", list(PREC))
def test_dx_add_with_wide_rows_at_a_ragged_tile(pname):
    """dx = float64 data gradient + addend under (b), the addend in the bound as judge treats `res`; the addend's rows are
    DX_ADD_PITCH floats apart and everything around the slice is a frame."""
    _train(ec.DX_ADD, "randn", pname, with_dx_add=True)


def test_worst_ratios():
    """(last in the file) the figures of the module docstring."""
    if WORST:
        print("worst |err| / bound at the edges:", {p: round(v, 4) for p, v in WORST.items()})
