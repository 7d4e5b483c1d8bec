"""Every form of the train head level (csrc/pred_ops.hip: k_pred_fwd<CPL, NG>, k_pred_bwd<CPL, NG>, k_pred_bwd_final) and of the
SPP pools (k_spp_train_fwd, k_spp_train_bwd) against float64, through the C ABI.  Each case names the plan it must get
(frlw_pred_plan: {CPL, NG, n_wg}; frlw_spp_train_plan: channels per workgroup) and asserts it with the query before it runs;
test_tables_reach_every_form checks that the tables reach all four <CPL, NG> forms, every n_wg class of the workgroup split and
of k_pred_bwd_final's 16 segments (1, 16, 17, 1024 without and with the cap) and every channel width -- a retune that moves a
case to another form fails there.

Every output and the scratch are NaN before each call, every output has a 64-float guard band behind it that must still be NaN
afterwards, and every output element must be finite (SPP forward: equal to the reference, which holds NaN and infinities on
purpose; it runs a second time over a finite fill, so an element left unwritten where the reference is NaN shows too).

Prediction level, judged twice per case:
  (a) integer data in {-3..3}: forward sums stay below 9 * 512 + 3, weight gradients below 9 M < 2^24, so float32 is exact in any
      order and every output must EQUAL the float64 reference.  A dropped, doubled or misplaced row, chunk, output index or
      partial is an integer-sized error.
  (b) randn + 0.5 data: per element |got - ref| <= 2 k u absref, u = 2^-24, absref = the same operation on absolute values in
      float64, k = the float32 roundings on the output's longest path in the kernel's order, from the plan:
        out       4 CPL + 8   (per chunk 4 products and 4 additions interleaved as x.x w.x + ... and s +=; 6 butterfly steps; bias)
        d_feat    outputs on that side + 1   (reg: 5 products accumulated, cls: nc)
        dw, db    ceil(M / (8 n_wg)) + 8 + ceil(n_wg / 16) + 17   (rows of a wavefront; 8 wavefronts through LDS; a segment of
                  workgroup partials; the 16 segments; the product)
      The factor 2 is the margin over that count (a differing contraction of multiply-adds).  Negative controls: a reference
      without one 4-channel chunk (forward) or without one row (dw) at M = 65 is rejected.
SPP pools: the reference is torch.nn.functional.max_pool2d(return_indices=True) on the CPU in float64 (NCHW-contiguous) -- the
first maximum wins a tie, the last NaN of a window wins, an all -inf window takes its first element; a literal triple loop over
one 3 x 4 map pins those three rules without ATen.  out and argmax must equal it exactly (NaN positions equal).  Backward: dout
in {-3..3} meets at most 1 + 25 + 81 + 169 terms in a pixel, so dx must equal the float64 scatter; randn dout is held to
2 * 277 u absref.

Worst |err| / bound when the tests were written (MI355X; test_pred_spp_worst_ratio_report prints them): out 0.136, d_feat 0.333,
dw 0.032, db 0.025, SPP dx 0.0093.
"""
import ctypes as C
import math
import zlib

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
NAN = float("nan")
GUARD = 64
WORST = {}  # output kind -> worst |err| / bound over the (b) cases


def _lib():
    from frlw_evd_amd import _lib as L
    return L, L.load()


def ptr(t):
    return C.c_void_p(t.data_ptr())


def seed(*key):
    return zlib.crc32(repr(key).encode())


class Guarded:
    """n elements filled with `fill` and a guard band of 64 more behind them (one allocation: 16-byte aligned)"""

    def __init__(self, n, fill=NAN, dtype=torch.float32, guard_fill=None):
        self.n = n
        self.guard_fill = fill if guard_fill is None else guard_fill
        self.buf = torch.full((n + GUARD,), fill, dtype=dtype, device=DEV)
        self.buf[n:] = self.guard_fill
        assert self.buf.data_ptr() % 16 == 0
        self.t = self.buf[:n]

    def guard_intact(self):
        g = self.buf[self.n:]
        return bool(torch.isnan(g).all()) if isinstance(self.guard_fill, float) and math.isnan(self.guard_fill) else bool((g == self.guard_fill).all())


def pred_plan(M, C_, nc):
    L, lib = _lib()
    out = (C.c_int32 * 3)()
    assert lib.frlw_pred_plan(M, C_, nc, out) == L.FRLW_OK
    return tuple(out)


def spp_plan(B, H, W, C_):
    L, lib = _lib()
    out = (C.c_int32 * 3)()
    assert lib.frlw_spp_train_plan(B, H, W, C_, out) == L.FRLW_OK
    return tuple(out)


# ================================================================================================================================
# the prediction level
# ================================================================================================================================
# (M, C, nc), the plan {CPL, NG, n_wg} the case must get.  C: one lane (4), a partly filled wavefront (64, 252), a full one (256),
# only lane 0 owning a second chunk (260), 508, 512.  nc: 1, 3 (nout = 8 fills group 0), 4 (the first output of group 1), 11.
# M: 1 (seven idle wavefronts write zero partials), 63 / 64 / 65 around one workgroup, 1024 / 1025 (16 and 17 workgroups: the
# last segments of k_pred_bwd_final are empty), 65 536 (1024 workgroups, not capped), 81 920 and 65 600 (capped: a wavefront
# strides over more than 8 rows; 65 600 x 260 x 2 is <2, 1> under the cap).
PRED_CASES = [
    ((1, 4, 1), (1, 1, 1)),
    ((1, 260, 4), (2, 2, 1)),
    ((1, 512, 11), (2, 2, 1)),
    ((63, 64, 3), (1, 1, 1)),
    ((63, 252, 1), (1, 1, 1)),
    ((63, 508, 4), (2, 2, 1)),
    ((64, 256, 3), (1, 1, 1)),
    ((64, 260, 11), (2, 2, 1)),
    ((64, 508, 1), (2, 1, 1)),
    ((65, 260, 3), (2, 1, 2)),
    ((65, 252, 4), (1, 2, 2)),
    ((65, 4, 11), (1, 2, 2)),
    ((65, 512, 1), (2, 1, 2)),
    ((1024, 256, 4), (1, 2, 16)),
    ((1024, 512, 3), (2, 1, 16)),
    ((1024, 64, 11), (1, 2, 16)),
    ((1024, 252, 3), (1, 1, 16)),
    ((1025, 512, 11), (2, 2, 17)),
    ((1025, 508, 3), (2, 1, 17)),
    ((1025, 4, 4), (1, 2, 17)),
    ((1025, 256, 1), (1, 1, 17)),
    ((65536, 64, 11), (1, 2, 1024)),
    ((65536, 4, 3), (1, 1, 1024)),
    ((81920, 8, 1), (1, 1, 1024)),
    ((65600, 260, 2), (2, 1, 1024)),
]
PRED_IDS = [f"M{m}_C{c}_nc{n}" for (m, c, n), _ in PRED_CASES]
PRED_OUTPUTS = ("out", "d_reg", "d_cls", "dw_reg", "db_reg", "dw_obj", "db_obj", "dw_cls", "db_cls")


def n_wg_class(M, n_wg):
    """1, 16, 17, or 1024 reached without / with the cap of kPredMaxWg"""
    if n_wg != 1024:
        return n_wg
    return "1024 uncapped" if -(-M // 64) == 1024 else "1024 capped"


def pred_inputs(M, C_, nc, kind, g):
    """float32 inputs of one call: integers in {-3..3}, or randn + 0.5"""
    shapes = dict(reg=(M, C_), cls=(M, C_), w_reg=(4, C_), b_reg=(4,), w_obj=(1, C_), b_obj=(1,), w_cls=(nc, C_), b_cls=(nc,),
                  dout=(M, 5 + nc))
    if kind == "int":
        return {k: torch.randint(-3, 4, s, generator=g, device=DEV).float() for k, s in shapes.items()}
    return {k: torch.randn(s, generator=g, device=DEV) + 0.5 for k, s in shapes.items()}


def pred_reference(d, drop_chunk=None, drop_row=None):
    """The operation of the module docstring of csrc/pred_ops.hip in float64, and the same on absolute values (absref).
    drop_chunk = (m, chunk): the forward without that 4-channel chunk of row m; drop_row = m: the weight and bias gradients without
    row m -- the deliberately wrong references of the negative controls."""
    def both(f):
        return f({k: v.double() for k, v in d.items()}), f({k: v.double().abs() for k, v in d.items()})

    def op(x):
        reg, cls = x["reg"], x["cls"]
        if drop_chunk is not None:
            m, ch = drop_chunk
            reg, cls = reg.clone(), cls.clone()
            reg[m, 4 * ch:4 * ch + 4] = 0
            cls[m, 4 * ch:4 * ch + 4] = 0
        w5 = torch.cat([x["w_reg"], x["w_obj"]], 0)
        out = torch.cat([reg @ w5.T + torch.cat([x["b_reg"], x["b_obj"]]), cls @ x["w_cls"].T + x["b_cls"]], 1)
        g = x["dout"]
        d_reg, d_cls = g[:, :5] @ w5, g[:, 5:] @ x["w_cls"]
        gw = g
        if drop_row is not None:
            gw = g.clone()
            gw[drop_row] = 0
        dw5, dw_cls, db = gw[:, :5].T @ x["reg"], gw[:, 5:].T @ x["cls"], gw.sum(0)
        return dict(out=out, d_reg=d_reg, d_cls=d_cls, dw_reg=dw5[:4], db_reg=db[:4], dw_obj=dw5[4:5], db_obj=db[4:5], dw_cls=dw_cls,
                    db_cls=db[5:])
    return both(op)


def run_pred(M, C_, nc, d):
    """frlw_pred_fwd + frlw_pred_bwd on NaN-filled guarded outputs and NaN-filled scratch; asserts guards and finiteness."""
    L, lib = _lib()
    nout = 5 + nc
    sizes = dict(out=M * nout, d_reg=M * C_, d_cls=M * C_, dw_reg=4 * C_, db_reg=4, dw_obj=C_, db_obj=1, dw_cls=nc * C_, db_cls=nc)
    o = {k: Guarded(n) for k, n in sizes.items()}
    n_sc = lib.frlw_pred_bwd_scratch_floats(M, C_, nc)
    sc = Guarded(n_sc)
    rc = lib.frlw_pred_fwd(ptr(d["reg"]), ptr(d["cls"]), M, C_, nc, ptr(d["w_reg"]), ptr(d["b_reg"]), ptr(d["w_obj"]), ptr(d["b_obj"]),
                           ptr(d["w_cls"]), ptr(d["b_cls"]), ptr(o["out"].t), None)
    assert rc == L.FRLW_OK, f"frlw_pred_fwd -> {rc}"
    rc = lib.frlw_pred_bwd(ptr(d["reg"]), ptr(d["cls"]), ptr(d["dout"]), M, C_, nc, ptr(d["w_reg"]), ptr(d["w_obj"]), ptr(d["w_cls"]),
                           ptr(o["d_reg"].t), ptr(o["d_cls"].t), ptr(o["dw_reg"].t), ptr(o["db_reg"].t), ptr(o["dw_obj"].t),
                           ptr(o["db_obj"].t), ptr(o["dw_cls"].t), ptr(o["db_cls"].t), ptr(sc.t), n_sc, None)
    assert rc == L.FRLW_OK, f"frlw_pred_bwd -> {rc}"
    torch.cuda.synchronize()
    for k, gd in list(o.items()) + [("scratch", sc)]:
        assert gd.guard_intact(), f"{k}: written past the end"
    shapes = dict(out=(M, nout), d_reg=(M, C_), d_cls=(M, C_), dw_reg=(4, C_), db_reg=(4,), dw_obj=(1, C_), db_obj=(1,), dw_cls=(nc, C_),
                  db_cls=(nc,))
    got = {k: o[k].t.view(shapes[k]) for k in PRED_OUTPUTS}
    for k, t in got.items():
        bad = ~torch.isfinite(t)
        assert not bad.any(), f"{k}: {int(bad.sum())} of {t.numel()} elements not finite (not written, or stale scratch read)"
    return got


def pred_k(M, nc, plan):
    """float32 roundings on the longest path of every output, from the plan (module docstring)"""
    cpl, _, n_wg = plan
    k_w = -(-M // (8 * n_wg)) + 8 + -(-n_wg // 16) + 17
    k = dict(out=4 * cpl + 8, d_reg=5 + 1, d_cls=nc + 1)
    k.update({n: k_w for n in ("dw_reg", "db_reg", "dw_obj", "db_obj", "dw_cls", "db_cls")})
    return k


def kind_of(name):
    return "d_feat" if name in ("d_reg", "d_cls") else name.split("_")[0]


def judge_pred(got, ref, absref, k, record=True):
    """the outputs that miss |got - ref| <= 2 k u absref somewhere, with their worst ratio"""
    fails = []
    for n in PRED_OUTPUTS:
        r = (got[n].double() - ref[n]).abs() / (2 * k[n] * U * absref[n]).clamp_min(1e-300)
        worst = float(r.max())
        if record:
            WORST[kind_of(n)] = max(WORST.get(kind_of(n), 0.0), worst)
        if not worst <= 1.0:
            fails.append(f"{n}: worst |err| / bound {worst:.3g} at {tuple(int(i) for i in torch.unravel_index(r.argmax(), r.shape))}")
    return fails


@pytest.mark.parametrize("case", PRED_CASES, ids=PRED_IDS)
def test_pred_integer_data_is_exact(case):
    (M, C_, nc), plan = case
    assert pred_plan(M, C_, nc) == plan
    d = pred_inputs(M, C_, nc, "int", torch.Generator(device=DEV).manual_seed(seed("pred int", M, C_, nc)))
    got = run_pred(M, C_, nc, d)
    ref, absref = pred_reference(d)
    assert float(absref["out"].max()) <= 9 * 512 + 3 and float(max(absref[n].max() for n in PRED_OUTPUTS)) < 2 ** 24
    wrong = {n: int((got[n].double() != ref[n]).sum()) for n in PRED_OUTPUTS if not torch.equal(got[n].double(), ref[n])}
    assert not wrong, f"elements that differ from float64: {wrong}"


@pytest.mark.parametrize("case", PRED_CASES, ids=PRED_IDS)
def test_pred_randn_data_within_rounding(case):
    (M, C_, nc), plan = case
    assert pred_plan(M, C_, nc) == plan
    d = pred_inputs(M, C_, nc, "randn", torch.Generator(device=DEV).manual_seed(seed("pred randn", M, C_, nc)))
    got = run_pred(M, C_, nc, d)
    ref, absref = pred_reference(d)
    fails = judge_pred(got, ref, absref, pred_k(M, nc, plan))
    assert not fails, "; ".join(fails)
    again = run_pred(M, C_, nc, d)
    assert all(torch.equal(got[n], again[n]) for n in PRED_OUTPUTS), "two runs differ"


def test_pred_bound_rejects_a_dropped_chunk_and_a_dropped_row():
    """Negative control of (b) at M = 65: the kernels against a forward reference without one 4-channel chunk of one row, and
    against a weight-gradient reference without one row, miss the bound (and meet it against the true reference)."""
    (M, C_, nc), plan = PRED_CASES[PRED_IDS.index("M65_C260_nc3")]
    d = pred_inputs(M, C_, nc, "randn", torch.Generator(device=DEV).manual_seed(seed("pred control")))
    got = run_pred(M, C_, nc, d)
    k = pred_k(M, nc, plan)
    assert not judge_pred(got, *pred_reference(d), k, record=False)
    no_chunk = judge_pred(got, *pred_reference(d, drop_chunk=(40, 64)), k, record=False)  # (chunk 64: lane 0's second chunk)
    assert [f.split(":")[0] for f in no_chunk] == ["out"], no_chunk
    no_row = judge_pred(got, *pred_reference(d, drop_row=64), k, record=False)
    assert [f.split(":")[0] for f in no_row] == ["dw_reg", "db_reg", "dw_obj", "db_obj", "dw_cls", "db_cls"], no_row


def test_pred_level_wrapper_layouts():
    """train_ops.pred_level with NCHW-contiguous inputs and a dout that is a channel slice of a wider channels_last tensor equals
    the call with channels_last inputs and a contiguous dout, bit for bit."""
    from frlw_evd_amd.yolox import train_ops
    B, C_, H, W, nc = 2, 260, 5, 7, 4
    torch.manual_seed(11)
    convs = [torch.nn.Conv2d(C_, n, 1).cuda() for n in (4, 1, nc)]
    reg0, cls0 = torch.randn(B, C_, H, W, device=DEV), torch.randn(B, C_, H, W, device=DEV)
    wide = torch.randn(B, 5 + nc + 7, H, W, device=DEV).contiguous(memory_format=torch.channels_last)
    assert train_ops.pred_eligible(reg0, cls0, *convs)

    def call(reg, cls, gout):
        reg, cls = reg.requires_grad_(True), cls.requires_grad_(True)
        for p in (p for c in convs for p in c.parameters()):
            p.grad = None
        out = train_ops.pred_level(reg, cls, *convs)
        out.backward(gout)
        return [out.detach().clone(), reg.grad.clone(), cls.grad.clone()] + [p.grad.clone() for c in convs for p in c.parameters()]
    gslice = wide[:, 3:3 + 5 + nc]
    assert reg0.is_contiguous() and not gslice.is_contiguous() and not gslice.is_contiguous(memory_format=torch.channels_last)
    a = call(reg0.clone(), cls0.clone(), gslice)
    b = call(reg0.clone().contiguous(memory_format=torch.channels_last), cls0.clone().contiguous(memory_format=torch.channels_last),
             gslice.contiguous())
    assert len(a) == len(b) == 9
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and torch.isfinite(x).all() and torch.equal(x, y), i


# ================================================================================================================================
# the SPP pools
# ================================================================================================================================
# (B, H, W, C), channels per workgroup the case must get
SPP_CASES = [
    ((256, 2, 3, 256), 64),    # pstep 4
    ((512, 2, 3, 72), 64),     # the second group holds 8 valid channels
    ((512, 2, 3, 64), 32),
    ((1024, 13, 10, 32), 32),  # 64 channels do not fit the LDS
    ((2, 16, 32, 40), 16),     # the 144 KiB launch, C not a multiple of ch
    ((1, 1, 1, 16), 16),       # the smallest map
    ((1, 1, 40, 16), 16),      # a map smaller than a window
    ((1, 40, 1, 20), 16),
    ((3, 3, 4, 24), 16),       # every window clipped on all sides
    ((2, 8, 10, 256), 16),     # the training shape
]
SPP_IDS = ["x".join(map(str, s)) for s, _ in SPP_CASES]
ARG_FILL = -21846  # 0xAAAA: no pixel of a map of at most 512
_SPP_CACHE = {}


def spp_input(B, H, W, C_):
    """x (B, H, W, C) float32 on the CPU.  The data sets cycle over the channels (period 5, so every set meets every lane of a
    16-, 32- or 64-channel group): randn; halves (many ties); a constant map; randn with NaN, +inf and -inf scattered; halves
    with -inf on every second pixel -- and channel 4 all -inf."""
    g = torch.Generator().manual_seed(seed("spp", B, H, W, C_))
    x = torch.randn(B, H, W, C_, generator=g)
    halves = torch.round(x * 2) / 2
    mark = torch.rand(B, H, W, C_, generator=g)
    kind = torch.arange(C_) % 5
    x = torch.where(kind == 1, halves, x)
    x = torch.where(kind == 2, (torch.arange(C_) * 0.25 - 3.0).expand_as(x), x)
    special = torch.where(mark < 0.1, torch.full_like(x, NAN), torch.where(mark < 0.2, torch.full_like(x, math.inf),
                          torch.where(mark < 0.3, torch.full_like(x, -math.inf), x)))
    x = torch.where(kind == 3, special, x)
    x = torch.where(kind == 4, torch.where(mark < 0.5, torch.full_like(x, -math.inf), halves), x)
    x[..., 4] = -math.inf
    return x.contiguous()


def spp_forward_reference(x):
    """(out (B, H, W, 4C) float64, argmax (B, H, W, 3, C) int64) of max_pool2d on the CPU in float64, NCHW-contiguous"""
    x64 = x.double().permute(0, 3, 1, 2).contiguous()
    outs, args = [x.double()], []
    for k in (5, 9, 13):
        v, i = torch.nn.functional.max_pool2d(x64, k, 1, k // 2, return_indices=True)
        outs.append(v.permute(0, 2, 3, 1))
        args.append(i.permute(0, 2, 3, 1))
    return torch.cat(outs, -1).contiguous(), torch.stack(args, 3).contiguous()


def spp_case_data(shape):
    """the input and its forward reference, computed once per case and shared by the forward and the backward tests (read-only)"""
    if shape not in _SPP_CACHE:
        x = spp_input(*shape)
        _SPP_CACHE[shape] = (x,) + spp_forward_reference(x)
    return _SPP_CACHE[shape]


def spp_backward_reference(g, arg, H, W):
    """dx (B, H W, C) float64 and the same of |g|: the identity branch plus every pooled gradient scattered to its arg-max pixel.
    Like the kernel's gather, an output counts only for a pixel inside its own window (true of every real arg-max; a hand-made
    one may point elsewhere)."""
    B, C_ = g.shape[0], g.shape[-1] // 4
    HW = H * W
    a = arg.reshape(B, HW, 3, C_).long()
    q = torch.arange(HW).view(1, HW, 1)
    res = []
    for gg in (g.double().reshape(B, HW, 4, C_), g.double().abs().reshape(B, HW, 4, C_)):
        dx = gg[:, :, 0, :].clone()
        for ki, r in enumerate((2, 4, 6)):
            idx = a[:, :, ki, :]
            inside = ((idx // W - q // W).abs() <= r) & ((idx % W - q % W).abs() <= r) & (idx < HW)
            dx.scatter_add_(1, idx.clamp(max=HW - 1), torch.where(inside, gg[:, :, ki + 1, :], torch.zeros((), dtype=torch.float64)))
        res.append(dx)
    return res


def same(a, b):
    """equal, NaN positions equal"""
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def run_spp_fwd(x, fill):
    L, lib = _lib()
    B, H, W, C_ = x.shape
    out = Guarded(B * H * W * 4 * C_, fill=fill, guard_fill=NAN)
    arg = Guarded(B * H * W * 3 * C_, fill=ARG_FILL, dtype=torch.int16)
    rc = lib.frlw_spp_train_fwd(ptr(x), B, H, W, C_, ptr(out.t), ptr(arg.t), None)
    assert rc == L.FRLW_OK, f"frlw_spp_train_fwd -> {rc}"
    torch.cuda.synchronize()
    assert out.guard_intact(), "out: written past the end"
    assert arg.guard_intact(), "argmax: written past the end (the rows of a group's invalid channels)"
    return out.t.view(B, H, W, 4 * C_), arg.t.view(B, H, W, 3, C_)


def run_spp_bwd(g, arg, B, H, W, C_):
    L, lib = _lib()
    dx = Guarded(B * H * W * C_)
    rc = lib.frlw_spp_train_bwd(ptr(g), ptr(arg), B, H, W, C_, ptr(dx.t), None)
    assert rc == L.FRLW_OK, f"frlw_spp_train_bwd -> {rc}"
    torch.cuda.synchronize()
    assert dx.guard_intact(), "dx: written past the end"
    bad = ~torch.isfinite(dx.t)
    assert not bad.any(), f"dx: {int(bad.sum())} of {dx.n} elements not finite"
    return dx.t.view(B, H * W, C_)


@pytest.mark.parametrize("case", SPP_CASES, ids=SPP_IDS)
def test_spp_forward_equals_max_pool2d(case):
    shape, ch = case
    assert spp_plan(*shape)[0] == ch
    x, ref_out, ref_arg = spp_case_data(shape)
    xd = x.to(DEV)
    for fill in (NAN, 12345.0):
        out, arg = run_spp_fwd(xd, fill)
        assert same(out.cpu().double(), ref_out), f"out differs (fill {fill})"
        assert torch.equal(arg.cpu().long() & 0xFFFF, ref_arg), f"argmax differs (fill {fill})"


@pytest.mark.parametrize("case", SPP_CASES, ids=SPP_IDS)
def test_spp_backward_equals_the_scatter(case):
    """dout in {-3..3} over all 4 C channels: exact; randn dout: within 2 * 277 u absref.  The arg-max is the reference's (the
    forward test holds the kernel's to it), so the constant channels send every window's gradient to its first pixel."""
    shape, ch = case
    B, H, W, C_ = shape
    plan = spp_plan(*shape)
    assert plan[0] == ch and plan[2] == 3 * H * W * ch * 6
    _, _, ref_arg = spp_case_data(shape)
    arg = ref_arg.to(torch.int16).to(DEV)
    gen = torch.Generator().manual_seed(seed("spp dout", shape))
    g = torch.randint(-3, 4, (B, H, W, 4 * C_), generator=gen).float()
    dx = run_spp_bwd(g.to(DEV), arg, B, H, W, C_)
    ref, absref = spp_backward_reference(g, ref_arg, H, W)
    assert float(absref.max()) <= 3 * (1 + 25 + 81 + 169)
    assert torch.equal(dx.cpu().double(), ref), f"{int((dx.cpu().double() != ref).sum())} elements differ from float64"
    g = torch.randn(B, H, W, 4 * C_, generator=gen)
    dx = run_spp_bwd(g.to(DEV), arg, B, H, W, C_)
    ref, absref = spp_backward_reference(g, ref_arg, H, W)
    r = (dx.cpu().double() - ref).abs() / (2 * 277 * U * absref).clamp_min(1e-300)
    WORST["spp dx"] = max(WORST.get("spp dx", 0.0), float(r.max()))
    assert float(r.max()) <= 1.0, f"worst |err| / bound {float(r.max()):.3g}"
    _SPP_CACHE.pop(shape, None)  # the last user: the large cases' float64 references are not kept for the rest of the session


@pytest.mark.parametrize("shape", [(3, 3, 4, 24), (2, 8, 10, 256), (512, 2, 3, 72)], ids=["3x3x4x24", "2x8x10x256", "512x2x3x72"])
def test_spp_backward_hand_made_argmax(shape):
    """Every arg-max entry points at pixel 0: pixel 0 gathers the outputs whose window holds it (9 + 25 + 49 at most), every other
    pixel keeps the identity branch alone."""
    B, H, W, C_ = shape
    arg = torch.zeros(B, H, W, 3, C_, dtype=torch.int16)
    g = torch.randint(-3, 4, (B, H, W, 4 * C_), generator=torch.Generator().manual_seed(seed("spp zero", shape))).float()
    dx = run_spp_bwd(g.to(DEV), arg.to(DEV), B, H, W, C_).cpu().double()
    ref, _ = spp_backward_reference(g, arg, H, W)
    assert torch.equal(dx, ref)
    assert torch.equal(dx[:, 1:], g.double().reshape(B, H * W, 4, C_)[:, 1:, 0])
    # pixel 0 without the scatter: windows of radius 2, 4, 6 around each output q hold pixel 0 when q lies in [0, r] x [0, r]
    want0 = g.double().reshape(B, H, W, 4, C_)[:, 0, 0, 0].clone()
    for ki, r in enumerate((2, 4, 6)):
        want0 += g.double().reshape(B, H, W, 4, C_)[:, :r + 1, :r + 1, ki + 1].sum((1, 2))
    assert torch.equal(dx[:, 0], want0)


def literal_pools(x):
    """cat[x, maxpool5, maxpool9, maxpool13] and the arg-max of one (H, W) map as nested lists, by a literal loop with the rule
    `v > best or v is NaN`, starting from the window's first element"""
    H, W = len(x), len(x[0])
    out, arg = [], []
    for r in (2, 4, 6):
        o, a = [[None] * W for _ in range(H)], [[None] * W for _ in range(H)]
        for y in range(H):
            for xx in range(W):
                best, at = -math.inf, None
                for yy in range(max(0, y - r), min(H - 1, y + r) + 1):
                    for xc in range(max(0, xx - r), min(W - 1, xx + r) + 1):
                        v = x[yy][xc]
                        if at is None or v > best or v != v:
                            best, at = v, yy * W + xc
                o[y][xx], a[y][xx] = best, at
        out.append(o)
        arg.append(a)
    return out, arg


def test_spp_rules_on_one_3x4_map_by_a_literal_loop():
    """Ties (the first maximum wins), NaN (the last NaN of the window wins), an all -inf map (the window's first element) and
    +inf twice on hand-made 3 x 4 maps: the literal loop, max_pool2d in float64 and the kernel agree exactly."""
    inf = math.inf
    maps = [
        [[1.0, 2.0, 2.0, 1.0], [2.0, 0.5, 2.0, 2.0], [1.0, 2.0, 1.0, 2.0]],            # ties
        [[0.0, NAN, 3.0, 1.0], [5.0, 1.0, NAN, 2.0], [1.0, 2.0, 7.0, NAN]],            # three NaN
        [[-inf] * 4, [-inf] * 4, [-inf] * 4],                                          # all -inf
        [[1.0, inf, 0.0, -inf], [0.0, -inf, inf, 2.0], [-inf, 1.0, 0.0, 1.0]],         # +inf twice, -inf
        [[7.0] * 4, [7.0] * 4, [7.0] * 4],                                             # constant
        [[NAN, 1.0, 2.0, 3.0], [0.0, 0.0, 0.0, 0.0], [3.0, 2.0, 1.0, 9.0]],            # NaN in the corner only
    ]
    H, W, C_ = 3, 4, 16
    x = torch.zeros(1, H, W, C_)
    for c in range(C_):
        x[0, :, :, c] = torch.tensor(maps[c % len(maps)])
    ref_out, ref_arg = spp_forward_reference(x)
    out, arg = run_spp_fwd(x.to(DEV), NAN)
    out, arg = out.cpu().double(), arg.cpu().long() & 0xFFFF
    for c in range(C_):
        lo, la = literal_pools(maps[c % len(maps)])
        for ki in range(3):
            want_o, want_a = torch.tensor(lo[ki], dtype=torch.float64), torch.tensor(la[ki])
            assert same(ref_out[0, :, :, (ki + 1) * C_ + c], want_o) and torch.equal(ref_arg[0, :, :, ki, c], want_a), ("max_pool2d", c, ki)
            assert same(out[0, :, :, (ki + 1) * C_ + c], want_o) and torch.equal(arg[0, :, :, ki, c], want_a), ("kernel", c, ki)
        assert same(out[0, :, :, c], x[0, :, :, c].double())
    # the three rules, spelled out on pool 5 (radius 2)
    _, la = literal_pools(maps[0])
    assert la[0][0][0] == 1 and la[0][1][1] == 1          # the first 2.0 in row-major order, not a later one
    _, la = literal_pools(maps[1])
    assert la[0][0][0] == 6 and la[0][1][2] == 11         # the last NaN of the window
    _, la = literal_pools(maps[2])
    assert la[0][0][0] == 0 and la[0][2][3] == 1          # the window's first element: (0, 0); window rows 0-2, columns 1-3


# ================================================================================================================================
# coverage
# ================================================================================================================================

def test_tables_reach_every_form():
    """The plans named in the tables are the ones the library gives (host query), and together they reach every <CPL, NG>, every
    n_wg class and every channel width; C, nc and M of the prediction level each take every listed value."""
    assert all(pred_plan(*a) == p for a, p in PRED_CASES)
    assert {(p[0], p[1]) for _, p in PRED_CASES} == {(1, 1), (2, 1), (1, 2), (2, 2)}
    assert {n_wg_class(a[0], p[2]) for a, p in PRED_CASES} >= {1, 16, 17, "1024 uncapped", "1024 capped"}
    under_cap = {(p[0], p[1]) for a, p in PRED_CASES if n_wg_class(a[0], p[2]) == "1024 capped"}
    assert (2, 1) in under_cap
    assert {a[1] for a, _ in PRED_CASES} >= {4, 64, 252, 256, 260, 508, 512}
    assert {a[2] for a, _ in PRED_CASES} >= {1, 3, 4, 11}
    assert {a[0] for a, _ in PRED_CASES} == {1, 63, 64, 65, 1024, 1025, 65536, 81920, 65600}
    assert all(spp_plan(*s)[0] == ch for s, ch in SPP_CASES)
    assert {ch for _, ch in SPP_CASES} == {64, 32, 16}
    assert spp_plan(2, 16, 32, 40)[2] == 147456
    assert len(PRED_CASES) == len(set(PRED_IDS)) and len(SPP_CASES) == len(set(SPP_IDS))


def test_pred_spp_worst_ratio_report():
    if WORST:
        print("pred / SPP forms, worst |err| / bound:", {k: round(v, 4) for k, v in sorted(WORST.items())})
