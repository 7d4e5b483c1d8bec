"""Every BatchNorm + SiLU form of the train step (csrc/train_ops.hip: the statistics pass, k_bn_silu_fwd<false | true>,
k_bn_silu_bwd_partial / _apply<false | true>; the statistics the convolution epilogues leave, conv_mfma.h) against float64,
through the C ABI.  Each call asserts the exact set of frlw_bn_path_counts counters it moved (and, through the train forward,
of frlw_conv_path_counts); test_every_bn_form_has_a_case checks that the cases reach every counter.

The reference is float64 torch on the kernel's own float32 input z: F.batch_norm(training=True), SiLU, autograd for dz, dgamma,
dbeta -- no convolution error enters.  Every output is judged PER CHANNEL (a tensor-wide max-norm lets one channel hide).

Bounds, from float32 arithmetic (u = 2^-24; mean_c, std_c = sqrt(var_c + eps) of the reference; kappa_c = 1 + |mean_c| / std_c):
  mean     float64 sums rounded once: |d mean| <= 4 u (|mean| + std).  The epilogue's shifted float32 sums err by u per term
           of size std, the stored float32 by u |mean|.
  var      relative to var itself: |d var| <= 1e-4 var + 2^-40 mean^2.  The sums of squares are float64 (exact squares in the
           statistics pass; n k^2 + 2 k S + Q from shifted float32 sums S, Q of at most 128 rows in the epilogues: <= 128 u
           relative of the variance); the float64 subtraction costs 2^-53 kappa^2.  eps_c = the measured relative error of var
           (+ 2u) then carries into every normalised value below: invstd relative error <= eps_c / 2 + 2 u.
  zhat     z - mean rounds by u |z - mean| and the float32 mean is u |mean| off: d zhat <= 8 u (|zhat| + kappa) + (eps_c / 2 + 2 u)
           |zhat| -- the rounding torch's float32 BatchNorm pays too.
  y        u = gamma zhat + beta: d u <= |gamma| d zhat + 4 u |u|; silu' <= 1.1, and the hardware exp / reciprocal add 4e-6
           |y| (the detector epilogue's bound): d y <= 1.1 d u + 4e-6 |y| + 1e-30 (FTZ of denormal sigmoids past u < -87).
  du       = dy silu'(u): |silu''| <= 0.5, the hardware sigmoid costs 4e-6 |silu'| and 1 - s cancels to 2u |u| absolute:
           d du <= |dy| (0.5 |gamma| d zhat + 4e-6 |silu'| + 2 u (1 + |u|)).
  dbeta    = sum du (float32 groups of four rows into float64): <= sum (d du + 8 u |du|) + u |dbeta|;
  dgamma   = sum du zhat: <= sum (d du |zhat| + |du| d zhat + 8 u |du zhat|) + u |dgamma|.
  dz       = gamma invstd (du - m1 - zhat m2), m1 = mean du, m2 = mean du zhat: the terms' own magnitudes set the scale (they
           cancel when dy is mean-dominated): <= |gamma| invstd [d du + D1 + |zhat| D2 + |m2| d zhat + 8 u (|du| + |m1| + |zhat m2|)]
           + (eps_c / 2 + 2 u) |dz|, D1 / D2 = the channel's dbeta / dgamma bounds over M.
  running  r' = (1 - m) r + m x: <= 4 u (|r| + |x|) + m * (bound of x).
Negative controls: torch's CPU float32 BatchNorm on the same input meets every bound; a reference with var (1 + 1e-3), or with
one channel's beta moved, fails.
"""
import ctypes as C
import math
import zlib

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
EPS = 1e-5
TOL_VAR = 1e-4
NAN = float("nan")
WORST = {}  # quantity -> worst |err| / bound over the cases (printed by the coverage test)
# the frlw_bn_path_counts forms each kind of call must move, exactly (test_every_bn_form_has_a_case: together, all of them)
FORMS_DIRECT = ({"stats_pass"}, {"fwd"}, {"bwd"})            # frlw_bn_stats, frlw_bn_silu_fwd, frlw_bn_silu_bwd
FORMS_FUSED = ({"stats_epilogue", "fwd_fused"}, {"bwd"})     # train forward / backward with a residual and row strides
FORMS_PAIR = ({"stats_epilogue", "fwd_fused"}, {"bwd_pair"})  # a stacked pair


def _lib():
    from frlw_evd_amd import _lib as L
    return L, L.load()


def bn_counts():
    L, lib = _lib()
    n = len(L.BN_PATHS)
    c = (C.c_uint64 * n)()
    assert lib.frlw_bn_path_counts(c, n) == n
    return list(c)


def conv_counts():
    L, lib = _lib()
    n = len(L.CONV_PATHS)
    c = (C.c_uint64 * n)()
    assert lib.frlw_conv_path_counts(c, n) == n
    return list(c)


class Moved:
    """the BN (and convolution) forms the calls inside the block enqueued"""

    def __enter__(self):
        torch.cuda.synchronize()
        self.b, self.c = bn_counts(), conv_counts()
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        L, _ = _lib()
        self.bn = {L.BN_PATHS[i] for i, (a, b) in enumerate(zip(self.b, bn_counts())) if a != b}
        self.conv = {L.CONV_PATHS[i] for i, (a, b) in enumerate(zip(self.c, conv_counts())) if a != b}


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def ok(rc, what):
    L, _ = _lib()
    assert rc == L.FRLW_OK, f"{what} -> {rc}"


def nan(*shape):
    return torch.full(shape, NAN, device=DEV)


def seed(*key):
    return zlib.crc32(repr(key).encode())


# ---- data ------------------------------------------------------------------------------------------------------------------
# channel kinds, cycled over the channels of every tensor (so every kind meets every column position of a float4 and of a chunk)
KINDS = ("randn", "ratio10", "ratio100", "ratio1000", "const", "gamma0", "gamma50", "randn_dymean", "randn_dyzero")


def make_inputs(M, C_, g, kinds=KINDS):
    """z (M, C) float32, gamma, beta, dy per channel kind; returns (z, gamma, beta, dy, kind index per channel)."""
    kind = torch.arange(C_, device=DEV) % len(kinds)
    names = [kinds[int(i)] for i in kind.tolist()]
    base = torch.randn(M, C_, generator=g, device=DEV)
    offs = torch.randn(C_, generator=g, device=DEV).sign()
    center = torch.zeros(C_, device=DEV)
    scale = torch.ones(C_, device=DEV)
    gamma = torch.rand(C_, generator=g, device=DEV) + 0.5
    beta = torch.randn(C_, generator=g, device=DEV) * 0.2
    dy = torch.randn(M, C_, generator=g, device=DEV)
    for c, k in enumerate(names):
        if k.startswith("ratio"):
            r = float(k[5:])
            scale[c] = 0.37 if r != 1000 else 0.05  # (var >> eps: mean * invstd is the ratio)
            center[c] = offs[c] * r * float(scale[c])
        elif k == "const":
            scale[c], center[c] = 0.0, 3.7
        elif k == "gamma0":
            gamma[c] = 0.0
        elif k == "gamma50":
            gamma[c] = 50.0  # |u| reaches ~200: __expf overflows on one side, the sigmoid flushes on the other
    z = (base * scale + center).float()
    for c, k in enumerate(names):
        if k == "randn_dymean":
            dy[:, c] = dy[:, c] * 0.5 + 40.0
        elif k == "randn_dyzero":
            dy[:, c] = 0.0
    return z, gamma, beta, dy, names


# ---- reference and judgement ----------------------------------------------------------------------------------------------

def reference(z, gamma, beta, dy, var_scale=1.0, beta_delta=None):
    """float64 BatchNorm (training) + SiLU of z (M, C) and its backward.  var_scale / beta_delta: deliberately wrong references
    for the negative controls (explicit formula then)."""
    z64 = z.double().requires_grad_(True)
    g64 = gamma.double().requires_grad_(True)
    b64 = beta.double().clone()
    if beta_delta is not None:
        b64 = b64 + beta_delta.double()
    b64.requires_grad_(True)
    if var_scale == 1.0:
        pre = torch.nn.functional.batch_norm(z64, None, None, g64, b64, training=True, eps=EPS)
    else:
        mu = z64.mean(0)
        var = ((z64 - mu) ** 2).mean(0) * var_scale
        pre = (z64 - mu) / torch.sqrt(var + EPS) * g64 + b64
    y = pre * torch.sigmoid(pre)
    y.backward(dy.double())
    with torch.no_grad():
        zd = z.double()
        mean = zd.mean(0)
        var = ((zd - mean) ** 2).mean(0) * var_scale
        invstd = 1.0 / torch.sqrt(var + EPS)
        zhat = (zd - mean) * invstd
        u = g64.detach() * zhat + b64.detach()
        s = torch.sigmoid(u)
        dsilu = s * (1 + u * (1 - s))
        du = dy.double() * dsilu
    return dict(mean=mean, var=var, invstd=invstd, y=y.detach(), dz=z64.grad, dgamma=g64.grad, dbeta=b64.grad,
                zhat=zhat, u=u, du=du, dsilu=dsilu, gamma=gamma.double(), dy=dy.double())


def _ratio(what, err, bound, fails, c_names=None, record=True):
    r = err / bound.clamp_min(1e-300)
    r = torch.where(torch.isnan(err), torch.full_like(r, math.inf), r)
    worst = float(r.max()) if r.numel() else 0.0
    if record:
        WORST[what] = max(WORST.get(what, 0.0), worst if math.isfinite(worst) else 0.0)
    if not worst <= 1.0:
        c = int(r.reshape(-1, r.shape[-1]).max(0).values.argmax()) if r.dim() else 0
        fails.append(f"{what}: worst |err| / bound {worst:.3g} (channel {c}{', ' + c_names[c] if c_names else ''})")


def judge(ref, got, names=None, fields=None, running=None, y_slack=0.0, record=True):
    """Per-channel judgement of the kernel outputs in `got` (any of mean, var, invstd, y, dz, dgamma, dbeta) against `ref`
    with the bounds of the module docstring.  Returns the list of failures (empty: all within bounds)."""
    fails = []
    fields = fields or list(got)
    mean, var, invstd = ref["mean"], ref["var"], ref["invstd"]
    std = 1.0 / invstd
    kappa = 1.0 + mean.abs() / std
    for f in ("mean", "var", "invstd", "y", "dz", "dgamma", "dbeta"):
        if f in got and not torch.isfinite(got[f]).all():
            fails.append(f"{f}: {int((~torch.isfinite(got[f])).sum())} values not finite")
    if fails:
        return fails
    # the relative variance error that the normalised values inherit: measured when the kernel's var is at hand
    if "var" in got:
        eps_c = (got["var"].double() - var).abs() / (var + EPS) + 2 * U
    else:
        eps_c = torch.full_like(var, 4 * U)  # mean / invstd handed over as float32 roundings of the reference
    if "mean" in fields:
        _ratio("mean", (got["mean"].double() - mean).abs(), 4 * U * (mean.abs() + std), fails, names, record)
    if "var" in fields:
        _ratio("var", (got["var"].double() - var).abs(), TOL_VAR * var + 2.0 ** -40 * mean * mean + 1e-300, fails, names, record)
    if "invstd" in fields:
        _ratio("invstd", (got["invstd"].double() - invstd).abs(), (TOL_VAR / 2 + 4 * U) * invstd, fails, names, record)
    zhat, u, du, gam = ref["zhat"], ref["u"], ref["du"], ref["gamma"].abs()
    dzhat = 8 * U * (zhat.abs() + kappa) + (eps_c / 2 + 2 * U) * zhat.abs()
    if "y" in fields:
        d_u = gam * dzhat + 4 * U * u.abs()
        _ratio("y", (got["y"].double() - ref["y"]).abs(), 1.1 * d_u + 4e-6 * ref["y"].abs() + 1e-30 + y_slack, fails, names, record)
    if any(f in fields for f in ("dz", "dgamma", "dbeta")):
        ddu = ref["dy"].abs() * (0.5 * gam * dzhat + 4e-6 * ref["dsilu"].abs() + 2 * U * (1 + u.abs()))
        b_dbeta = (ddu + 8 * U * du.abs()).sum(0) + U * ref["dbeta"].abs()
        b_dgamma = (ddu * zhat.abs() + du.abs() * dzhat + 8 * U * (du * zhat).abs()).sum(0) + U * ref["dgamma"].abs()
        if "dbeta" in fields:
            _ratio("dbeta", (got["dbeta"].double() - ref["dbeta"]).abs(), b_dbeta + 1e-30, fails, names, record)
        if "dgamma" in fields:
            _ratio("dgamma", (got["dgamma"].double() - ref["dgamma"]).abs(), b_dgamma + 1e-30, fails, names, record)
        if "dz" in fields:
            M = du.shape[0]
            m1, m2 = du.mean(0), (du * zhat).mean(0)
            b = gam * invstd * (ddu + b_dbeta / M + zhat.abs() * b_dgamma / M + m2.abs() * dzhat
                                + 8 * U * (du.abs() + m1.abs() + (zhat * m2).abs())) + (eps_c / 2 + 2 * U) * ref["dz"].abs()
            _ratio("dz", (got["dz"].double() - ref["dz"]).abs(), b + 1e-30, fails, names, record)
    if running is not None:  # (rm0, rv0, momentum, M, got_rm, got_rv)
        rm0, rv0, mom, M, grm, grv = running
        want_m = (1 - mom) * rm0.double() + mom * mean
        unb = var * M / (M - 1)
        want_v = (1 - mom) * rv0.double() + mom * unb
        _ratio("running_mean", (grm.double() - want_m).abs(), 4 * U * (rm0.double().abs() + mean.abs()) + mom * 4 * U * (mean.abs() + std), fails, None, record)
        _ratio("running_var", (grv.double() - want_v).abs(), 4 * U * (rv0.double().abs() + unb) + mom * (TOL_VAR * unb + 2.0 ** -40 * mean * mean), fails, None, record)
    return fails


def assert_ok(fails, what):
    assert not fails, f"{what}: " + "; ".join(fails)


# ---- the per-operator ABI ------------------------------------------------------------------------------------------------

def run_stats(z, M, C_):
    _, lib = _lib()
    mean, var, invstd = nan(C_), nan(C_), nan(C_)
    scratch = torch.full((lib.frlw_bn_scratch_doubles(M, C_),), NAN, dtype=torch.float64, device=DEV)
    with Moved() as mv:
        ok(lib.frlw_bn_stats(ptr(z), M, C_, C.c_float(EPS), ptr(mean), ptr(var), ptr(invstd), ptr(scratch), None), "frlw_bn_stats")
    assert mv.bn == FORMS_DIRECT[0] and mv.conv == set(), (mv.bn, mv.conv)
    return mean, var, invstd


def run_fwd(z, M, C_, gamma, beta, mean, invstd):
    _, lib = _lib()
    y = nan(M, C_)
    with Moved() as mv:
        ok(lib.frlw_bn_silu_fwd(ptr(z), M, C_, ptr(gamma), ptr(beta), ptr(mean), ptr(invstd), ptr(y), None), "frlw_bn_silu_fwd")
    assert mv.bn == FORMS_DIRECT[1], mv.bn
    return y


def run_bwd(dy, dy_rs, z, M, C_, gamma, beta, mean, invstd):
    _, lib = _lib()
    dz, dgamma, dbeta = nan(M, C_), nan(C_), nan(C_)
    scratch = torch.full((lib.frlw_bn_scratch_doubles(M, C_),), NAN, dtype=torch.float64, device=DEV)
    sums = nan(2 * C_)
    with Moved() as mv:
        ok(lib.frlw_bn_silu_bwd(ptr(dy), dy_rs, ptr(z), M, C_, ptr(gamma), ptr(beta), ptr(mean), ptr(invstd), ptr(dz), ptr(dgamma),
                                ptr(dbeta), ptr(scratch), ptr(sums), None), "frlw_bn_silu_bwd")
    assert mv.bn == FORMS_DIRECT[2], mv.bn
    return dz, dgamma, dbeta


# (M, C): row-lane counts that do not divide 256 (C 12, 20), second / third column chunks of bn_reduce_rows (1028, 2056),
# bn_rows_per_wg's clamps (32 rows up to M 32768, 512 from 512 K rows), more than 256 partial rows (the four-rows loop of
# bn_sum_partials: 32 K rows -> 1024 workgroups, 512 K + 1 -> 1025), M C / 4 beyond the 4096 x 256 grid (grid-stride loops
# go round: 512 K + 1 rows x 12, 64 x 80 x 64 x 256), and M = 1, 2, 33.
DIRECT = [(1, 4), (2, 12), (33, 20), (1023, 256), (1023, 1028), (33, 2056), (2, 2056), (32 * 1024, 1024), (512 * 1024 + 1, 12),
          (64 * 80 * 64, 256), (1023, 4)]


@pytest.mark.parametrize("M,C_", DIRECT, ids=[f"M{m}_C{c}" for m, c in DIRECT])
def test_direct_abi(M, C_):
    g = torch.Generator(device=DEV).manual_seed(seed("direct", M, C_))
    z, gamma, beta, dy, names = make_inputs(M, C_, g)
    mean, var, invstd = run_stats(z, M, C_)
    y = run_fwd(z, M, C_, gamma, beta, mean, invstd)
    # dy as a channel slice of a wider buffer (row stride C + 8) with NaN canaries in the gaps
    wide = torch.full((M, C_ + 8), NAN, device=DEV)
    wide[:, 4:4 + C_] = dy
    dz, dgamma, dbeta = run_bwd(wide[:, 4:], C_ + 8, z, M, C_, gamma, beta, mean, invstd)
    assert torch.isnan(wide[:, :4]).all() and torch.isnan(wide[:, 4 + C_:]).all(), "dy canaries overwritten"
    if M == 1:  # no torch reference (nn.BatchNorm2d refuses M = 1 in training): what the header promises
        assert (var == 0).all() and torch.equal(mean, z[0])
        assert torch.allclose(invstd.double(), torch.full_like(invstd.double(), EPS ** -0.5), rtol=4 * U)
        assert torch.allclose(y[0].double(), torch.nn.functional.silu(beta.double()), rtol=1e-5, atol=1e-30)
        assert (dz == 0).all() and torch.isfinite(dgamma).all() and torch.isfinite(dbeta).all()
        return
    ref = reference(z, gamma, beta, dy)
    assert_ok(judge(ref, dict(mean=mean, var=var, invstd=invstd, y=y), names), f"forward M={M} C={C_}")
    assert_ok(judge(ref, dict(dz=dz, dgamma=dgamma, dbeta=dbeta, var=var), names, fields=["dz", "dgamma", "dbeta"]),
              f"backward M={M} C={C_}")
    # the special channels, exactly
    const = [c for c, k in enumerate(names) if k == "const"]
    if const:  # (dz is not 0 there: gamma invstd (du - mean du) with invstd = eps^-1/2 -- judged above)
        assert torch.equal(mean[const], z[0, const]) and (var[const] <= 2.0 ** -40 * mean[const] ** 2).all()
        assert torch.allclose(y[:, const].double(), torch.nn.functional.silu(beta[const].double()).expand(M, -1), rtol=1e-5)
    zero_dy = [c for c, k in enumerate(names) if k == "randn_dyzero"]
    if zero_dy:
        assert (dz[:, zero_dy] == 0).all() and (dgamma[zero_dy] == 0).all() and (dbeta[zero_dy] == 0).all()
    g0 = [c for c, k in enumerate(names) if k == "gamma0"]
    if g0:
        assert (dz[:, g0] == 0).all()


def test_negative_controls():
    """torch's CPU float32 BatchNorm meets every bound; the kernels against a reference with var (1 + 1e-3), or with one channel's
    beta moved by 1e-3, fail.  (No constant channel here: torch's CPU float32 BatchNorm sums the mean in float32, 81 u |mean|
    off on a constant channel of 4099 rows, where std = sqrt(eps) makes kappa ~ 1000 -- the kernels sum in float64 and are held
    to the tighter bound on such channels in test_direct_abi.)"""
    M, C_ = 4099, 32
    g = torch.Generator(device=DEV).manual_seed(77)
    z, gamma, beta, dy, names = make_inputs(M, C_, g, kinds=tuple(k for k in KINDS if k != "const"))
    ref = reference(z, gamma, beta, dy)
    # torch float32 on the CPU
    zc = z.cpu().requires_grad_(True)
    gc, bc = gamma.cpu().requires_grad_(True), beta.cpu().requires_grad_(True)
    pre = torch.nn.functional.batch_norm(zc, None, None, gc, bc, training=True, eps=EPS)
    yc = torch.nn.functional.silu(pre)
    yc.backward(dy.cpu())
    var_c, mean_c = torch.var_mean(z.cpu(), 0, unbiased=False)
    tch = dict(mean=mean_c, var=var_c, invstd=1.0 / torch.sqrt(var_c + EPS), y=yc.detach(), dz=zc.grad, dgamma=gc.grad, dbeta=bc.grad)
    tch = {k: v.to(DEV) for k, v in tch.items()}
    assert_ok(judge(ref, tch, names), "torch float32 (CPU)")
    # the kernels
    mean, var, invstd = run_stats(z, M, C_)
    y = run_fwd(z, M, C_, gamma, beta, mean, invstd)
    dz, dgamma, dbeta = run_bwd(dy, 0, z, M, C_, gamma, beta, mean, invstd)
    got = dict(mean=mean, var=var, invstd=invstd, y=y, dz=dz, dgamma=dgamma, dbeta=dbeta)
    assert_ok(judge(ref, got, names), "kernels")
    wrong_var = judge(reference(z, gamma, beta, dy, var_scale=1.0 + 1e-3), got, names, record=False)
    assert any(f.startswith("var") for f in wrong_var) and any(f.startswith("invstd") for f in wrong_var), wrong_var
    delta = torch.zeros(C_, device=DEV)
    delta[0] = 1e-3  # a randn channel
    wrong_beta = judge(reference(z, gamma, beta, dy, beta_delta=delta), got, names, fields=["y", "dz", "dgamma", "dbeta"], record=False)
    assert any(f.startswith("y") and "channel 0" in f for f in wrong_beta), wrong_beta


def test_argument_rejection():
    """FRLW_ERR_ARG, nothing launched and nothing written: C % 4, C < 4, M < 1, y / dy off by 4 bytes, dy_row_stride < C."""
    L, lib = _lib()
    M, C_ = 64, 16
    g = torch.Generator(device=DEV).manual_seed(3)
    z, gamma, beta, dy, _ = make_inputs(M, C_, g)
    buf = nan(M * C_ + 8)
    outs = [nan(C_) for _ in range(3)]
    sc = torch.full((lib.frlw_bn_scratch_doubles(M, C_) + 64,), NAN, dtype=torch.float64, device=DEV)
    sums = nan(2 * C_)
    mean, invstd = z.mean(0), torch.ones(C_, device=DEV)
    dyb = torch.zeros(M * C_ + 8, device=DEV)
    dyb[:M * C_] = dy.reshape(-1)

    def stats(Mx, Cx):
        return lib.frlw_bn_stats(ptr(z), Mx, Cx, C.c_float(EPS), ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), ptr(sc), None)

    def fwd(Mx, Cx, off=0):
        return lib.frlw_bn_silu_fwd(ptr(z), Mx, Cx, ptr(gamma), ptr(beta), ptr(mean), ptr(invstd), C.c_void_p(buf.data_ptr() + off), None)

    def bwd(Mx, Cx, rs=0, off=0):
        return lib.frlw_bn_silu_bwd(C.c_void_p(dyb.data_ptr() + off), rs, ptr(z), Mx, Cx, ptr(gamma), ptr(beta), ptr(mean), ptr(invstd),
                                    ptr(buf), ptr(outs[0]), ptr(outs[1]), ptr(sc), ptr(sums), None)
    with Moved() as mv:
        for Mx, Cx in ((M, 14), (M, 2), (M, 0), (0, C_), (-1, C_)):
            assert stats(Mx, Cx) == L.FRLW_ERR_ARG, (Mx, Cx)
            assert fwd(Mx, Cx) == L.FRLW_ERR_ARG, (Mx, Cx)
            assert bwd(Mx, Cx) == L.FRLW_ERR_ARG, (Mx, Cx)
        assert fwd(M, C_, off=4) == L.FRLW_ERR_ARG
        assert bwd(M, C_, off=4) == L.FRLW_ERR_ARG
        assert bwd(M, C_, rs=C_ - 4) == L.FRLW_ERR_ARG
        assert bwd(M, C_, rs=C_ + 2) == L.FRLW_ERR_ARG  # not a multiple of 4
    assert mv.bn == set() and mv.conv == set(), (mv.bn, mv.conv)
    assert all(torch.isnan(t).all() for t in outs + [buf, sums]) and torch.isnan(sc).all(), "a rejected call wrote"


# ---- the train forward / backward: the statistics producers and the fused forms -----------------------------------------------

def conv_case(B, Cin, H, W, Cout, k, s, g, ratio):
    """x = 1 + sx randn, w = 100 (a_c + small noise) on the centre tap only (the other taps zero: no border effect), so that
    mean(z) / std(z) ~ sqrt(Cin) / sx = `ratio` on the channels with a_c != 0 (every third channel is zero-mean); |mean(z)| ~ 100
    keeps var(z) far above eps, so that mean * invstd reaches the ratio too."""
    sx = math.sqrt(Cin) / ratio
    x = 1.0 + sx * torch.randn(B, H, W, Cin, generator=g, device=DEV)
    w = torch.zeros(Cout, Cin, k, k, device=DEV)
    a = (torch.rand(Cout, 1, generator=g, device=DEV) + 0.5) / Cin * torch.randn(Cout, 1, generator=g, device=DEV).sign()
    a[::3] = 0.0
    noise = torch.randn(Cout, Cin, generator=g, device=DEV)
    noise[1::3] *= 1e-4 / Cin  # mean / std = ratio
    noise[2::3] *= 1e-2 / Cin
    noise[::3] *= 1.0 / math.sqrt(Cin)  # zero-mean weights: mean / std ~ |randn| / sx
    w[:, :, k // 2, k // 2] = 100.0 * (a + noise)
    return x.contiguous(), w.contiguous()


def train_fwd(x, w, gamma, beta, s, prec, Cout, fuse=None, y=None, running=None, tracked=None):
    """frlw_baseconv_train_fwd; Cout = both blocks' channels of a stacked pair"""
    _, lib = _lib()
    B, H, W_, Cin = x.shape
    k = w.shape[-1]
    pad = (k - 1) // 2
    Ho, Wo = (H + 2 * pad - k) // s + 1, (W_ + 2 * pad - k) // s + 1
    nbytes = lib.frlw_baseconv_train_scratch_bytes(B, H, W_, Cin, Cout, k, s)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    cnt = torch.zeros(1024, dtype=torch.int32, device=DEV)
    z, mean, var, invstd = nan(B, Ho, Wo, Cout), nan(Cout), nan(Cout), nan(Cout)
    if y is None:
        y = nan(B, Ho, Wo, Cout)
    rm, rv = running if running is not None else (None, None)
    with Moved() as mv:
        ok(lib.frlw_baseconv_train_fwd(ptr(x), ptr(w), ptr(gamma), ptr(beta), C.c_float(EPS), B, H, W_, Cin, Cout, k, s, ptr(z), ptr(y),
                                       ptr(mean), ptr(var), ptr(invstd), ptr(rm), ptr(rv), C.c_float(0.1), ptr(tracked), None,
                                       ptr(scratch), nbytes, ptr(cnt), C.byref(fuse) if fuse is not None else None, prec, None), "train_fwd")
    assert int(cnt.abs().sum()) == 0
    return dict(z=z, y=y, mean=mean, var=var, invstd=invstd, scratch=scratch, nbytes=nbytes, cnt=cnt), mv


def train_bwd(dy, dy_rs, x, w, gamma, beta, f, s, prec, fuse=None):
    _, lib = _lib()
    B, H, W_, Cin = x.shape
    z = f["z"]
    Cout, k = z.shape[-1], w.shape[-1]
    Ho, Wo = z.shape[1], z.shape[2]
    dz, dx, dw, dgamma, dbeta = nan(B, Ho, Wo, Cout), nan(B, H, W_, Cin), nan(Cout, Cin, k, k), nan(Cout), nan(Cout)
    with Moved() as mv:
        ok(lib.frlw_baseconv_train_bwd(ptr(dy), dy_rs, ptr(x), ptr(z), ptr(w), ptr(gamma), ptr(beta), ptr(f["mean"]), ptr(f["invstd"]),
                                       B, H, W_, Cin, Cout, k, s, ptr(dz), ptr(dx), ptr(dw), ptr(dgamma), ptr(dbeta), None,
                                       ptr(f["scratch"]), f["nbytes"], ptr(f["cnt"]), C.byref(fuse) if fuse is not None else None,
                                       prec, None), "train_bwd")
    return dict(dz=dz, dgamma=dgamma, dbeta=dbeta), mv


PRODUCERS = [  # (name, (B, Cin, H, W, Cout, k, stride), precision, convolution forms, statistics producer)
    ("epilogue 128x32", (2, 64, 32, 40, 32, 3, 1), 0, {"128x32"}, "stats_epilogue"),
    ("epilogue 64x64", (2, 16, 32, 40, 64, 3, 1), 0, {"64x64"}, "stats_epilogue"),
    ("epilogue 128x128 2x2", (2, 16, 256, 320, 128, 1, 1), 0, {"128x128_2x2"}, "stats_epilogue"),
    ("epilogue 64x128", (2, 64, 128, 160, 256, 3, 1), 0, {"64x128"}, "stats_epilogue"),
    ("epilogue 128x128 4x1", (2, 64, 128, 160, 256, 3, 1), 1, {"128x128_4x1"}, "stats_epilogue"),
    ("epilogue 64x64, M not a multiple of 64", (1, 16, 15, 13, 64, 3, 1), 0, {"64x64"}, "stats_epilogue"),
    ("epilogue 128x32, M not a multiple of 128", (1, 16, 15, 13, 32, 3, 1), 0, {"128x32"}, "stats_epilogue"),
    ("in-kernel split-K", (2, 512, 8, 10, 256, 1, 1), 0, {"split_inkernel_stats"}, "stats_split_inkernel"),
    ("in-kernel split-K, M not a multiple of 64", (1, 512, 9, 7, 128, 1, 1), 0, {"split_inkernel_stats"}, "stats_split_inkernel"),
    ("statistics pass (bf16x3 split_vec)", (2, 512, 8, 10, 256, 1, 1), 1, {"split_vec"}, "stats_pass"),
]


def Fuse(**kw):
    L, _ = _lib()
    return L.FrlwBaseconvFuse(**kw)


@pytest.mark.parametrize("ratio", [10, 1000])
@pytest.mark.parametrize("case", PRODUCERS, ids=[c[0] for c in PRODUCERS])
def test_statistics_producers(case, ratio):
    """Each producer of the per-channel sums (the unsplit vector epilogue, the in-kernel split-K last arriver, the separate pass)
    on mean-dominated outputs, judged against float64 statistics of the z the call returned; then the backward of the block."""
    name, (B, Cin, H, W, Cout, k, s), prec, cforms, producer = case
    g = torch.Generator(device=DEV).manual_seed(seed(name, ratio))
    x, w = conv_case(B, Cin, H, W, Cout, k, s, g, ratio)
    gamma = torch.rand(Cout, generator=g, device=DEV) + 0.5
    beta = torch.randn(Cout, generator=g, device=DEV) * 0.2
    rm0, rv0 = torch.randn(Cout, generator=g, device=DEV), torch.rand(Cout, generator=g, device=DEV) + 0.5
    rm, rv = rm0.clone(), rv0.clone()
    tracked = torch.tensor([5], dtype=torch.int64, device=DEV)
    f, mv = train_fwd(x, w, gamma, beta, s, prec, Cout, running=(rm, rv), tracked=tracked)
    assert mv.conv == cforms and mv.bn == {producer} | FORMS_DIRECT[1], (mv.conv, mv.bn)
    assert int(tracked) == 6
    z = f["z"].reshape(-1, Cout)
    M = z.shape[0]
    dy = torch.randn(M, Cout, generator=g, device=DEV)
    ref = reference(z, gamma, beta, dy)
    kap = ref["mean"].abs() * ref["invstd"]  # (var >> eps: the same as mean / sqrt(var))
    assert float(kap.max()) >= 0.6 * ratio, f"the case is not mean-dominated: max mean/std {float(kap.max()):.1f}"
    assert_ok(judge(ref, dict(mean=f["mean"], var=f["var"], invstd=f["invstd"], y=f["y"].reshape(-1, Cout)),
                    running=(rm0, rv0, 0.1, M, rm, rv)), f"{name} forward")
    v_ratio = (f["var"].double() - ref["var"]).abs() / (TOL_VAR * ref["var"] + 2.0 ** -40 * ref["mean"] ** 2)
    key = f"var / bound, {producer}, mean/std {ratio}"
    WORST[key] = max(WORST.get(key, 0.0), float(v_ratio.max()))
    b, mvb = train_bwd(dy.reshape(f["z"].shape), 0, x, w, gamma, beta, f, s, prec)
    assert mvb.bn == FORMS_DIRECT[2], mvb.bn
    assert_ok(judge(ref, dict(dz=b["dz"].reshape(-1, Cout), dgamma=b["dgamma"], dbeta=b["dbeta"], var=f["var"]),
                    fields=["dz", "dgamma", "dbeta"]), f"{name} backward")


FUSED = (2, 16, 16, 20, 3, 1)  # B, Cin, H, W, k, stride: M = 640 (64 x 64 tile, K = 144: unsplit, epilogue statistics)


def _canaries_intact(buf, lo, hi, what):
    outside = torch.ones(buf.shape[-1], dtype=torch.bool, device=DEV)
    outside[lo:hi] = False
    assert torch.isnan(buf[..., outside]).all(), f"{what}: stores outside the channel slice"


def test_fused_residual_and_slice():
    """y = silu(bn(z)) + residual (residual rows 16 floats wider), written into a channel slice of a wider buffer
    (y_row_stride): k_bn_silu_fwd<true>; then the backward with dy read as a slice (dy_row_stride)."""
    B, Cin, H, W, k, s = FUSED
    Cout = 48
    g = torch.Generator(device=DEV).manual_seed(21)
    x, w = conv_case(B, Cin, H, W, Cout, k, s, g, 300)
    gamma = torch.rand(Cout, generator=g, device=DEV) + 0.5
    beta = torch.randn(Cout, generator=g, device=DEV) * 0.2
    resb = torch.full((B, H, W, Cout + 16), NAN, device=DEV)
    resb[..., 8:8 + Cout] = torch.randn(B, H, W, Cout, generator=g, device=DEV)
    yb = nan(B, H, W, Cout + 40)
    y = yb[..., 20:20 + Cout]
    fuse = Fuse(residual=resb[..., 8:].data_ptr(), residual_row_stride=Cout + 16, y_row_stride=Cout + 40)
    f, mv = train_fwd(x, w, gamma, beta, s, 0, Cout, fuse=fuse, y=y)
    assert mv.bn == FORMS_FUSED[0], mv.bn
    _canaries_intact(yb, 20, 20 + Cout, "y")
    z = f["z"].reshape(-1, Cout)
    M = z.shape[0]
    dyb = torch.full((B, H, W, Cout + 12), NAN, device=DEV)
    dyb[..., 4:4 + Cout] = torch.randn(B, H, W, Cout, generator=g, device=DEV)
    ref = reference(z, gamma, beta, dyb[..., 4:4 + Cout].reshape(-1, Cout))
    res = resb[..., 8:8 + Cout].reshape(-1, Cout).double()
    # y - residual (exact in float64) against silu(bn(z)), with the rounding of the one float32 addition on top of the y bound
    assert_ok(judge(ref, dict(mean=f["mean"], var=f["var"], invstd=f["invstd"], y=y.reshape(-1, Cout).double() - res),
                    y_slack=U * (ref["y"] + res).abs()), "fused forward")
    b, mvb = train_bwd(dyb[..., 4:], Cout + 12, x, w, gamma, beta, f, s, 0)
    assert mvb.bn == FORMS_FUSED[1], mvb.bn
    assert torch.isnan(dyb[..., :4]).all() and torch.isnan(dyb[..., 4 + Cout:]).all()
    assert_ok(judge(ref, dict(dz=b["dz"].reshape(-1, Cout), dgamma=b["dgamma"], dbeta=b["dbeta"], var=f["var"]),
                    fields=["dz", "dgamma", "dbeta"]), "fused backward")


def test_stacked_pair():
    """Two BaseConvs stacked along the channels (split): k_bn_silu_fwd<true> writes both blocks' y into slices of their own
    buffers, the statistics update both blocks' running buffers and counters, k_bn_silu_bwd_partial / _apply<true> read dy and
    dy2 from slices; every output per channel against float64, canaries around every slice."""
    B, Cin, H, W, k, s = FUSED
    c1, c2 = 24, 40
    Cout = c1 + c2
    g = torch.Generator(device=DEV).manual_seed(22)
    x, wall = conv_case(B, Cin, H, W, Cout, k, s, g, 1000)
    w1, w2 = wall[:c1].contiguous(), wall[c1:].contiguous()
    gamma = torch.rand(Cout, generator=g, device=DEV) + 0.5
    beta = torch.randn(Cout, generator=g, device=DEV) * 0.2
    g1, g2, b1, b2 = gamma[:c1].clone(), gamma[c1:].clone(), beta[:c1].clone(), beta[c1:].clone()
    rm0, rv0 = torch.randn(Cout, generator=g, device=DEV), torch.rand(Cout, generator=g, device=DEV) + 0.5
    rm1, rv1, rm2, rv2 = rm0[:c1].clone(), rv0[:c1].clone(), rm0[c1:].clone(), rv0[c1:].clone()
    t1, t2 = torch.tensor([0], dtype=torch.int64, device=DEV), torch.tensor([10], dtype=torch.int64, device=DEV)
    yb1, yb2 = nan(B, H, W, c1 + 8), nan(B, H, W, c2 + 24)
    y1, y2 = yb1[..., 4:4 + c1], yb2[..., 12:12 + c2]
    fuse = Fuse(split=c1, w2=w2.data_ptr(), gamma2=g2.data_ptr(), beta2=b2.data_ptr(), running_mean2=rm2.data_ptr(),
                running_var2=rv2.data_ptr(), num_batches_tracked2=t2.data_ptr(), y2=y2.data_ptr(), y2_row_stride=c2 + 24,
                y_row_stride=c1 + 8)
    f, mv = train_fwd(x, w1, g1, b1, s, 0, Cout, fuse=fuse, y=y1, running=(rm1, rv1), tracked=t1)
    assert mv.bn == FORMS_PAIR[0], mv.bn
    assert int(t1) == 1 and int(t2) == 11
    _canaries_intact(yb1, 4, 4 + c1, "y")
    _canaries_intact(yb2, 12, 12 + c2, "y2")
    z = f["z"].reshape(-1, Cout)
    M = z.shape[0]
    # (a row of NaN behind dy: reading the second block's channels from dy's rows, a bug this test must catch, stays in bounds)
    dyb1 = torch.full((B * H * W + 2, c1 + 4), NAN, device=DEV)[:-2].view(B, H, W, c1 + 4)
    dyb2 = torch.full((B, H, W, c2 + 8), NAN, device=DEV)
    dyb1[..., :c1] = torch.randn(B, H, W, c1, generator=g, device=DEV)
    dyb2[..., 8:] = torch.randn(B, H, W, c2, generator=g, device=DEV) + 3.0
    dy = torch.cat([dyb1[..., :c1], dyb2[..., 8:]], -1).reshape(-1, Cout)
    ref = reference(z, gamma, beta, dy)
    assert float((ref["mean"].abs() * ref["invstd"]).max()) >= 600
    y = torch.cat([y1, y2], -1).reshape(-1, Cout)
    assert_ok(judge(ref, dict(mean=f["mean"], var=f["var"], invstd=f["invstd"], y=y),
                    running=(rm0, rv0, 0.1, M, torch.cat([rm1, rm2]), torch.cat([rv1, rv2]))), "stacked forward")
    fuse.dy2, fuse.dy2_row_stride = dyb2[..., 8:].data_ptr(), c2 + 8
    b, mvb = train_bwd(dyb1, c1 + 4, x, w1, g1, b1, f, s, 0, fuse=fuse)
    assert mvb.bn == FORMS_PAIR[1], mvb.bn
    assert torch.isnan(dyb1[..., c1:]).all() and torch.isnan(dyb2[..., :8]).all()
    assert_ok(judge(ref, dict(dz=b["dz"].reshape(-1, Cout), dgamma=b["dgamma"], dbeta=b["dbeta"], var=f["var"]),
                    fields=["dz", "dgamma", "dbeta"]), "stacked backward")


def test_cumulative_average_module():
    """momentum None (the cumulative average, yolox/train_ops.py:_bn_cfg) through the Python module, two steps, against
    nn.BatchNorm2d in float64 -- running statistics and num_batches_tracked."""
    from frlw_evd_amd.yolox.network_blocks import BaseConv
    from frlw_evd_amd.yolox import train_ops
    torch.manual_seed(9)
    mine = BaseConv(32, 64, 3, 1, act="silu").cuda().train()
    mine.bn.momentum = None
    ref = BaseConv(32, 64, 3, 1, act="silu").cuda().train()
    ref.load_state_dict(mine.state_dict())
    ref.bn.momentum = None
    ref = ref.double()
    for step in range(2):
        x = (torch.randn(2, 32, 16, 20, device=DEV) + 2.0).contiguous(memory_format=torch.channels_last)
        ym = train_ops.base_conv_train(x, mine.conv, mine.bn)
        with torch.no_grad():
            z = torch.nn.functional.conv2d(x.double(), ref.conv.weight, padding=1)
            ref.bn(z)
        assert int(mine.bn.num_batches_tracked) == step + 1 == int(ref.bn.num_batches_tracked)
        M = z.numel() // z.shape[1]
        var = z.var((0, 2, 3), unbiased=False)
        # float32 products of the convolution (1e-5 of |x| (*) |w|) dominate; the statistics are judged elsewhere
        absz = torch.nn.functional.conv2d(x.double().abs(), ref.conv.weight.abs(), padding=1)
        tol_m = 1e-5 * absz.mean((0, 2, 3))
        assert ((mine.bn.running_mean.double() - ref.bn.running_mean).abs() <= tol_m + 4 * U * ref.bn.running_mean.abs()).all()
        tol_v = 2e-5 * (absz * absz).mean((0, 2, 3)) * M / (M - 1) + 4 * U * ref.bn.running_var
        assert ((mine.bn.running_var.double() - ref.bn.running_var).abs() <= tol_v).all()
        assert torch.isfinite(ym).all() and var.min() > 0


# ---- coverage ------------------------------------------------------------------------------------------------------------------

def test_every_bn_form_has_a_case():
    """Every FRLW_BN_PATH_* counter is the expected result of at least one case above (each case asserts its set exactly): a
    form added without a case fails."""
    L, _ = _lib()
    reached = set().union(*FORMS_DIRECT, *FORMS_FUSED, *FORMS_PAIR, *({c[-1]} for c in PRODUCERS))
    assert reached <= set(L.BN_PATHS), reached - set(L.BN_PATHS)
    assert set(L.BN_PATHS) <= reached, set(L.BN_PATHS) - reached
    if WORST:
        print("worst |err| / bound:", {k: round(v, 4) for k, v in sorted(WORST.items())})
