"""Dual TV-L1 optical flow (Zach, Pock, Bischof 2007) restated in numpy, statement by statement as DESIGN.md's motion section
specifies it, with the dtype as a parameter: float64 is the yardstick of the tests, float32 the same code in the arithmetic the
kernels of csrc/tvl1.hip use.  ``tvl1(i0, i1, dtype, **params)`` returns a dict: ``flow`` (H, W, 2), ``levels`` [(h, w), ...] from
the full frame down, ``iters`` (levels, warps) inner iterations run, ``errors`` (levels, warps) the last error of each warp and
``eps`` (levels,) the threshold it is compared with.

Every scalar is cast to the dtype before it meets an array, and sums of products are written left to right in the order the
kernels use, so the float32 run differs from the device only where the issue licenses it (the order of the error sum)."""
import numpy as np

DEFAULTS = dict(tau=0.25, lam=0.15, theta=0.3, nscales=5, warps=5, epsilon=0.01, inner=30, outer=10, scale_step=0.8, median=5)
A = -0.75   # Keys' cubic kernel


def plan(H, W, nscales=5, scale_step=0.8):
    """Level shapes from the full frame down; the first level with a side below 16 is dropped with all above it."""
    out = []
    h, w = int(H), int(W)
    for _ in range(int(nscales)):
        if h < 16 or w < 16:
            break
        out.append((h, w))
        h, w = int(round(h * scale_step)), int(round(w * scale_step))
    return out


def _axis(n_src, n_dst, dt):
    s = (np.arange(n_dst).astype(dt) + dt(0.5)) * (dt(n_src) / dt(n_dst)) - dt(0.5)
    i0 = np.floor(s)
    f = (s - i0).astype(dt)
    i0 = i0.astype(np.int64)
    return np.clip(i0, 0, n_src - 1), np.clip(i0 + 1, 0, n_src - 1), f


def resize(a, shape, dt):
    """Bilinear, half-pixel centres, neighbour indices clamped to the edge; along x first, then along y."""
    y0, y1, fy = _axis(a.shape[0], shape[0], dt)
    x0, x1, fx = _axis(a.shape[1], shape[1], dt)
    top = a[y0][:, x0] * (dt(1) - fx) + a[y0][:, x1] * fx
    bot = a[y1][:, x0] * (dt(1) - fx) + a[y1][:, x1] * fx
    return (top * (dt(1) - fy)[:, None] + bot * fy[:, None]).astype(dt)


def gradient(s, dt):
    gx, gy = np.empty_like(s), np.empty_like(s)
    gx[:, 1:-1] = dt(0.5) * (s[:, 2:] - s[:, :-2])
    gx[:, 0] = dt(0.5) * (s[:, 1] - s[:, 0])
    gx[:, -1] = dt(0.5) * (s[:, -1] - s[:, -2])
    gy[1:-1] = dt(0.5) * (s[2:] - s[:-2])
    gy[0] = dt(0.5) * (s[1] - s[0])
    gy[-1] = dt(0.5) * (s[-1] - s[-2])
    return gx, gy


def _cubic_weights(t, dt):
    a = dt(A)
    t1 = t + dt(1)
    w0 = ((a * t1 - dt(5) * a) * t1 + dt(8) * a) * t1 - dt(4) * a
    w1 = ((a + dt(2)) * t - (a + dt(3))) * (t * t) + dt(1)
    s = dt(1) - t
    w2 = ((a + dt(2)) * s - (a + dt(3))) * (s * s) + dt(1)
    w3 = dt(1) - w0 - w1 - w2
    return [w0, w1, w2, w3]


def bicubic(images, u1, u2, dt):
    """``images`` sampled at (x + u1, y + u2): taps floor - 1 .. floor + 2, a tap outside the image contributes 0; per tap row the
    four products are added left to right, then the four rows top to bottom."""
    h, w = u1.shape
    fx = np.arange(w).astype(dt)[None, :] + u1
    fy = np.arange(h).astype(dt)[:, None] + u2
    ix, iy = np.floor(fx), np.floor(fy)
    wx, wy = _cubic_weights((fx - ix).astype(dt), dt), _cubic_weights((fy - iy).astype(dt), dt)
    ix, iy = ix.astype(np.int64), iy.astype(np.int64)
    out = []
    for img in images:
        total = None
        for j in range(4):
            yy = iy + (j - 1)
            row = None
            for i in range(4):
                xx = ix + (i - 1)
                ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
                tap = np.where(ok, img[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)], dt(0))
                row = wx[i] * tap if row is None else row + wx[i] * tap
            total = wy[j] * row if total is None else total + wy[j] * row
        out.append(total.astype(dt))
    return out


def median5(u):
    """5 x 5 median with replicated border."""
    h, w = u.shape
    p = np.pad(u, 2, mode="edge")
    stack = np.stack([p[j:j + h, i:i + w] for j in range(5) for i in range(5)], axis=-1)
    return np.ascontiguousarray(np.partition(stack, 12, axis=-1)[..., 12])


def _divergence(a, b):
    """(a - a_left) + (b - b_up); the missing neighbour of the first column / row counts as 0."""
    out = a.copy()
    out[:, 1:] = a[:, 1:] - a[:, :-1]
    vert = b.copy()
    vert[1:] = b[1:] - b[:-1]
    return out + vert


def _forward(u):
    ux, uy = np.zeros_like(u), np.zeros_like(u)
    ux[:, :-1] = u[:, 1:] - u[:, :-1]
    uy[:-1] = u[1:] - u[:-1]
    return ux, uy


def tvl1(i0, i1, dtype=np.float64, **params):
    prm = dict(DEFAULTS)
    prm.update(params)
    dt = np.dtype(dtype).type
    tau, lam, theta, eps_p = dt(prm["tau"]), dt(prm["lam"]), dt(prm["theta"]), dt(prm["epsilon"])
    levels = plan(i0.shape[0], i0.shape[1], prm["nscales"], prm["scale_step"])
    if not levels:
        raise ValueError("a frame with a side below 16")
    pyr0, pyr1 = [i0.astype(dt)], [i1.astype(dt)]
    for shape in levels[1:]:
        pyr0.append(resize(pyr0[-1], shape, dt))
        pyr1.append(resize(pyr1[-1], shape, dt))
    n_warps, n_inner, n_outer = int(prm["warps"]), int(prm["inner"]), int(prm["outer"])
    iters = np.zeros((len(levels), n_warps), np.int32)
    errors = np.full((len(levels), n_warps), np.inf)
    eps_out = np.zeros(len(levels))
    l_t, taut = lam * theta, tau / theta
    flt_eps = dt(np.finfo(np.float32).eps)
    inv_step = dt(1) / dt(prm["scale_step"])
    u1 = u2 = None
    for s in range(len(levels) - 1, -1, -1):
        I0, I1 = pyr0[s], pyr1[s]
        h, w = levels[s]
        if u1 is None:
            u1, u2 = np.zeros((h, w), dt), np.zeros((h, w), dt)
        else:
            u1, u2 = resize(u1, (h, w), dt) * inv_step, resize(u2, (h, w), dt) * inv_step
        scaled_eps = eps_p * eps_p * dt(h * w)
        eps_out[s] = float(scaled_eps)
        I1x, I1y = gradient(I1, dt)
        p11, p12, p21, p22 = (np.zeros((h, w), dt) for _ in range(4))
        for wi in range(n_warps):
            I1w, I1wx, I1wy = bicubic([I1, I1x, I1y], u1, u2, dt)
            grad = I1wx * I1wx + I1wy * I1wy
            rho_c = I1w - I1wx * u1 - I1wy * u2 - I0
            error = np.inf
            n_o = 0
            while error > scaled_eps and n_o < n_outer:
                if prm["median"] > 1:
                    u1, u2 = median5(u1), median5(u2)
                n_i = 0
                while error > scaled_eps and n_i < n_inner:
                    rho = rho_c + I1wx * u1 + I1wy * u2
                    lo, hi = rho < -l_t * grad, rho > l_t * grad
                    with np.errstate(all="ignore"):
                        fi = np.where(grad > flt_eps, -rho / grad, dt(0))
                    fi = np.where(lo, l_t, np.where(hi, -l_t, fi)).astype(dt)
                    v1, v2 = u1 + fi * I1wx, u2 + fi * I1wy
                    n1 = v1 + theta * _divergence(p11, p12)
                    n2 = v2 + theta * _divergence(p21, p22)
                    d1, d2 = n1 - u1, n2 - u2
                    error = float(np.sum(d1 * d1 + d2 * d2, dtype=dt))
                    u1, u2 = n1, n2
                    u1x, u1y = _forward(u1)
                    u2x, u2y = _forward(u2)
                    g1 = np.sqrt(u1x * u1x + u1y * u1y)
                    g2 = np.sqrt(u2x * u2x + u2y * u2y)
                    den1, den2 = dt(1) + taut * g1, dt(1) + taut * g2
                    p11, p12 = (p11 + taut * u1x) / den1, (p12 + taut * u1y) / den1
                    p21, p22 = (p21 + taut * u2x) / den2, (p22 + taut * u2y) / den2
                    n_i += 1
                    iters[s, wi] += 1
                n_o += 1
            errors[s, wi] = error
    return {"flow": np.stack([u1, u2], axis=-1), "levels": levels, "iters": iters, "errors": errors, "eps": eps_out}


def interior_epe(flow, shift, margin=8):
    """Median endpoint error against a constant true flow, ``margin`` pixels off the border."""
    d = flow[margin:-margin, margin:-margin].astype(np.float64) - np.asarray(shift, np.float64)
    return float(np.median(np.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2)))
