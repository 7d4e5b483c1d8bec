"""Seeded inputs of the TV-L1 tests, regenerated on both sides (tests/golden/make_golden_tvl1.py and the tests).

``blob_pair``: a smooth texture, a sum of Gaussian blobs with sigma between 2.5 and 6, and the same texture shifted analytically
by ``shift`` = (dx, dy) -- the true flow of the pair is that constant.  ``surface_pair``: what a time-surface pair looks like: large
zero areas, a few moving edges with a ramp of values behind them, 2 % impulse cells."""
import numpy as np

# name -> (H, W, shift, seed, contrast): the default-parameter cases.  Seed and contrast are CHOSEN, by the restatement alone, so that
# the last error of every (level, warp) keeps 5 % off the convergence threshold (tests/test_tvl1_cpu.py): with full contrast 4 to 17
# of the 25 (level, warp) loops of a case end within 5 % of it, whatever the seed; at a low contrast one texture in ten ((6, 4): in a thousand) passes.
SMOOTH = {"40x52": (40, 52, (1.5, -0.75), 110, 45.0), "64x80_a": (64, 80, (3.0, -2.0), 21, 15.0), "64x80_b": (64, 80, (6.0, 4.0), 1513, 15.0)}
SHORT = dict(epsilon=0.0, nscales=5, warps=2, outer=2, inner=5)
NOISY = (64, 80)
NOISY_BOXES = np.asarray([[0, 4, 40, 6, 30], [0, 30, 76, 20, 60], [0, 10, 70, 34, 58]], np.int32)   # [flow, x0, x1, y0, y1]


def _texture(rng, H, W, sigma):
    n = max(24, H * W // 40)
    cx, cy = rng.uniform(-8, W + 8, n), rng.uniform(-8, H + 8, n)
    sg, am = rng.uniform(sigma[0], sigma[1], n), rng.uniform(-1.0, 1.0, n)

    def render(dx, dy):
        y, x = np.mgrid[0:H, 0:W].astype(np.float64)
        out = np.zeros((H, W))
        for k in range(n):
            out += am[k] * np.exp(-((x - cx[k] - dx) ** 2 + (y - cy[k] - dy) ** 2) / (2 * sg[k] ** 2))
        return out
    return render


def blob_pair(H, W, shift, seed=7401, contrast=255.0, sigma=(2.5, 6.0)):
    """uint8 images; the first spans 0 .. ``contrast`` grey levels, the blobs' sigma is drawn from ``sigma``."""
    render = _texture(np.random.default_rng([seed, H, W]), H, W, sigma)
    a, b = render(0.0, 0.0), render(float(shift[0]), float(shift[1]))
    lo, hi = a.min(), a.max()
    q = lambda v: np.clip(np.rint((v - lo) / (hi - lo) * contrast), 0, 255).astype(np.uint8)   # noqa: E731
    return q(a), q(b)


def surface_pair(H, W, seed=7402, shift=(2.0, 1.0)):
    rng = np.random.default_rng([seed, H, W])
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = []
    for k, (dx, dy) in enumerate(((0.0, 0.0), shift)):
        img = np.zeros((H, W))
        for cx, cy, r in ((0.3 * W, 0.4 * H, 0.16 * H), (0.7 * W, 0.6 * H, 0.22 * H)):
            d = np.sqrt((x - cx - dx) ** 2 + (y - cy - dy) ** 2)
            ring = (d < r) & (d > r - 5)
            img = np.where(ring, 255.0 * (1 - (r - d) / 5.0 * 0.6), img)
        edge = np.abs(x - 0.5 * W - dx - 0.3 * (y - dy)) < 2
        img = np.where(edge, 200.0, img)
        hit = np.random.default_rng([seed, H, W, k]).uniform(size=(H, W)) < 0.02
        img = np.where(hit, rng.uniform(1, 255, (H, W)), img)
        out.append(img.astype(np.uint8))
    return out[0], out[1]


def timing_pairs(n, H, W, seed=7403):
    """``n`` time-surface-like pairs for the timing tool, (n, 2, H, W) uint8."""
    return np.stack([np.stack(surface_pair(H, W, seed + i, (1.0 + i % 3, 0.5 * (i % 4)))) for i in range(n)])


def wave_pair(H, W, shift, seed=7404):
    """A smooth texture for a large frame: twelve sinusoids of wavelength 12 .. 60 px, and the same shifted by ``shift``."""
    rng = np.random.default_rng([seed, H, W])
    k = 2 * np.pi / rng.uniform(12, 60, 12)
    th, ph, am = rng.uniform(0, np.pi, 12), rng.uniform(0, 2 * np.pi, 12), rng.uniform(0.3, 1.0, 12)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)

    def render(dx, dy):
        out = np.zeros((H, W))
        for i in range(12):
            out += am[i] * np.sin(k[i] * ((x - dx) * np.cos(th[i]) + (y - dy) * np.sin(th[i])) + ph[i])
        return out
    a, b = render(0.0, 0.0), render(float(shift[0]), float(shift[1]))
    lo, hi = a.min(), a.max()
    q = lambda v: np.clip(np.rint((v - lo) / (hi - lo) * 255.0), 0, 255).astype(np.uint8)   # noqa: E731
    return q(a), q(b)


def short_cases():
    """name -> ((image 0, image 1), parameters): the fixed short schedules (epsilon = 0, every loop runs its full count)."""
    return {
        "17x21": (blob_pair(17, 21, (0.7, -0.4)), dict(epsilon=0.0, nscales=1, warps=1, outer=1, inner=1)),
        "40x52": (blob_pair(40, 52, (1.5, -0.75)), dict(SHORT)),
        "noisy_64x80": (surface_pair(*NOISY), dict(SHORT)),
        "720x1280": (wave_pair(720, 1280, (2.5, -1.5)), dict(epsilon=0.0, nscales=5, warps=1, outer=1, inner=3)),
    }
