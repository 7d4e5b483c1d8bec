"""numpy restatement of the renderer (frlw_evd_amd/csrc/render.hip), statement by statement: every background,
HSV -> BGR, the nearest sampling, the host packing of the boxes and the box painter.  float32 wherever the definition says
float32.  The glyph table below is this file's own copy; test_render_cpu.py compares it with csrc/render_font.h."""
import math

import numpy as np

f32 = np.float32

# character -> seven rows, top first; bit 4 of a row is the leftmost of the five columns
GLYPHS = {
    'a': (0b00000, 0b00000, 0b01110, 0b00001, 0b01111, 0b10001, 0b01111),
    'b': (0b10000, 0b10000, 0b11110, 0b10001, 0b10001, 0b10001, 0b11110),
    'c': (0b00000, 0b00000, 0b01110, 0b10001, 0b10000, 0b10001, 0b01110),
    'd': (0b00001, 0b00001, 0b01111, 0b10001, 0b10001, 0b10001, 0b01111),
    'e': (0b00000, 0b00000, 0b01110, 0b10001, 0b11111, 0b10000, 0b01110),
    'f': (0b00110, 0b01001, 0b01000, 0b11100, 0b01000, 0b01000, 0b01000),
    'g': (0b00000, 0b01111, 0b10001, 0b10001, 0b01111, 0b00001, 0b01110),
    'h': (0b10000, 0b10000, 0b10110, 0b11001, 0b10001, 0b10001, 0b10001),
    'i': (0b00100, 0b00000, 0b01100, 0b00100, 0b00100, 0b00100, 0b01110),
    'j': (0b00010, 0b00000, 0b00110, 0b00010, 0b00010, 0b10010, 0b01100),
    'k': (0b10000, 0b10000, 0b10010, 0b10100, 0b11000, 0b10100, 0b10010),
    'l': (0b01100, 0b00100, 0b00100, 0b00100, 0b00100, 0b00100, 0b01110),
    'm': (0b00000, 0b00000, 0b11010, 0b10101, 0b10101, 0b10101, 0b10101),
    'n': (0b00000, 0b00000, 0b10110, 0b11001, 0b10001, 0b10001, 0b10001),
    'o': (0b00000, 0b00000, 0b01110, 0b10001, 0b10001, 0b10001, 0b01110),
    'p': (0b00000, 0b11110, 0b10001, 0b10001, 0b11110, 0b10000, 0b10000),
    'q': (0b00000, 0b01111, 0b10001, 0b10001, 0b01111, 0b00001, 0b00001),
    'r': (0b00000, 0b00000, 0b10110, 0b11001, 0b10000, 0b10000, 0b10000),
    's': (0b00000, 0b00000, 0b01111, 0b10000, 0b01110, 0b00001, 0b11110),
    't': (0b01000, 0b01000, 0b11100, 0b01000, 0b01000, 0b01001, 0b00110),
    'u': (0b00000, 0b00000, 0b10001, 0b10001, 0b10001, 0b10011, 0b01101),
    'v': (0b00000, 0b00000, 0b10001, 0b10001, 0b10001, 0b01010, 0b00100),
    'w': (0b00000, 0b00000, 0b10001, 0b10001, 0b10101, 0b10101, 0b01010),
    'x': (0b00000, 0b00000, 0b10001, 0b01010, 0b00100, 0b01010, 0b10001),
    'y': (0b00000, 0b10001, 0b10001, 0b10001, 0b01111, 0b00001, 0b01110),
    'z': (0b00000, 0b00000, 0b11111, 0b00010, 0b00100, 0b01000, 0b11111),
    '0': (0b01110, 0b10001, 0b10011, 0b10101, 0b11001, 0b10001, 0b01110),
    '1': (0b00100, 0b01100, 0b00100, 0b00100, 0b00100, 0b00100, 0b01110),
    '2': (0b01110, 0b10001, 0b00001, 0b00010, 0b00100, 0b01000, 0b11111),
    '3': (0b11110, 0b00001, 0b00001, 0b01110, 0b00001, 0b00001, 0b11110),
    '4': (0b00010, 0b00110, 0b01010, 0b10010, 0b11111, 0b00010, 0b00010),
    '5': (0b11111, 0b10000, 0b11110, 0b00001, 0b00001, 0b10001, 0b01110),
    '6': (0b00110, 0b01000, 0b10000, 0b11110, 0b10001, 0b10001, 0b01110),
    '7': (0b11111, 0b00001, 0b00010, 0b00100, 0b01000, 0b01000, 0b01000),
    '8': (0b01110, 0b10001, 0b10001, 0b01110, 0b10001, 0b10001, 0b01110),
    '9': (0b01110, 0b10001, 0b10001, 0b01111, 0b00001, 0b00010, 0b01100),
    '.': (0b00000, 0b00000, 0b00000, 0b00000, 0b00000, 0b01100, 0b01100),
}

COLOUR_GT = (0, 255, 149)    # BGR
COLOUR_DT = (209, 255, 0)
SECTORS = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])
LIMIT = 1 << 20


def hsv_to_bgr(hsv):
    """(..., 3) uint8 H (units of 2 degrees), S, V -> (..., 3) uint8 B, G, R."""
    hsv = np.asarray(hsv, np.uint8)
    h = hsv[..., 0].astype(f32) * (f32(6) / f32(180))
    s = hsv[..., 1].astype(f32) * (f32(1) / f32(255))
    v = hsv[..., 2].astype(f32) * (f32(1) / f32(255))
    while (h < 0).any():
        h = np.where(h < 0, h + f32(6), h)
    while (h >= 6).any():
        h = np.where(h >= 6, h - f32(6), h)
    k = np.floor(h)
    f = h - k
    one = f32(1)
    tab = np.stack([v, v * (one - s), v * (one - s * f), v * (one - s * (one - f))], axis=-1)
    assert tab.dtype == np.float32
    idx = SECTORS[k.astype(np.int64)]                              # (..., 3): the table entry of b, g, r
    bgr = np.take_along_axis(tab, idx, axis=-1)
    bgr = np.where((s == 0)[..., None], v[..., None], bgr)
    return np.clip(np.rint(bgr * f32(255)), 0, 255).astype(np.uint8)


def nearest_index(n_out, n_in):
    """torch's interpolate(mode='nearest'): src = min(floor(dst * (float(in) / float(out))), in - 1), in float32."""
    scale = f32(n_in) / f32(n_out)
    return np.minimum(np.floor(np.arange(n_out, dtype=f32) * scale).astype(np.int64), n_in - 1)


def resize(vol, shape):
    """(C, h, w) -> (C, H, W) by nearest sampling."""
    return vol[:, nearest_index(shape[0], vol.shape[1])][:, :, nearest_index(shape[1], vol.shape[2])]


def _hsv_image(H, S, V):
    return hsv_to_bgr(np.stack([H.astype(np.uint8), np.broadcast_to(np.uint8(S), H.shape), np.broadcast_to(np.asarray(V, np.uint8), H.shape)], axis=-1))


def background_taf(vol):
    """visualizeTaf (visualization.py:222-233) on the sampled (C, H, W) uint8 volume."""
    ecds = vol.astype(f32)
    ecd = ecds.max(0)
    tar = ecd / f32(255)
    img_0 = (f32(120) * tar).astype(np.uint8) + np.uint8(119)
    tar2 = np.median(ecds, 0) / f32(180) * f32(255)
    assert tar2.dtype == np.float32
    tar2 = np.where(tar2 > 255, f32(255), tar2).astype(np.uint8)
    return _hsv_image(img_0, 255, tar2)


def background_sae(vol):
    """visualizeTimeSurface (:296-303)."""
    ecd = vol.astype(f32).max(0)
    img_0 = (f32(120) * (ecd / f32(255))).astype(np.uint8) + np.uint8(119)
    return _hsv_image(img_0, 255, 255)


def background_eci(vol):
    """visualizeFrame (:244-255); the negative float -> uint8 cast read as two's complement."""
    c_p = vol[1].astype(f32) / f32(255)
    c_n = vol[0].astype(f32) / f32(255)
    c_p = np.where(c_p > c_n, c_p, f32(0))
    c_n = np.where(c_n > c_p, c_n, f32(0))
    c_map = c_p * f32(127) - c_n * f32(127)
    assert c_map.dtype == np.float32
    grey = np.uint8(127) + c_map.astype(np.int32).astype(np.uint8)       # uint8 addition wraps
    return np.repeat(grey[:, :, None], 3, axis=2)


def background_ev(vol):
    """The evident intent of visualizeVolume (:266-284) with B = C / 2 bins."""
    B = vol.shape[0] // 2
    c = np.maximum(vol[B:2 * B], vol[:B])
    H = np.full(vol.shape[1:], 119, np.uint8)
    V = np.zeros(vol.shape[1:], np.uint8)
    best = np.zeros(vol.shape[1:], np.uint8)
    for i in range(B):
        win = c[i] > best
        H = np.where(win, np.uint8((239 + 30 * i) & 255), H)
        V = np.where(win, c[i], V)
        best = np.where(win, c[i], best)
    return _hsv_image(H, 255, V)


BACKGROUNDS = {"TAF": background_taf, "SAE": background_sae, "ECI": background_eci, "EV": background_ev}


def _clamp(v):
    return max(-LIMIT, min(LIMIT, v))


def _int(v):
    """int(v), truncation toward zero, clamped to +-2^20 (also for values no int32 holds)."""
    return _clamp(int(v)) if abs(v) < 1e18 else (LIMIT if v > 0 else -LIMIT)


def pack(gt, dt, labelmap):
    """Rows [t, x, y, w, h, class, confidence, track] -> [(x1, y1, x2, y2, kind, label, score)], ground truth (kind 0) first."""
    out = []
    for kind, rows in ((0, gt), (1, dt)):
        for row in ([] if rows is None else rows):
            row = [float(v) for v in row]
            if not all(math.isfinite(v) for v in row):
                continue
            x1, y1 = _int(row[1]), _int(row[2])
            x2, y2 = _clamp(x1 + _int(row[3])), _clamp(y1 + _int(row[4]))
            cls = _int(row[5])
            name = labelmap[cls] if 0 <= cls < len(labelmap) else str(cls)
            out.append((x1, y1, x2, y2, kind, name[:5] if kind else name[:3], "{0:.2f}".format(row[6])[:4] if kind else ""))
    return out


def _text(img, text, x, y):
    """Black 5 x 7 glyphs, advance 6, top-left of the first at (x, y); clipped to the image."""
    for ci, ch in enumerate(text):
        rows = GLYPHS.get(ch, (0,) * 7)
        for ry in range(7):
            for cx in range(5):
                px, py = x + 6 * ci + cx, y + ry
                if rows[ry] >> (4 - cx) & 1 and 0 <= px < img.shape[1] and 0 <= py < img.shape[0]:
                    img[py, px] = 0


def paint(img, boxes):
    """``boxes``: ``pack``'s list, applied in order onto the (H, W, 3) image in place: outline, tag fill, glyphs."""
    yy, xx = np.mgrid[0:img.shape[0], 0:img.shape[1]]
    for x1, y1, x2, y2, kind, label, score in boxes:
        colour = COLOUR_DT if kind else COLOUR_GT
        inside = (xx >= x1) & (xx <= x2) & (yy >= y1) & (yy <= y2)
        inner = (xx >= x1 + 2) & (xx <= x2 - 2) & (yy >= y1 + 2) & (yy <= y2 - 2)
        img[inside & ~inner] = colour
        img[(xx >= x1) & (xx <= x1 + (75 if kind else 35)) & (yy >= y1 - 15) & (yy <= y1)] = colour
        _text(img, label, x1 + 3, y1 - 11)
        if kind:
            _text(img, score, x1 + 40, y1 - 11)
    return img


def render(volumes, mode, shape, gt=None, dt=None, labelmap=("car", "ped")):
    """The whole of visualize.render in numpy: (n, C, h, w) uint8 (or (n, H, W, 3) for mode BGR) -> (n, H, W, 3) uint8 BGR."""
    out = []
    for i, vol in enumerate(volumes):
        img = vol.copy() if mode == "BGR" else BACKGROUNDS[mode](resize(vol, shape))
        out.append(paint(np.ascontiguousarray(img), pack(None if gt is None else gt[i], None if dt is None else dt[i], labelmap)))
    return np.stack(out)
