"""Visualization (the reference's ``visualization.py``, README section 7): representation -> colour image -> boxes with tags.

``render`` paints up to 64 frames per launch on the GPU (``csrc/render.hip``; the definitions are in DESIGN.md 3.16): the uint8
volumes stay where the encoder left them, and what comes back is ``(n, H, W, 3)`` uint8 BGR.  The OpticalFlow datatype is the
exception: ``flow_image`` restates the reference's Middlebury colouring on the host in float64 (one image per call, ``arctan2``
and quantiles -- not a hot path, and not something a GPU reproduces bit for bit), and its result goes through
``render(..., "BGR")`` for the boxes.  ``write_png`` needs nothing but the standard library.
"""
from __future__ import annotations

import ctypes as C
import struct
import zlib

import numpy as np

from . import _lib

LABELMAPS = {"gen1": ["car", "ped"], "gen4": ["ped", "cyc", "car", "trk", "bus", "sign", "light"]}   # visualization.py:350-354
DATATYPES = {"TAF": "TAF", "SurfaceOfActiveEvent": "SAE", "SAE": "SAE", "EventCountImage": "ECI", "ECI": "ECI",
             "EventVolume": "EV", "EV": "EV", "BGR": "BGR"}
COORD_LIMIT = 1 << 20
GT_LABEL_CHARS, DT_LABEL_CHARS, SCORE_CHARS = 3, 5, 4

# frlw_render_box_t
BOX_DTYPE = np.dtype([("x1", "<i4"), ("y1", "<i4"), ("x2", "<i4"), ("y2", "<i4"), ("kind", "u1"), ("n_label", "u1"),
                      ("n_score", "u1"), ("reserved", "u1"), ("label", "u1", (8,)), ("score", "u1", (4,))])
assert BOX_DTYPE.itemsize == 32

_FIELDS = ("t", "x", "y", "w", "h", "class_id", "class_confidence", "track_id")


def box_rows(boxes):
    """``(n, 8)`` float64 rows ``[t, x, y, w, h, class, confidence, track]`` of a row array or of a structured ``*_bbox.npy``
    array (its fields in this order); None -> no rows."""
    if boxes is None:
        return np.zeros((0, 8), np.float64)
    a = np.asarray(boxes)
    if a.dtype.names:
        return np.stack([a[name].astype(np.float64) for name in _FIELDS], axis=1).reshape(-1, 8)
    return a.astype(np.float64).reshape(-1, 8)


def _trunc_clamped(v):
    return np.clip(np.trunc(v), -COORD_LIMIT, COORD_LIMIT).astype(np.int64)


def _pack_kind(rows, kind, labelmap):
    rows = box_rows(rows)
    rows = rows[np.isfinite(rows).all(axis=1)]
    rec = np.zeros(len(rows), BOX_DTYPE)
    x1, y1 = _trunc_clamped(rows[:, 1]), _trunc_clamped(rows[:, 2])
    rec["x1"], rec["y1"] = x1, y1
    rec["x2"] = np.clip(x1 + _trunc_clamped(rows[:, 3]), -COORD_LIMIT, COORD_LIMIT)
    rec["y2"] = np.clip(y1 + _trunc_clamped(rows[:, 4]), -COORD_LIMIT, COORD_LIMIT)
    rec["kind"] = kind
    for i, row in enumerate(rows):
        cls = int(np.clip(np.trunc(row[5]), -COORD_LIMIT, COORD_LIMIT))
        name = labelmap[cls] if 0 <= cls < len(labelmap) else str(cls)
        label = name[:DT_LABEL_CHARS if kind else GT_LABEL_CHARS].encode("ascii", "replace")
        score = "{0:.2f}".format(row[6])[:SCORE_CHARS].encode("ascii") if kind else b""
        rec["n_label"][i], rec["n_score"][i] = len(label), len(score)
        rec["label"][i, :len(label)] = np.frombuffer(label, np.uint8)
        rec["score"][i, :len(score)] = np.frombuffer(score, np.uint8)
    return rec


def pack_boxes(gt, dt, labelmap=LABELMAPS["gen1"]):
    """One frame's ground truth and detections -> the 32-byte records ``frlw_render_frames`` reads, ground truth first, each in
    file order.  ``x1 = int(x)``, ``x2 = x1 + int(w)`` (truncation toward zero, everything clamped to +-2^20), rows with a
    non-finite field dropped; ground truth carries the first three characters of its class name, a detection the first five and
    its confidence as ``"{:.2f}"`` (four characters).  A class outside the label map shows its number."""
    return np.concatenate([_pack_kind(gt, 0, labelmap), _pack_kind(dt, 1, labelmap)])


def select_boxes(gt, dt, t, tol=4999):
    """The reference's choice of boxes for the frame at ``t`` (visualization.py:234-237): ground truth (a structured
    ``*_bbox.npy`` array) with ``t == end``, detections (rows of ``summarise.npz``'s ``dts``; None = no result file) with
    ``end - tol < t < end + tol``."""
    gt = np.asarray(gt)
    gt_sel = gt[gt["t"] == t] if gt.dtype.names else gt[gt[:, 0] == t]
    if dt is None:
        return gt_sel, None
    dt = np.asarray(dt)
    if not dt.dtype.names:
        dt = dt.reshape(-1, 8)
    ts = dt["t"].astype(np.int64) if dt.dtype.names else dt[:, 0]
    return gt_sel, dt[(ts > t - tol) & (ts < t + tol)]


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def render(volumes, datatype, sensor_shape, gt=None, dt=None, labelmap=LABELMAPS["gen1"]):
    """``volumes``: uint8 CUDA tensor ``(n, C, h, w)`` at the stored shape, or ``(n, H, W, 3)`` BGR with ``datatype="BGR"``.
    ``datatype``: TAF, SurfaceOfActiveEvent, EventCountImage, EventVolume (or SAE / ECI / EV) or BGR.  ``gt`` / ``dt``: None, or
    one entry per frame (row array, structured array or None).  Returns ``(n, H, W, 3)`` uint8 BGR on the device.  More than
    64 frames are split into calls; more than 512 boxes in a frame raise ``ValueError``."""
    import torch
    if datatype not in DATATYPES:
        raise ValueError(f"datatype: one of {sorted(DATATYPES)}")
    mode = DATATYPES[datatype]
    if volumes.dtype != torch.uint8 or volumes.dim() != 4 or not volumes.is_cuda:
        raise ValueError("render: a 4-D uint8 CUDA tensor")
    H, W = int(sensor_shape[0]), int(sensor_shape[1])
    src = volumes.contiguous()
    n = src.shape[0]
    if mode == "BGR":
        if tuple(src.shape[1:]) != (H, W, 3):
            raise ValueError("render: BGR backgrounds are (n, H, W, 3) at the sensor shape")
        Cn, h, w = 3, H, W
    else:
        Cn, h, w = (int(v) for v in src.shape[1:])
    for name, lst in (("gt", gt), ("dt", dt)):
        if lst is not None and len(lst) != n:
            raise ValueError(f"render: {name} needs one entry per frame")
    packed = [pack_boxes(None if gt is None else gt[i], None if dt is None else dt[i], labelmap) for i in range(n)]
    if any(len(p) > _lib.RENDER_MAX_BOXES for p in packed):
        raise ValueError(f"render: more than {_lib.RENDER_MAX_BOXES} boxes in a frame")
    out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=src.device)
    lib = _lib.load()
    with torch.cuda.device(src.device):
        for lo in range(0, n, _lib.RENDER_MAX_FRAMES):
            part = packed[lo:lo + _lib.RENDER_MAX_FRAMES]
            m = len(part)
            offsets = np.zeros(m + 1, np.int32)
            offsets[1:] = np.cumsum([len(p) for p in part])
            boxes_d = None
            if offsets[-1]:
                host = np.concatenate(part).view(np.uint8).reshape(-1, BOX_DTYPE.itemsize)
                boxes_d = torch.from_numpy(host).to(src.device)
            rc = lib.frlw_render_frames(_ptr(src[lo:lo + m]), m, Cn, h, w, _lib.RENDER_MODES.index(mode), H, W,
                                        None if boxes_d is None else _ptr(boxes_d), offsets.ctypes.data_as(C.POINTER(C.c_int32)),
                                        _ptr(out[lo:lo + m]), _stream())
            _lib.check(rc, "render")
            if boxes_d is not None:
                boxes_d.record_stream(torch.cuda.current_stream())
    return out


def hsv_to_bgr(hsv):
    """uint8 CUDA tensor ``(..., 3)`` of H (units of 2 degrees; values above 180 wrap), S, V -> B, G, R, the conversion the TAF,
    SurfaceOfActiveEvent and EventVolume backgrounds go through."""
    import torch
    if hsv.dtype != torch.uint8 or not hsv.is_cuda or hsv.shape[-1] != 3:
        raise ValueError("hsv_to_bgr: a uint8 CUDA tensor (..., 3)")
    src = hsv.contiguous()
    out = torch.empty_like(src)
    with torch.cuda.device(src.device):
        _lib.check(_lib.load().frlw_hsv_to_bgr_u8(_ptr(src), _ptr(out), src.numel() // 3, _stream()), "hsv_to_bgr")
    return out


# ---- OpticalFlow: flow_to_image / compute_color / save_flow (visualization.py:64-207) on the host, float64

def _color_wheel():
    RY, YG, GC, CB, BM, MR = 15, 6, 4, 11, 13, 6
    wheel = np.zeros([RY + YG + GC + CB + BM + MR, 3])
    col = 0
    wheel[0:RY, 0] = 255
    wheel[0:RY, 1] = np.floor(255 * np.arange(0, RY) / RY)
    col += RY
    wheel[col:col + YG, 0] = 255 - np.floor(255 * np.arange(0, YG) / YG)
    wheel[col:col + YG, 1] = 255
    col += YG
    wheel[col:col + GC, 1] = 255
    wheel[col:col + GC, 2] = np.floor(255 * np.arange(0, GC) / GC)
    col += GC
    wheel[col:col + CB, 1] = 255 - np.floor(255 * np.arange(0, CB) / CB)
    wheel[col:col + CB, 2] = 255
    col += CB
    wheel[col:col + BM, 2] = 255
    wheel[col:col + BM, 0] = np.floor(255 * np.arange(0, BM) / BM)
    col += BM
    wheel[col:col + MR, 2] = 255 - np.floor(255 * np.arange(0, MR) / MR)
    wheel[col:col + MR, 0] = 255
    return wheel


def _compute_color(u, v):
    img = np.zeros(u.shape + (3,))
    nan = np.isnan(u) | np.isnan(v)
    u[nan] = 0
    v[nan] = 0
    wheel = _color_wheel()
    ncols = wheel.shape[0]
    rad = np.sqrt(u ** 2 + v ** 2)
    a = np.arctan2(-v, -u) / np.pi
    fk = (a + 1) / 2 * (ncols - 1) + 1
    k0 = np.floor(fk).astype(int)
    k1 = k0 + 1
    k1[k1 == ncols + 1] = 1
    f = fk - k0
    for i in range(3):
        tmp = wheel[:, i]
        col = (1 - f) * (tmp[k0 - 1] / 255) + f * (tmp[k1 - 1] / 255)
        idx = rad <= 1
        col[idx] = 1 - rad[idx] * (1 - col[idx])
        col[np.logical_not(idx)] *= 0.75
        img[:, :, i] = np.uint8(np.floor(255 * col * (1 - nan)))
    return img


def flow_image(flow):
    """``(H, W, 2)`` flow -> ``(H, W, 3)`` uint8, the image ``save_flow`` hands to ``draw_bboxes`` and ``cv2.imwrite`` (so its
    channel order is what the reference writes as BGR): the Middlebury colouring of the flow clipped to its 2 % / 98 % quantiles --
    with the reference's own mix on line 186, where ``v`` is compared with ``u``'s lower quantile -- then ``255 - img`` and the
    power 0.4.  float64 throughout; the caller's array is left alone."""
    flow = np.array(flow, dtype=np.float64, copy=True)
    u, v = flow[:, :, 0], flow[:, :, 1]
    unknown = (abs(u) > 1e7) | (abs(v) > 1e7)
    u[unknown] = 0
    v[unknown] = 0
    u = np.where(u > np.quantile(u, 0.98), np.quantile(u, 0.98), u)
    u = np.where(u < np.quantile(u, 0.02), np.quantile(u, 0.02), u)
    v = np.where(v > np.quantile(v, 0.98), np.quantile(v, 0.98), v)
    v = np.where(v < np.quantile(u, 0.02), np.quantile(v, 0.02), v)
    rad = np.sqrt(u ** 2 + v ** 2)
    maxrad = max(-1, np.max(rad))
    u = u / (maxrad + np.finfo(float).eps)
    v = v / (maxrad + np.finfo(float).eps)
    img = _compute_color(u, v)
    img[np.repeat(unknown[:, :, np.newaxis], 3, axis=2)] = 0
    img = 255 - np.uint8(img)
    return (np.power(img / 255.0, 0.4) * 255.0).astype(np.uint8)


# ---- PNG

def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def png_bytes(bgr, level=6):
    """``(H, W, 3)`` uint8 BGR -> the bytes of an 8-bit RGB PNG (filter 0 on every row)."""
    img = np.asarray(bgr)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError("write_png: (H, W, 3) uint8")
    H, W = img.shape[:2]
    rows = np.zeros((H, 1 + 3 * W), np.uint8)
    rows[:, 1:] = img[:, :, ::-1].reshape(H, 3 * W)
    return (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)) +
            _chunk(b"IDAT", zlib.compress(rows.tobytes(), level)) + _chunk(b"IEND", b""))


def write_png(path, bgr):
    """Write ``(H, W, 3)`` uint8 BGR (numpy, or a tensor on any device) as an RGB PNG; standard library only."""
    if hasattr(bgr, "detach"):
        bgr = bgr.detach().cpu().numpy()
    with open(path, "wb") as f:
        f.write(png_bytes(bgr))


def read_png(path):
    """The inverse of ``write_png`` for the files it writes (8-bit RGB, no interlace, filter 0): ``(H, W, 3)`` uint8 BGR."""
    data = open(path, "rb").read()
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError("not a PNG file")
    pos, idat, shape = 8, b"", None
    while pos < len(data):
        (n,), tag = struct.unpack(">I", data[pos:pos + 4]), data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        if struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] != zlib.crc32(tag + body) & 0xFFFFFFFF:
            raise ValueError("PNG chunk checksum")
        if tag == b"IHDR":
            W, H, depth, colour, _, _, interlace = struct.unpack(">IIBBBBB", body)
            if (depth, colour, interlace) != (8, 2, 0):
                raise ValueError("read_png reads what write_png writes: 8-bit RGB, no interlace")
            shape = (H, W)
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(shape[0], 1 + 3 * shape[1])
    if rows[:, 0].any():
        raise ValueError("read_png reads filter 0 rows only")
    return np.ascontiguousarray(rows[:, 1:].reshape(shape[0], shape[1], 3)[:, :, ::-1])
