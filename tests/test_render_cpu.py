"""Visualization without a GPU: the restated colour conversion on the primaries, the glyph table of csrc/render_font.h against
the restatement's own copy, the host side of frlw_evd_amd/visualize.py (box selection and packing, the PNG writer, the OpticalFlow
colouring) and the argument checks of frlw_render_frames, which run before any launch."""
import ctypes as C
import os
import re
import struct
import sys
import zlib

import numpy as np
import pytest

import render_restated as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from frlw_evd_amd import _lib, visualize  # noqa: E402
from frlw_evd_amd.stream import BBOX_DTYPE  # noqa: E402


def test_hsv_to_bgr_on_the_primaries():
    def bgr(h, s, v):
        return tuple(int(c) for c in rr.hsv_to_bgr(np.array([h, s, v], np.uint8)))
    assert bgr(0, 255, 255) == (0, 0, 255)          # red
    assert bgr(60, 255, 255) == (0, 255, 0)         # green
    assert bgr(120, 255, 255) == (255, 0, 0)        # blue
    assert bgr(239, 255, 255) == bgr(59, 255, 255)  # H wraps at 180
    for v in (0, 1, 93, 254, 255):
        assert bgr(77, 0, v) == (v, v, v)           # S = 0: grey V
    assert bgr(30, 255, 255) == (0, 255, 255) and bgr(90, 255, 255) == (255, 255, 0) and bgr(150, 255, 255) == (255, 0, 255)


def test_glyph_header_equals_the_restatements_copy():
    text = open(os.path.join(ROOT, "frlw-evd_amd", "csrc", "render_font.h")).read()
    found = re.findall(r"^FRLW_GLYPH\('(.)',\s*((?:0b[01]{5}(?:,\s*)?){7})\)\s*$", text, flags=re.M)
    table = {ch: tuple(int(r, 2) for r in re.findall(r"0b[01]{5}", rows)) for ch, rows in found}
    assert [ch for ch, _ in found] == list("abcdefghijklmnopqrstuvwxyz0123456789.")     # the order render.hip indexes by
    assert len(re.findall(r"^FRLW_GLYPH\(", text, flags=re.M)) == len(found) == 37   # every entry parsed
    assert table == {ch: tuple(rows) for ch, rows in rr.GLYPHS.items()}
    assert all(any(rows) for rows in table.values()) and len(set(table.values())) == 37   # no blank glyph, no two alike


def test_select_boxes_at_the_tolerance():
    end = 1_000_000
    gt = np.zeros(3, BBOX_DTYPE)
    gt["t"] = [end - 1, end, end]
    gt["x"] = [1, 2, 3]
    dt = np.zeros((6, 8), np.float64)
    dt[:, 0] = [end - 5000, end - 4999, end - 4998, end + 4998, end + 4999, end + 5000]
    dt[:, 1] = np.arange(6)
    g, d = visualize.select_boxes(gt, dt, end)
    assert g["x"].tolist() == [2, 3]
    assert d[:, 1].tolist() == [2, 3]                  # end - tol < t < end + tol with tol = 4999: +-4999 and +-5000 are outside
    assert visualize.select_boxes(gt, dt, end, tol=5000)[1][:, 1].tolist() == [1, 2, 3, 4]
    assert visualize.select_boxes(gt, None, end)[1] is None


PACK_ROWS = np.array([
    [0, 10.9, 20.2, 30.7, 40.5, 0, 0.876, 0],          # fractions truncate
    [0, -3.9, -0.5, 7.99, 2.0, 1, 1.0, 0],             # toward zero: -3, 0
    [0, 1e30, -1e30, 1e12, 5, 0, 0.005, 0],            # clamped to +-2^20
    [0, 5, 5, -4.5, -2, 1, 0.995, 0],                  # negative size: x2 < x1
    [0, np.nan, 5, 5, 5, 0, 0.5, 0],                   # dropped
    [0, 5, 5, 5, np.inf, 0, 0.5, 0],                   # dropped
    [0, 5, 5, 5, 5, 0, np.nan, 0],                     # dropped
    [0, 7, 8, 9, 10, 6, 0.25, 0],                      # class outside the gen1 label map: its number
    [0, 1048570, 3, 100, 4, 0, 0.5, 0],                # x2 clamps
])


def unpack(rec):
    return [(int(r["x1"]), int(r["y1"]), int(r["x2"]), int(r["y2"]), int(r["kind"]), bytes(r["label"][:r["n_label"]]).decode(),
             bytes(r["score"][:r["n_score"]]).decode()) for r in rec]


def test_pack_boxes_against_the_restatement():
    for labelmap in (visualize.LABELMAPS["gen1"], visualize.LABELMAPS["gen4"]):
        rec = visualize.pack_boxes(PACK_ROWS, PACK_ROWS[::-1], labelmap)
        assert rec.dtype.itemsize == 32 and not rec["reserved"].any()
        want = rr.pack(PACK_ROWS, PACK_ROWS[::-1], labelmap)
        assert len(want) == 12 and unpack(rec) == want
    got = unpack(visualize.pack_boxes(PACK_ROWS, PACK_ROWS))
    assert got[0] == (10, 20, 40, 60, 0, "car", "") and got[6] == (10, 20, 40, 60, 1, "car", "0.88")
    assert got[1][:4] == (-3, 0, 4, 2) and got[7][5:] == ("ped", "1.00")
    assert got[2][:4] == (1 << 20, -(1 << 20), 1 << 20, -(1 << 20) + 5)
    assert got[3][:4] == (5, 5, 1, 3) and got[4][5] == "6" and got[5][:4] == (1048570, 3, 1 << 20, 7)
    assert unpack(visualize.pack_boxes(None, np.array([[0, 1, 2, 3, 4, 5, 0.5, 0]]), visualize.LABELMAPS["gen4"]))[0][5] == "sign"
    assert unpack(visualize.pack_boxes(np.array([[0, 1, 2, 3, 4, 6, 0.5, 0]]), None, visualize.LABELMAPS["gen4"]))[0][5] == "lig"
    # a structured *_bbox.npy array packs like its rows
    gt = np.zeros(2, BBOX_DTYPE)
    gt["x"], gt["y"], gt["w"], gt["h"], gt["class_id"] = [3.5, 9], [4, 9], [10, 2], [11, 2], [1, 0]
    assert unpack(visualize.pack_boxes(gt, None)) == [(3, 4, 13, 15, 0, "ped", ""), (9, 9, 11, 11, 0, "car", "")]
    assert len(visualize.pack_boxes(None, None)) == 0


def test_write_png_decodes_by_hand(tmp_path):
    rng = np.random.default_rng(5)
    for shape in ((1, 1), (7, 5), (40, 56)):
        img = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
        path = str(tmp_path / "x.png")
        visualize.write_png(path, img)
        data = open(path, "rb").read()
        assert data[:8] == b"\x89PNG\r\n\x1a\n"
        pos, chunks = 8, []
        while pos < len(data):
            n, = struct.unpack(">I", data[pos:pos + 4])
            tag, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
            assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF, tag
            chunks.append((tag, body))
            pos += 12 + n
        assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"] and pos == len(data)
        assert chunks[0][1] == struct.pack(">IIBBBBB", shape[1], shape[0], 8, 2, 0, 0, 0)
        raw = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(shape[0], 1 + 3 * shape[1])
        assert not raw[:, 0].any()                                                       # filter byte 0 on every row
        assert np.array_equal(raw[:, 1:].reshape(shape + (3,)), img[:, :, ::-1])         # RGB order in the file
        assert np.array_equal(visualize.read_png(path), img)
        try:
            from PIL import Image
        except ImportError:
            continue
        assert np.array_equal(np.asarray(Image.open(path).convert("RGB")), img[:, :, ::-1])
    with pytest.raises(ValueError):
        visualize.png_bytes(np.zeros((4, 4), np.uint8))


# ---- the reference's OpticalFlow colouring (visualization.py:64-207), transliterated: the yardstick of visualize.flow_image

def make_color_wheel():
    RY = 15
    YG = 6
    GC = 4
    CB = 11
    BM = 13
    MR = 6
    ncols = RY + YG + GC + CB + BM + MR
    colorwheel = np.zeros([ncols, 3])
    col = 0
    colorwheel[0:RY, 0] = 255
    colorwheel[0:RY, 1] = np.transpose(np.floor(255 * np.arange(0, RY) / RY))
    col += RY
    colorwheel[col:col + YG, 0] = 255 - np.transpose(np.floor(255 * np.arange(0, YG) / YG))
    colorwheel[col:col + YG, 1] = 255
    col += YG
    colorwheel[col:col + GC, 1] = 255
    colorwheel[col:col + GC, 2] = np.transpose(np.floor(255 * np.arange(0, GC) / GC))
    col += GC
    colorwheel[col:col + CB, 1] = 255 - np.transpose(np.floor(255 * np.arange(0, CB) / CB))
    colorwheel[col:col + CB, 2] = 255
    col += CB
    colorwheel[col:col + BM, 2] = 255
    colorwheel[col:col + BM, 0] = np.transpose(np.floor(255 * np.arange(0, BM) / BM))
    col += + BM
    colorwheel[col:col + MR, 2] = 255 - np.transpose(np.floor(255 * np.arange(0, MR) / MR))
    colorwheel[col:col + MR, 0] = 255
    return colorwheel


def compute_color(u, v):
    [h, w] = u.shape
    img = np.zeros([h, w, 3])
    nanIdx = np.isnan(u) | np.isnan(v)
    u[nanIdx] = 0
    v[nanIdx] = 0
    colorwheel = make_color_wheel()
    ncols = np.size(colorwheel, 0)
    rad = np.sqrt(u ** 2 + v ** 2)
    a = np.arctan2(-v, -u) / np.pi
    fk = (a + 1) / 2 * (ncols - 1) + 1
    k0 = np.floor(fk).astype(int)
    k1 = k0 + 1
    k1[k1 == ncols + 1] = 1
    f = fk - k0
    for i in range(0, np.size(colorwheel, 1)):
        tmp = colorwheel[:, i]
        col0 = tmp[k0 - 1] / 255
        col1 = tmp[k1 - 1] / 255
        col = (1 - f) * col0 + f * col1
        idx = rad <= 1
        col[idx] = 1 - rad[idx] * (1 - col[idx])
        notidx = np.logical_not(idx)
        col[notidx] *= 0.75
        img[:, :, i] = np.uint8(np.floor(255 * col * (1 - nanIdx)))
    return img


def flow_to_image(flow):
    u = flow[:, :, 0]
    v = flow[:, :, 1]
    UNKNOWN_FLOW_THRESH = 1e7
    idxUnknow = (abs(u) > UNKNOWN_FLOW_THRESH) | (abs(v) > UNKNOWN_FLOW_THRESH)
    u[idxUnknow] = 0
    v[idxUnknow] = 0
    u = np.where(u > np.quantile(u, 0.98), np.quantile(u, 0.98), u)
    u = np.where(u < np.quantile(u, 0.02), np.quantile(u, 0.02), u)
    v = np.where(v > np.quantile(v, 0.98), np.quantile(v, 0.98), v)
    v = np.where(v < np.quantile(u, 0.02), np.quantile(v, 0.02), v)
    rad = np.sqrt(u ** 2 + v ** 2)
    maxrad = max(-1, np.max(rad))
    u = u / (maxrad + np.finfo(float).eps)
    v = v / (maxrad + np.finfo(float).eps)
    img = compute_color(u, v)
    idx = np.repeat(idxUnknow[:, :, np.newaxis], 3, axis=2)
    img[idx] = 0
    return np.uint8(img)


def save_flow_image(flow):
    flow_img = 255 - flow_to_image(flow)
    flow_img = flow_img / 255.0
    return (np.power(flow_img, 0.4) * 255.0).astype(np.uint8)


def test_flow_image_against_the_transliteration():
    rng = np.random.default_rng(9)
    flow = rng.normal(0, 3, (12, 16, 2))
    flow[2, 3] = (40.0, -35.0)                         # beyond the quantiles
    keep = flow.copy()
    got = visualize.flow_image(flow)
    assert np.array_equal(flow, keep)                  # the caller's array is left alone (the reference writes into it)
    assert got.dtype == np.uint8 and got.shape == (12, 16, 3)
    assert np.array_equal(got, save_flow_image(keep.copy()))
    assert len(np.unique(got.reshape(-1, 3), axis=0)) > 50
    # float32 input is computed in float64 all the same
    assert np.array_equal(visualize.flow_image(keep.astype(np.float32)), save_flow_image(keep.astype(np.float32).astype(np.float64)))


def test_flow_image_zero_and_unknown_flow():
    zero = visualize.flow_image(np.zeros((5, 7, 2)))   # maxrad = 0: u / eps = 0, radius 0 -> white -> 255 - 255 = 0
    assert zero.shape == (5, 7, 3) and not zero.any()
    rng = np.random.default_rng(10)
    flow = rng.normal(0, 2, (12, 16, 2))
    flow[1, 1, 0] = 2e7                                # unknown: zeroed, then painted 0 -> 255 after the inversion
    flow[4, 5, 1] = -3e7
    got = visualize.flow_image(flow)
    assert (got[1, 1] == 255).all() and (got[4, 5] == 255).all()
    assert np.array_equal(got, save_flow_image(flow.copy()))
    flow[7, 2, 0] = np.nan                             # a NaN survives to the quantiles: nothing is clipped, maxrad = -1
    with np.errstate(all="ignore"):
        got = visualize.flow_image(flow)
        want = save_flow_image(flow.copy())
    assert got.shape == (12, 16, 3) and np.array_equal(got, want)
    assert (got[7, 2] == 255).all()                    # the NaN pixel itself is painted 0, 255 after the inversion


# ---- argument checks of the C-ABI: host only, nothing is launched

def render_rc(n=1, Cn=16, h=8, w=8, mode=0, H=8, W=8, src=0x1000, out=0x2000, boxes=0x4000, offsets=(0, 0), null_offsets=False):
    lib = _lib.load()
    offs = (C.c_int32 * len(offsets))(*offsets)
    return lib.frlw_render_frames(C.c_void_p(src), n, Cn, h, w, mode, H, W, C.c_void_p(boxes), None if null_offsets else offs,
                                  C.c_void_p(out), None)


def test_render_argument_checks_are_host_only():
    E = _lib.FRLW_ERR_ARG
    assert render_rc(src=None) == E and render_rc(out=None) == E and render_rc(null_offsets=True) == E
    assert render_rc(n=0) == E and render_rc(n=-1) == E and render_rc(n=65, offsets=(0,) * 66) == E
    assert render_rc(offsets=(0, 513)) == E                                   # more than 512 boxes in a frame
    assert render_rc(n=2, offsets=(0, 512, 1025)) == E
    assert render_rc(offsets=(3, 2)) == E and render_rc(offsets=(-1, 0)) == E   # offsets run backwards / start below 0
    assert render_rc(offsets=(0, 4), boxes=None) == E                         # boxes announced, none given
    assert render_rc(offsets=(0, 4), boxes=0x4004) == E                       # records are read as 16-byte halves
    taf, sae, eci, ev, bgr = range(5)
    assert render_rc(mode=taf, Cn=15) == E and render_rc(mode=taf, Cn=0) == E and render_rc(mode=taf, Cn=1) == E
    assert render_rc(mode=sae, Cn=0) == E
    assert render_rc(mode=eci, Cn=1) == E and render_rc(mode=eci, Cn=4) == E
    assert render_rc(mode=ev, Cn=5) == E and render_rc(mode=ev, Cn=0) == E
    assert render_rc(mode=bgr, Cn=16) == E and render_rc(mode=bgr, Cn=3, h=4) == E
    assert render_rc(mode=5) == E and render_rc(mode=-1) == E
    for name in ("h", "w", "H", "W"):
        assert render_rc(**{name: 0}) == E and render_rc(**{name: -8}) == E
    lib = _lib.load()
    p = C.c_void_p(0x1000)
    assert lib.frlw_hsv_to_bgr_u8(None, p, 4, None) == E and lib.frlw_hsv_to_bgr_u8(p, None, 4, None) == E
    assert lib.frlw_hsv_to_bgr_u8(p, p, -1, None) == E and lib.frlw_hsv_to_bgr_u8(p, p, 0, None) == 0
    assert _lib.RENDER_MAX_FRAMES == 64 and _lib.RENDER_MAX_BOXES == 512 and _lib.RENDER_MODES.index("BGR") == 4


def test_render_refuses_what_the_library_would():
    """visualize.render's own checks come before any device work."""
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError):
        visualize.render(torch.zeros((1, 16, 8, 8), dtype=torch.uint8), "TAF", (8, 8))      # not on the GPU
    with pytest.raises(ValueError):
        visualize.render(torch.zeros((1, 16, 8, 8), dtype=torch.uint8), "Taf", (8, 8))      # no such datatype


# ---- the command

def test_nearest_index_is_torchs_rule():
    torch = pytest.importorskip("torch")
    for n_in, n_out in ((16, 13), (24, 19), (16, 16), (256, 240), (320, 304), (512, 720), (640, 1280), (7, 50)):
        x = torch.arange(n_in, dtype=torch.float32).reshape(1, 1, 1, n_in)
        want = torch.nn.functional.interpolate(x, size=(1, n_out), mode="nearest").reshape(-1).numpy().astype(np.int64)
        assert np.array_equal(rr.nearest_index(n_out, n_in), want), (n_in, n_out)


README_GEN4 = ("-item EVENT_STREAM_NAME -end 12345 -volume_bins 8 -ecd taf -bbox_path root/Large_Automotive_Detection_Dataset_sampling "
               "-data_path root/Large_Automotive_Detection_Dataset_processed -result_path log/EXP_NAME/summarise.npz -datatype TAF "
               "-suffix taf -dataset gen4")
README_GEN1 = ("-item EVENT_STREAM_NAME -end 12345 -volume_bins 5 -ecd long -bbox_path root/detection_dataset_duration_60s_ratio_1.0 "
               "-data_path root/ATIS_Automotive_Detection_Dataset_processed/long -datatype EventVolume -suffix long -dataset gen1")


def test_visualization_parser_and_file_names():
    import visualization as vz
    a = vz.build_parser().parse_args(README_GEN4.split())
    assert (a.item, a.end, a.volume_bins, a.dataset, a.datatype, a.suffix) == ("EVENT_STREAM_NAME", 12345, 8.0, "gen4", "TAF", "taf")
    assert a.result_path == "log/EXP_NAME/summarise.npz"
    assert vz.output_name(a.item, a.end, a.suffix, a.datatype, True) == "EVENT_STREAM_NAME_12345_taf_TAF_result.png"
    root = os.path.join("root/Large_Automotive_Detection_Dataset_processed", "test")
    assert vz.volume_files(a) == [(os.path.join(root, "bins4", "EVENT_STREAM_NAME_12345.npy"), 8),
                                  (os.path.join(root, "bins8", "EVENT_STREAM_NAME_12345.npy"), 8)]
    assert vz.SHAPES[vz.dataset_key(a.dataset)] == ((720, 1280), (512, 640))
    b = vz.build_parser().parse_args(README_GEN1.split())
    assert b.result_path is None and b.volume_bins == 5.0
    assert vz.output_name(b.item, b.end, b.suffix, b.datatype, False) == "EVENT_STREAM_NAME_12345_long_EventVolume.png"
    assert vz.volume_files(b) == [(os.path.join("root/ATIS_Automotive_Detection_Dataset_processed/long", "long", "test",
                                                "EVENT_STREAM_NAME_12345.npy"), 10)]
    assert vz.SHAPES[vz.dataset_key(b.dataset)] == ((240, 304), (256, 320))
    names = {d: vz.output_name("i", 7, "s", d, r) for d in vz.DATATYPES for r in (False,)}
    assert names == {"TAF": "i_7_s_TAF.png", "SurfaceOfActiveEvent": "i_7_s_SurfaceOfActiveEvent.png",
                     "EventCountImage": "i_7_s_EventCountImage.png", "EventVolume": "i_7_s_EventVolume.png",
                     "OpticalFlow": "i_7_OpticalFlow.png"}
    assert vz.output_name("i", 7, "s", "OpticalFlow", True) == "i_7_OpticalFlow_result.png"
    a.volume_bins = 4.0
    assert vz.volume_files(a) == [(os.path.join(root, "bins4", "EVENT_STREAM_NAME_12345.npy"), 8)]
    assert len(vz.build_parser()._actions) == 11     # the reference's ten flags and -h
