"""Numpy restatement of the volume hand-off (frlw_volume_hand_off_u8, transforms.hand_off): sample ``b`` is the first ``C``
``(h, w)`` planes of ``sources[b]``'s bytes; out (B, C, H, W) float32 = the planes at torch's nearest source indices -- computed in
float32: ``min(floor(float32(dst) * (float32(in) / float32(out))), in - 1)`` -- divided by ``float32(255)``."""
import numpy as np


def nearest_src(out_size, in_size):
    scale = np.float32(in_size) / np.float32(out_size)
    return np.minimum(np.floor(np.arange(out_size, dtype=np.float32) * scale).astype(np.int64), in_size - 1)


def hand_off(sources, C, src_shape, out_shape):
    h, w = (int(v) for v in src_shape)
    H, W = (int(v) for v in out_shape)
    ys, xs = nearest_src(H, h), nearest_src(W, w)
    out = np.empty((len(sources), C, H, W), np.float32)
    for b, s in enumerate(sources):
        planes = np.ascontiguousarray(s).view(np.uint8).reshape(-1)[:C * h * w].reshape(C, h, w)
        out[b] = planes[:, ys][:, :, xs].astype(np.float32) / np.float32(255)
    return out


# (h, w) -> (H, W) of tests/test_hand_off_gpu.py: resize up with W % 4 == 0; equal shapes (the word-load path); odd sizes (the
# scalar path); equal shapes whose samples are sliced at an odd plane offset of a larger tensor, at byte addresses that are no
# multiple of 4 (the byte-load path at equal shapes)
SHAPES = [((56, 72), (64, 96)), ((64, 96), (64, 96)), ((57, 73), (61, 97)), ((90, 160), (90, 160))]
