"""The left-neighbour sample prediction of BIC_OPT_SAMPLE_PREDICT in numpy, on uint8 images [..., rows, cols]:
predict(img, mode) = T(img), unpredict(z, mode) its inverse. Mode 1: d(i, j) = (v(i, j) - v(i, j - 1)) mod 256 with
v(i, -1) = 0; mode 2: d read as a signed byte and folded, z = ((d << 1) ^ (d >> 7)) & 0xFF; mode 0: the identity.
Plain integer arithmetic along the last axis: nothing here knows of planes, strips or lanes."""
import numpy as np


def fold(d):
    """signed byte d (given as uint8) -> ((d << 1) ^ (d >> 7)) & 0xFF: 0, -1, 1, -128 -> 0, 1, 2, 255"""
    s = np.asarray(d, np.uint8).astype(np.int8).astype(np.int32)
    return (((s << 1) ^ (s >> 7)) & 0xFF).astype(np.uint8)


def unfold(z):
    """the inverse of fold: d = (z >> 1) ^ -(z & 1), as uint8"""
    z = np.asarray(z, np.uint8).astype(np.int32)
    return (((z >> 1) ^ -(z & 1)) & 0xFF).astype(np.uint8)


def predict(img, mode):
    img = np.asarray(img, np.uint8)
    if mode == 0:
        return img.copy()
    assert mode in (1, 2), mode
    d = np.diff(img, axis=-1, prepend=np.uint8(0)).astype(np.uint8)  # (uint8 arithmetic wraps mod 256)
    return fold(d) if mode == 2 else d


def unpredict(z, mode):
    z = np.asarray(z, np.uint8)
    if mode == 0:
        return z.copy()
    assert mode in (1, 2), mode
    d = unfold(z) if mode == 2 else z
    return np.cumsum(d, axis=-1, dtype=np.uint8)
