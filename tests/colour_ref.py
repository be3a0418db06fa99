"""The reversible colour transforms of BIC_OPT_COLOR_TRANSFORM in numpy, on interleaved images [..., 3] of
one-byte samples R, G, B. forward(img, mode): mode 0 the image itself; mode 1 R' = (R - G) mod 256, G' = G,
B' = (B - G) mod 256; mode 2 the same differences read as signed 8-bit d and folded, z = ((d << 1) ^ (d >> 7))
& 0xFF with an arithmetic shift. inverse(img, mode) undoes it: d = (z >> 1) ^ -(z & 1), R = (d + G) & 0xFF.
Plain integer arithmetic on the samples: nothing here knows of planes, bytes in a dword or Gray codes."""
import numpy as np


def fold(d):
    """signed 8-bit difference(s) d (-128 .. 127) -> 0 .. 255: 0, -1, 1, -2, ... -> 0, 1, 2, 3, ..."""
    d = np.asarray(d, dtype=np.int64)
    return ((d << 1) ^ (d >> 7)) & 0xFF


def unfold(z):
    """the inverse of fold(): 0 .. 255 -> -128 .. 127"""
    z = np.asarray(z, dtype=np.int64)
    return (z >> 1) ^ -(z & 1)


def forward(img, mode):
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.shape[-1] == 3 and mode in (0, 1, 2)
    if mode == 0:
        return img.copy()
    v = img.astype(np.int64)
    out = v.copy()
    for c in (0, 2):
        d = (v[..., c] - v[..., 1]) & 0xFF
        if mode == 2:
            d = fold(np.where(d >= 128, d - 256, d))
        out[..., c] = d
    return out.astype(np.uint8)


def inverse(img, mode):
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.shape[-1] == 3 and mode in (0, 1, 2)
    if mode == 0:
        return img.copy()
    v = img.astype(np.int64)
    out = v.copy()
    for c in (0, 2):
        d = unfold(v[..., c]) if mode == 2 else v[..., c]
        out[..., c] = (d + v[..., 1]) & 0xFF
    return out.astype(np.uint8)
