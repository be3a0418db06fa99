"""The binary-reflected Gray code of BIC_OPT_GRAY_CODE in numpy: gray(v) = v ^ (v >> 1) on the whole sample,
ungray(g, width) its inverse (bit b of v = XOR of the bits k >= b of g). Plain integer arithmetic on
the samples: nothing here knows of planes, bytes or byte orders."""
import numpy as np


def gray(v):
    v = np.asarray(v)
    return v ^ (v >> 1)


def ungray(g, width):
    """the inverse of gray() on `width`-bit values: v = g ^ (g >> 1) ^ (g >> 2) ^ ... (shifts doubled)"""
    v = np.array(g, copy=True)
    s = 1
    while s < width:
        v ^= v >> s
        s *= 2
    return v
