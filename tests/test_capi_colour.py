"""BIC_OPT_COLOR_TRANSFORM at every layer that needs no device: defined as 8 in include/bic.h, bound as
pybic.Context.set_color_transform; the numpy reference the GPU tests take their expected values from
(colour_ref.py) is a bijection with the stated fold; bic_rgb_p00 (host code of the library) agrees with it; and
the size claim that motivates the option holds on the oracle's bit counts."""
import os
import re

import numpy as np
import pytest

import pybic
from colour_ref import fold, forward, inverse, unfold
from graycode_ref import gray

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "bic.h")).read()


def test_option_defined_as_8():
    h = _header()
    m = re.search(r"^#define\s+BIC_OPT_COLOR_TRANSFORM\s+(\d+)\s*$", h, re.M)
    assert m and int(m.group(1)) == 8
    nums = re.findall(r"^#define\s+BIC_OPT_\w+\s+(\d+)\s*$", h, re.M)
    assert sorted(nums) == sorted(set(nums)), nums  # no other option shares the number
    for name, val in (("BIC_CT_NONE", 0), ("BIC_CT_SUBTRACT_GREEN", 1), ("BIC_CT_SUBTRACT_GREEN_FOLDED", 2)):
        m = re.search(r"^#define\s+%s\s+(\d+)\s*$" % name, h, re.M)
        assert m and int(m.group(1)) == val, name
    assert (pybic.OPT_COLOR_TRANSFORM, pybic.CT_NONE, pybic.CT_SUBTRACT_GREEN, pybic.CT_SUBTRACT_GREEN_FOLDED) == (8, 0, 1, 2)
    assert callable(getattr(pybic.Context, "set_color_transform", None))


def test_header_states_the_range_rule():
    text = " ".join(_header().replace("*", " ").split())
    assert "exactly when plane0 = 0 and nplanes = 8" in text
    assert "all eight bits of the result are written" in text


def test_rgb_p00_declared_and_exported():
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"\bint\s+bic_rgb_p00\s*\(([^)]*)\)", src)
    assert m and len(m.group(1).split(",")) == 6
    assert "bic_rgb_p00" in pybic.EXPORTS and hasattr(pybic.load(), "bic_rgb_p00")
    assert callable(pybic.rgb_p00)


def _all_rg():
    r, g = np.mgrid[0:256, 0:256]
    return np.stack([r, g, (r * 7 + g * 13 + 5) & 0xFF], axis=2).astype(np.uint8)


@pytest.mark.parametrize("mode", [1, 2])
def test_reference_round_trips_every_pair(mode):
    img = _all_rg()  # all 65,536 (R, G) pairs; B runs through every (B, G) pair too (7 is odd)
    t = forward(img, mode)
    assert t.dtype == np.uint8 and t.shape == img.shape
    assert np.array_equal(t[..., 1], img[..., 1])  # G is unchanged
    assert np.array_equal(inverse(t, mode), img)
    for c in (0, 2):  # a bijection on (channel, G)
        assert len(np.unique(t[..., c].astype(np.int64) * 256 + t[..., 1])) == 65536
    assert np.array_equal(forward(img, 0), img) and np.array_equal(inverse(img, 0), img)


def test_fold_examples():
    assert [int(fold(d)) for d in (0, -1, 1, -128)] == [0, 1, 2, 255]
    d = np.arange(-128, 128)
    assert sorted(fold(d).tolist()) == list(range(256))
    assert np.array_equal(unfold(fold(d)), d)
    assert (fold(np.arange(-3, 4)) <= 6).all()
    # through forward(): R - G = d for |d| <= 3 gives a mode 2 sample <= 6, whatever G
    g = np.arange(256)
    for dd in range(-3, 4):
        img = np.stack([(g + dd) & 0xFF, g, (g - dd) & 0xFF], axis=1).astype(np.uint8)
        t = forward(img, 2)
        assert t[:, 0].max() <= 6 and t[:, 2].max() <= 6
        assert (forward(img, 1)[:, 0] == (dd & 0xFF)).all()


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("gc", [0, 1])
@pytest.mark.parametrize("plane0,nplanes", [(0, 8), (3, 2), (7, 1)])
def test_rgb_p00_matches_the_reference(mode, gc, plane0, nplanes):
    rng = np.random.default_rng(0xC0105 + 16 * mode + gc)
    px = rng.integers(0, 256, (32, 3)).astype(np.uint8)
    px[:4] = [(0, 255, 255), (255, 0, 0), (128, 0, 127), (0, 128, 255)]  # borrow and fold extremes
    t = forward(px, mode)
    if gc:
        t = gray(t)
    for p, v in zip(px, t):
        want = [(int(v[c]) >> (plane0 + k)) & 1 for c in range(3) for k in range(nplanes)]
        got = pybic.rgb_p00(mode, gc, p, plane0, nplanes)
        assert got.dtype == np.uint8 and got.tolist() == want, (p, mode, gc)


def test_rgb_p00_rejects():
    for args in ((3, 0, (1, 2, 3), 0, 8), (-1, 0, (1, 2, 3), 0, 8), (1, 2, (1, 2, 3), 0, 8), (1, 0, (1, 2, 3), -1, 2),
                 (1, 0, (1, 2, 3), 0, 0), (1, 0, (1, 2, 3), 1, 8), (2, 1, (1, 2, 3), 8, 1), (0, 0, (1, 2, 3), 0, 9)):
        with pytest.raises(pybic.BicError) as e:
            pybic.rgb_p00(*args)
        assert e.value.code == pybic.BIC_EINVAL, args
    out = np.zeros(24, np.uint8)
    assert pybic.load().bic_rgb_p00(1, 0, None, 0, 8, out.ctypes.data) == pybic.BIC_EINVAL
    assert pybic.load().bic_rgb_p00(1, 0, bytes([1, 2, 3]), 0, 8, None) == pybic.BIC_EINVAL


def test_size_claim(oracle):
    """the motivation, on the oracle alone (predict = 1, Golomb, summed over the 24 planes): subtract-green with
    the Gray code codes the synthetic luminance image in fewer bits than the Gray code alone, and the folded
    form without the Gray code in fewer than no transform without it"""
    rows, cols = 96, 1024
    i, j = np.mgrid[0:rows, 0:cols]
    n = oracle.gen_bytes(0x434C5200, 3 * rows * cols).reshape(3, rows, cols).astype(np.int64)
    Y = (40 + (3 * i) // 2 + j // 5 + 30 * np.sin(j / 37) + 20 * np.cos(i / 11)).astype(np.int64)
    R = np.clip(Y + (6 * np.sin(i / 9 + j / 50)).astype(np.int64) + n[0] % 3 - 1, 0, 255)
    G = np.clip(Y + n[1] % 3, 0, 255)
    B = np.clip(Y + (5 * np.cos(i / 13 - j / 70)).astype(np.int64) + n[2] % 3 - 1, 0, 255)
    img = np.stack([R, G, B], axis=2).astype(np.uint8)

    def bits(mode, gc):
        v = forward(img, mode)
        if gc:
            v = gray(v)
        total = 0
        for c in range(3):
            P = oracle.bitplanes(np.ascontiguousarray(v[:, :, c]), 8)
            total += sum(oracle.encode_plane(P[k], cols, 1, 0, want_stream=False)[0] for k in range(8))
        return total

    got = {(m, gc): bits(m, gc) for m in (0, 1, 2) for gc in (0, 1)}
    print(got)
    assert got[(1, 1)] < got[(0, 1)]
    assert got[(2, 0)] < got[(0, 0)]
