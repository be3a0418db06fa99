"""BIC_OPT_RGB_PREDICT exists at every layer (CPU only: nothing is computed on a device): defined as 10 in
include/bic.h with the exactness rule and the list of which calls ignore which option, bound as
pybic.Context.set_rgb_predict, bic_rgb_p00_predict agrees with the numpy reference the GPU tests take their expected
values from and with bic_rgb_p00 at mode 0, and that reference round-trips."""
import os
import re

import numpy as np
import pytest

import colour_ref
import pybic
import rgb_predict_ref
from graycode_ref import gray
from sample_predict_ref import fold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "bic.h")).read()


def test_option_defined_as_10():
    h = _header()
    m = re.search(r"^#define\s+BIC_OPT_RGB_PREDICT\s+(\d+)\s*$", h, re.M)
    assert m and int(m.group(1)) == 10
    nums = re.findall(r"^#define\s+BIC_OPT_\w+\s+(\d+)\s*$", h, re.M)
    assert sorted(nums) == sorted(set(nums)), nums  # no other option shares the number
    # behind option 9's define, whose block stays where it was
    assert h.index("#define BIC_OPT_RGB_PREDICT") > h.index("#define BIC_OPT_SAMPLE_PREDICT 9")
    assert h.index("BIC_OPT_RGB_PREDICT:") > h.index("#define BIC_OPT_SAMPLE_PREDICT 9")


def test_header_states_the_exactness_rule_and_who_ignores_what():
    text = " ".join(_header().replace("*", " ").split())
    block = text[text.index("BIC_OPT_RGB_PREDICT:"):text.index("#define BIC_OPT_RGB_PREDICT")]
    assert "The result is the image exactly when plane0 = 0 and nplanes = 8" in block
    assert "for any other range it is this formula" in block
    assert "c'(i,-1) = 0 in every row of every frame" in block
    assert "with options 8 and 10 both off on the image U(img) = T_sp(T_ct(img))" in block
    for name in ("bic_encode_rgb", "bic_encode_rgb_packed", "bic_bitplanes_rgb", "bic_encode_rgb_frames",
                 "bic_encode_rgb_frames_packed", "bic_planes_to_rgb", "bic_decode_rgb", "bic_decode_rgb_frames",
                 "BIC_SP_NONE", "BIC_SP_LEFT", "BIC_SP_LEFT_FOLDED", "BIC_EINVAL"):
        assert name in block, name
    assert "Use mode 2 with BIC_CT_NONE or BIC_CT_SUBTRACT_GREEN" in block
    assert "The gray, 16-bit, PBM and planes-only calls ignore option 10; the RGB calls ignore option 9" in block
    assert re.search(r"int\s+bic_rgb_p00_predict\(int color_transform, int rgb_predict, int gray_code, "
                     r"const uint8_t pixel\[3\], int plane0,\s*int nplanes, uint8_t\*\s*p00\);", _header())
    # bic_rgb_p00 keeps its signature
    assert re.search(r"int\s+bic_rgb_p00\(int color_transform, int gray_code, const uint8_t pixel\[3\], int plane0, "
                     r"int nplanes, uint8_t\*\s*p00\);", _header())


def test_pybic_names_exist():
    assert pybic.OPT_RGB_PREDICT == 10
    assert callable(getattr(pybic.Context, "set_rgb_predict", None))
    assert callable(pybic.rgb_p00_predict)
    assert "bic_rgb_p00_predict" in pybic.EXPORTS
    assert hasattr(pybic.load(), "bic_rgb_p00_predict")


_PIXELS = [(0, 0, 0), (255, 255, 255), (255, 0, 255), (0, 255, 0), (128, 0, 127), (1, 129, 2), (200, 100, 50),
           (17, 18, 16), (127, 255, 128)]


def test_rgb_p00_predict_agrees_with_the_reference():
    rng = np.random.default_rng(0x10A)
    pixels = _PIXELS + [tuple(int(x) for x in p) for p in rng.integers(0, 256, (40, 3))]
    for mode in (0, 1, 2):
        for ct in (0, 1, 2):
            for gc in (0, 1):
                for px in pixels:
                    # a one-pixel image: the first pixel has no left neighbour
                    v = rgb_predict_ref.forward(np.array([[px]], np.uint8), ct, mode)[0, 0]
                    t = colour_ref.forward(np.array([[px]], np.uint8), ct)[0, 0]
                    assert np.array_equal(v, fold(t) if mode == 2 else t)
                    if gc:
                        v = gray(v)
                    for plane0, n in ((0, 8), (3, 4)):
                        got = pybic.rgb_p00_predict(ct, mode, gc, px, plane0, n)
                        assert got.dtype == np.uint8 and got.shape == (3 * n,)
                        want = [(int(v[c]) >> (plane0 + k)) & 1 for c in range(3) for k in range(n)]
                        assert list(got) == want, (mode, ct, gc, px, plane0, n)


def test_rgb_p00_predict_equals_rgb_p00_at_mode_0():
    for ct in (0, 1, 2):
        for gc in (0, 1):
            for px in _PIXELS:
                for plane0, n in ((0, 8), (2, 5), (7, 1)):
                    assert np.array_equal(pybic.rgb_p00_predict(ct, 0, gc, px, plane0, n),
                                          pybic.rgb_p00(ct, gc, px, plane0, n)), (ct, gc, px, plane0, n)


def test_rgb_p00_predict_rejects_bad_arguments():
    lib = pybic.load()
    out = np.zeros(24, np.uint8)
    px = bytes([1, 2, 3])
    assert lib.bic_rgb_p00_predict(2, 2, 1, px, 0, 8, out.ctypes.data) == pybic.BIC_OK
    for args in ((0, 3, 0, px, 0, 8), (0, -1, 0, px, 0, 8), (3, 0, 0, px, 0, 8), (-1, 0, 0, px, 0, 8),
                 (0, 0, 2, px, 0, 8), (0, 0, -1, px, 0, 8), (0, 0, 0, px, -1, 8), (0, 0, 0, px, 0, 0),
                 (0, 0, 0, px, 0, 9), (0, 0, 0, px, 1, 8), (0, 0, 0, px, 8, 1), (0, 0, 0, None, 0, 8)):
        assert lib.bic_rgb_p00_predict(*args, out.ctypes.data) == pybic.BIC_EINVAL, args
    assert lib.bic_rgb_p00_predict(0, 0, 0, px, 0, 8, None) == pybic.BIC_EINVAL  # a NULL p00
    for args in ((0, 3, 0, (1, 2, 3)), (3, 0, 0, (1, 2, 3)), (0, 0, 2, (1, 2, 3)), (0, 0, 0, (1, 2))):
        with pytest.raises(pybic.BicError) as err:
            pybic.rgb_p00_predict(*args)
        assert err.value.code == pybic.BIC_EINVAL


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("ct", [0, 1, 2])
def test_reference_round_trips(ct, mode):
    rng = np.random.default_rng(0xB1C + 3 * ct + mode)
    img = rng.integers(0, 256, (2, 5, 301, 3), dtype=np.uint8)
    z = rgb_predict_ref.forward(img, ct, mode)
    assert z.dtype == np.uint8 and z.shape == img.shape
    assert np.array_equal(rgb_predict_ref.inverse(z, ct, mode), img)
    assert np.array_equal(rgb_predict_ref.forward(rgb_predict_ref.inverse(img, ct, mode), ct, mode), img)  # onto
    # the definition, element by element: one row of one channel (G is differenced too)
    t = colour_ref.forward(img, ct).astype(np.int64)
    for c in range(3):
        row = t[1, 3, :, c]
        d = (row - np.concatenate(([0], row[:-1]))) % 256
        want = d if mode == 1 else np.where(d < 128, 2 * d, 2 * (256 - d) - 1) if mode == 2 else row
        assert np.array_equal(z[1, 3, :, c], want.astype(np.uint8)), c
    if mode == 0:
        assert np.array_equal(z, colour_ref.forward(img, ct))
