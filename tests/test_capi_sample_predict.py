"""BIC_OPT_SAMPLE_PREDICT exists at every layer (CPU only: nothing is computed on a device): defined as 9 in
include/bic.h with the exactness rule and the list of calls that ignore it, bound as
pybic.Context.set_sample_predict with its constants, bic_gray_p00 agrees with the numpy reference the GPU tests
take their expected values from, and that reference is a bijection with the stated fold."""
import os
import re

import numpy as np
import pytest

import pybic
from graycode_ref import gray
from sample_predict_ref import fold, predict, unfold, unpredict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "bic.h")).read()


def test_option_defined_as_9():
    m = re.search(r"^#define\s+BIC_OPT_SAMPLE_PREDICT\s+(\d+)\s*$", _header(), re.M)
    assert m and int(m.group(1)) == 9
    # no other option shares the number
    nums = re.findall(r"^#define\s+BIC_OPT_\w+\s+(\d+)\s*$", _header(), re.M)
    assert sorted(nums) == sorted(set(nums)), nums
    for name, val in (("BIC_SP_NONE", 0), ("BIC_SP_LEFT", 1), ("BIC_SP_LEFT_FOLDED", 2)):
        m = re.search(r"^#define\s+%s\s+(\d+)\s*$" % name, _header(), re.M)
        assert m and int(m.group(1)) == val, name


def test_header_states_the_exactness_rule_and_the_ignoring_calls():
    text = " ".join(_header().replace("*", " ").split())
    block = text[text.index("BIC_OPT_SAMPLE_PREDICT:"):text.index("#define BIC_OPT_SAMPLE_PREDICT")]
    assert "The result is the image exactly when plane0 = 0 and nplanes = 8" in block
    assert "for any other range it is this formula" in block
    assert "v(i,-1) = 0 in every row of every frame" in block
    assert "equal those of the same call with the option off on the image T(img)" in block
    tail = block[block.index("Two-byte samples"):]
    for word in ("bic_bitplanes_u16", "bic_encode_gray16", "the RGB calls", "the PBM calls", "planes-only calls",
                 "ignore the option"):
        assert word in tail, word
    assert re.search(r"int\s+bic_gray_p00\(int sample_predict, int gray_code, uint8_t sample, int plane0, int nplanes,"
                     r"\s*uint8_t\*\s*p00\);", _header())


def test_pybic_names_exist():
    assert callable(getattr(pybic.Context, "set_sample_predict", None))
    assert (pybic.SP_NONE, pybic.SP_LEFT, pybic.SP_LEFT_FOLDED) == (0, 1, 2)
    assert pybic.OPT_SAMPLE_PREDICT == 9
    assert callable(pybic.gray_p00)
    assert "bic_gray_p00" in pybic.EXPORTS


def test_fold_values():
    d = np.array([0, -1, 1, -128, 127, -2], np.int8).view(np.uint8)
    assert list(fold(d)) == [0, 1, 2, 255, 254, 3]
    z = np.arange(256, dtype=np.uint8)
    assert np.array_equal(fold(unfold(z)), z) and np.array_equal(unfold(fold(z)), z)
    assert len(np.unique(fold(z))) == 256


@pytest.mark.parametrize("mode", [1, 2])
def test_reference_is_a_bijection_on_rows(mode):
    rng = np.random.default_rng(0x5A3 + mode)
    img = rng.integers(0, 256, (7, 3, 301), dtype=np.uint8)
    z = predict(img, mode)
    assert z.dtype == np.uint8 and z.shape == img.shape
    assert np.array_equal(unpredict(z, mode), img)
    assert np.array_equal(predict(unpredict(img, mode), mode), img)  # onto as well: any z is some row's T
    # column 0 has no left neighbour: it is its own difference, in every row of every frame
    assert np.array_equal(z[..., 0], fold(img[..., 0]) if mode == 2 else img[..., 0])
    # the definition, element by element on one row
    row = img[3, 1].astype(np.int64)
    d = (row - np.concatenate(([0], row[:-1]))) % 256
    want = d if mode == 1 else np.where(d < 128, 2 * d, 2 * (256 - d) - 1)
    assert np.array_equal(z[3, 1], want.astype(np.uint8))
    assert np.array_equal(predict(img, 0), img) and np.array_equal(unpredict(img, 0), img)


def test_gray_p00_agrees_with_the_reference():
    for mode in (0, 1, 2):
        for gc in (0, 1):
            for s in range(256):
                v = int(predict(np.array([[s]], np.uint8), mode)[0, 0])  # the first sample: no left neighbour
                if gc:
                    v = int(gray(np.uint8(v)))
                for plane0, n in ((0, 8), (2, 6), (3, 4), (7, 1), (0, 1)):
                    got = pybic.gray_p00(mode, gc, s, plane0, n)
                    assert got.dtype == np.uint8 and got.shape == (n,)
                    assert list(got) == [(v >> (plane0 + k)) & 1 for k in range(n)], (mode, gc, s, plane0, n)


def test_gray_p00_rejects_bad_arguments():
    lib = pybic.load()
    out = np.zeros(8, np.uint8)
    ok = lib.bic_gray_p00(2, 1, 200, 0, 8, out.ctypes.data)
    assert ok == pybic.BIC_OK
    for args in ((3, 0, 1, 0, 8), (-1, 0, 1, 0, 8), (0, 2, 1, 0, 8), (0, -1, 1, 0, 8), (0, 0, 1, -1, 8), (0, 0, 1, 0, 0),
                 (0, 0, 1, 0, 9), (0, 0, 1, 1, 8), (0, 0, 1, 8, 1)):
        assert lib.bic_gray_p00(*args, out.ctypes.data) == pybic.BIC_EINVAL, args
        with pytest.raises(pybic.BicError) as err:
            pybic.gray_p00(*args)
        assert err.value.code == pybic.BIC_EINVAL
    assert lib.bic_gray_p00(0, 0, 1, 0, 8, None) == pybic.BIC_EINVAL  # a NULL p00
