"""BIC_OPT_GRAY_CODE exists at every layer (CPU only: nothing is computed on a device): defined as 7 in
include/bic.h with the documented range rule, bound as pybic.Context.set_gray_code, and the numpy reference
the GPU tests take their expected values from is a bijection with the stated bit rule."""
import os
import re

import numpy as np

import pybic
from graycode_ref import gray, ungray

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "bic.h")).read()


def test_option_defined_as_7():
    m = re.search(r"^#define\s+BIC_OPT_GRAY_CODE\s+(\d+)\s*$", _header(), re.M)
    assert m and int(m.group(1)) == 7
    # no other option shares the number
    nums = re.findall(r"^#define\s+BIC_OPT_\w+\s+(\d+)\s*$", _header(), re.M)
    assert sorted(nums) == sorted(set(nums)), nums


def test_header_states_the_range_rule():
    text = " ".join(_header().split())
    assert "highest non-zero plane of G" in text
    assert "not invertible" in text


def test_context_method_exists():
    assert callable(getattr(pybic.Context, "set_gray_code", None))


def test_reference_round_trips_every_value():
    v = np.arange(65536, dtype=np.uint16)
    g = gray(v)
    assert g.dtype == np.uint16
    assert np.array_equal(ungray(g, 16), v)
    assert len(np.unique(g)) == 65536
    v8 = np.arange(256, dtype=np.uint8)
    assert np.array_equal(ungray(gray(v8), 8), v8)
    assert gray(v8).max() == 255
    # neighbours differ in one bit; 127 -> 128 flips one plane, not eight
    assert (np.array([bin(int(x)).count("1") for x in g[1:] ^ g[:-1]]) == 1).all()
    assert int(gray(np.uint8(127)) ^ gray(np.uint8(128))) == 0x80
    # bit 7 of a 16-bit sample's code is v7 ^ v8
    assert np.array_equal((g >> 7) & 1, ((v >> 7) ^ (v >> 8)) & 1)
    # bit b of the inverse = XOR of the code's bits k >= b
    acc = np.zeros_like(g)
    for b in range(15, -1, -1):
        acc ^= (g >> b) & 1
        assert np.array_equal((v >> b) & 1, acc), b
