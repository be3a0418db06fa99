"""The interleaved-RGB entry points are declared in include/bic.h, listed in pybic.EXPORTS and exported by
the library (CPU only: nothing is called)."""
import os
import re

import pytest

import pybic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"bic_encode_rgb": 16, "bic_encode_rgb_packed": 19, "bic_bitplanes_rgb": 9, "bic_planes_to_rgb": 9,
         "bic_decode_rgb": 15}


@pytest.mark.parametrize("name", sorted(NAMES))
def test_rgb_entry_point(name):
    src = open(os.path.join(ROOT, "include", "bic.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, src)
    assert m, f"{name} not declared in include/bic.h"
    assert len(m.group(1).split(",")) == NAMES[name]
    assert name in pybic.EXPORTS
    assert hasattr(pybic.load(), name)
    assert len(getattr(pybic.load(), name).argtypes) == NAMES[name]


def test_rgb_methods():
    for m in ("encode_rgb", "encode_rgb_packed", "bitplanes_rgb", "planes_to_rgb", "decode_rgb"):
        assert callable(getattr(pybic.Context, m))


def test_rgb_header_scope():
    """the header says what the calls cannot express"""
    flat = " ".join(open(os.path.join(ROOT, "include", "bic.h")).read().replace("*", " ").split())
    assert "maxval >= 256) are out of scope" in flat
