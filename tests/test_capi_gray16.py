"""The 16-bit gray entry points are declared in include/bic.h, listed in pybic.EXPORTS and exported by
the library (CPU only: nothing is called)."""
import os
import re

import pytest

import pybic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bic_encode_gray16", "bic_encode_gray16_packed", "bic_bitplanes_u16")


@pytest.mark.parametrize("name", NAMES)
def test_gray16_entry_point(name):
    src = open(os.path.join(ROOT, "include", "bic.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(" % name, src), f"{name} not declared in include/bic.h"
    assert name in pybic.EXPORTS
    assert hasattr(pybic.load(), name)


def test_gray16_methods():
    for m in ("encode_gray16", "encode_gray16_packed", "bitplanes_u16"):
        assert callable(getattr(pybic.Context, m))
