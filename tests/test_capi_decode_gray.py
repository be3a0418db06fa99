"""bic_decode_gray is declared in include/bic.h, listed in pybic.EXPORTS, exported by the library and
bound as pybic.Context.decode_gray (CPU only: nothing is called)."""
import os
import re

import pybic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    src = open(os.path.join(ROOT, "include", "bic.h")).read()
    return src, re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_decode_gray_entry_point():
    _, code = _header()
    m = re.search(r"\bint\s+bic_decode_gray\s*\(([^)]*)\)", code)
    assert m, "bic_decode_gray not declared in include/bic.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 17, args  # the signature the binding passes
    assert args[-4:] == ["int sample_bytes", "int big_endian", "void* gray", "size_t pitch"], args
    assert "bic_decode_gray" in pybic.EXPORTS
    assert hasattr(pybic.load(), "bic_decode_gray")
    assert len(pybic.load().bic_decode_gray.argtypes) == 17


def test_decode_gray_method():
    assert callable(getattr(pybic.Context, "decode_gray"))


def test_header_names_the_round_trip():
    """the comments of bic_encode_gray16 and bic_planes_to_gray name the one-call device round trip"""
    src, _ = _header()
    flat = re.sub(r"[\s*]+", " ", src)
    assert "bic_encode_gray16_packed -> bic_decode_gray" in flat
    assert "bic_encode_gray_packed -> bic_decode_gray" in flat
