"""bic_encode_gray_frames / bic_encode_gray_frames_packed / bic_decode_gray_frames exist at every layer (CPU
only: nothing is computed): declared in include/bic.h with the documented argument counts, exported by
libbic.so with matching argtypes, listed in pybic.EXPORTS and bound as Context methods."""
import os
import re

import pytest

import pybic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NARGS = {"bic_encode_gray_frames": 20, "bic_encode_gray_frames_packed": 23, "bic_decode_gray_frames": 19}


def _declarations():
    src = open(os.path.join(ROOT, "include", "bic.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(bic_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src)}


@pytest.mark.parametrize("name", sorted(NARGS))
def test_declared_with_argument_count(name):
    decl = _declarations()
    assert name in decl, name
    args = [a.strip() for a in decl[name].split(",")]
    assert len(args) == NARGS[name], args
    assert args[0] == "bic_ctx* ctx"


def test_declared_argument_order():
    """the frame arguments stand where the issue puts them"""
    decl = _declarations()
    enc = [a.strip() for a in decl["bic_encode_gray_frames_packed"].split(",")]
    assert enc[1:11] == ["const void* gray", "size_t frame_stride", "int nframes", "size_t pitch", "size_t rows",
                         "size_t cols", "int sample_bytes", "int big_endian", "int plane0", "int nplanes"]
    assert enc[-1] == "uint64_t* row_index" and enc[17] == "uint64_t* off_golomb" and enc[21] == "uint64_t* off_eg"
    dec = [a.strip() for a in decl["bic_decode_gray_frames"].split(",")]
    assert dec[7:10] == ["int nframes", "int plane0", "int nplanes"]
    assert dec[-3:] == ["void* gray", "size_t pitch", "size_t frame_stride"]


@pytest.mark.parametrize("name", sorted(NARGS))
def test_exported_and_listed(name):
    lib = pybic.load()
    assert name in pybic.EXPORTS
    f = getattr(lib, name)  # AttributeError if libbic.so does not export it
    assert len(f.argtypes) == NARGS[name]


@pytest.mark.parametrize("method", ["encode_gray_frames", "encode_gray_frames_packed", "decode_gray_frames"])
def test_bound_as_context_method(method):
    assert callable(getattr(pybic.Context, method, None)), method


def test_documents_name_the_round_trip():
    flat = " ".join(open(os.path.join(ROOT, "INTEGRATION.md")).read().split())
    assert "bic_encode_gray_frames_packed -> bic_decode_gray_frames" in flat
