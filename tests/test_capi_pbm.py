"""bic_encode_pbm / bic_encode_pbm_packed / bic_decode_pbm exist at every layer (CPU only: nothing is
computed): declared in include/bic.h with the documented argument counts, exported by libbic.so, listed
in pybic.EXPORTS and bound as Context methods."""
import os
import re

import pytest

import pybic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NARGS = {"bic_encode_pbm": 15, "bic_encode_pbm_packed": 18, "bic_decode_pbm": 14}


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


@pytest.mark.parametrize("name", sorted(NARGS))
def test_exported_and_listed(name):
    lib = pybic.load()
    assert name in pybic.EXPORTS
    f = getattr(lib, name)  # AttributeError if libbic.so does not export it
    assert len(f.argtypes) == NARGS[name]


@pytest.mark.parametrize("method", ["encode_pbm", "encode_pbm_packed", "decode_pbm"])
def test_bound_as_context_method(method):
    assert callable(getattr(pybic.Context, method, None)), method


def test_header_states_the_contracts():
    """the header says what p00 is and that no chunk beyond a frame's raster is read"""
    src = open(os.path.join(ROOT, "include", "bic.h")).read()
    src = " ".join(re.sub(r"\n \* ?", "\n", src).split())  # comment text without its line starts
    assert "p00[f] = raster_f[0] >> 7" in src
    assert "never a chunk without one of the frame's raster bytes" in src
