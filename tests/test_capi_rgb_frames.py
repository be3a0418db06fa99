"""bic_encode_rgb_frames / bic_encode_rgb_frames_packed / bic_decode_rgb_frames exist at every layer (CPU only:
nothing runs on a device): declared in include/bic.h with the documented arguments and the output-order sentence,
exported by libbic.so with matching argtypes, listed in pybic.EXPORTS and bound as Context methods; and
pybic.rgb_frames_p00 is rgb_p00 per frame."""
import os
import re

import numpy as np
import pytest

import pybic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NARGS = {"bic_encode_rgb_frames": 18, "bic_encode_rgb_frames_packed": 21, "bic_decode_rgb_frames": 17}


def _header():
    return open(os.path.join(ROOT, "include", "bic.h")).read()


def _declarations():
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(bic_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src)}


@pytest.mark.parametrize("name", sorted(NARGS))
def test_declared_with_argument_count(name):
    decl = _declarations()
    assert name in decl, name
    args = [a.strip() for a in decl[name].split(",")]
    assert len(args) == NARGS[name], args
    assert args[0] == "bic_ctx* ctx"


def test_declared_argument_order():
    """the frame arguments stand where the gray-frame calls have them"""
    decl = _declarations()
    enc = [a.strip() for a in decl["bic_encode_rgb_frames_packed"].split(",")]
    assert enc[1:9] == ["const uint8_t* rgb", "size_t frame_stride", "int nframes", "size_t pitch", "size_t rows",
                        "size_t cols", "int plane0", "int nplanes"]
    assert enc[-1] == "uint64_t* row_index" and enc[15] == "uint64_t* off_golomb" and enc[19] == "uint64_t* off_eg"
    slots = [a.strip() for a in decl["bic_encode_rgb_frames"].split(",")]
    assert slots[:12] == enc[:12] and slots[-1] == "uint64_t* bits_eg"
    dec = [a.strip() for a in decl["bic_decode_rgb_frames"].split(",")]
    one = [a.strip() for a in decl["bic_decode_rgb"].split(",")]
    assert dec[7] == "int nframes" and dec[-1] == "size_t frame_stride"
    assert dec[:7] + dec[8:-1] == one  # bic_decode_rgb's arguments around them


def test_output_order_is_documented():
    flat = " ".join(re.sub(r"^ \* ?", "", _header(), flags=re.M).split())  # (the comment lines' leading " * ")
    assert "entry (f * 3 + c) * nplanes + k belongs to plane plane0 + k of channel c of frame f" in flat
    assert "bic_encode_rgb_frames_packed -> bic_decode_rgb_frames" in flat


@pytest.mark.parametrize("name", sorted(NARGS))
def test_exported_and_listed(name):
    lib = pybic.load()
    assert name in pybic.EXPORTS
    f = getattr(lib, name)  # AttributeError if libbic.so does not export it
    assert len(f.argtypes) == NARGS[name]


@pytest.mark.parametrize("method", ["encode_rgb_frames", "encode_rgb_frames_packed", "decode_rgb_frames"])
def test_bound_as_context_method(method):
    assert callable(getattr(pybic.Context, method, None)), method


@pytest.mark.parametrize("ct", [0, 1, 2])
@pytest.mark.parametrize("gcode", [0, 1])
@pytest.mark.parametrize("plane0,nplanes", [(0, 8), (2, 3)])
def test_rgb_frames_p00_is_rgb_p00_per_frame(ct, gcode, plane0, nplanes):
    pixels = [(255, 255, 255), (0, 0, 0), (0x12, 0xF3, 0x80), (0x80, 0x7F, 0x01), (1, 2, 3)]
    got = pybic.rgb_frames_p00(ct, gcode, pixels, plane0, nplanes)
    assert got.dtype == np.uint8 and got.shape == (len(pixels) * 3 * nplanes,)
    for f, px in enumerate(pixels):
        one = pybic.rgb_p00(ct, gcode, px, plane0, nplanes)
        assert np.array_equal(got[f * 3 * nplanes:(f + 1) * 3 * nplanes], one), (f, px)
    assert set(got.tolist()) <= {0, 1} and got.any()
    assert pybic.rgb_frames_p00(ct, gcode, [], plane0, nplanes).shape == (0,)
