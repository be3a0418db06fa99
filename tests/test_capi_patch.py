"""The image-mode entries exist at every layer (CPU only: nothing is computed on a device): declared in
include/bic.h with the documented argument counts, exported by libbic.so, listed in pybic.EXPORTS, bound as Context
methods and behind the C++ bridge; bic_mosaic_dims works on the host; the header states the flat read, the padding
decisions and the difference from set_submatrix; DESIGN.md no longer lists patch vectorisation as not built."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

import pybic
from conftest import PKG, ROOT

NARGS = {"bic_patches_gather": 8, "bic_patches_scatter": 8, "bic_mosaic_dims": 4, "bic_mosaic": 7,
         "bic_bsvd_learn_image": 23}


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
    assert args[0] == ("size_t n" if name == "bic_mosaic_dims" else "bic_ctx* ctx")


def test_signatures():
    decl = {k: [a.strip() for a in v.split(",")] for k, v in _declarations().items()}
    assert decl["bic_patches_gather"][1:] == ["const uint64_t* plane", "size_t rows", "size_t cols", "size_t wpr",
                                              "unsigned W", "uint64_t* X", "size_t x_wpr"]
    assert decl["bic_patches_scatter"][1:] == ["const uint64_t* X", "size_t x_wpr", "unsigned W", "uint64_t* plane",
                                               "size_t rows", "size_t cols", "size_t wpr"]
    assert decl["bic_mosaic_dims"] == ["size_t n", "size_t m", "size_t* rows", "size_t* cols"]
    assert decl["bic_mosaic"][1:] == ["const uint64_t* D", "size_t n", "size_t m", "size_t d_wpr", "uint64_t* image",
                                      "size_t i_wpr"]
    li = decl["bic_bsvd_learn_image"]
    assert li[1:9] == ["int mi", "int lm", "int du", "const uint64_t* plane", "size_t rows", "size_t cols",
                       "size_t wpr", "unsigned W"]
    assert li[9:18] == ["uint64_t* X", "size_t x_wpr", "uint64_t* E", "size_t e_wpr", "uint64_t* D", "size_t p",
                        "size_t d_wpr", "uint64_t* A", "size_t a_wpr"]
    assert li[18:] == ["uint64_t* rng_state", "size_t max_iter", "size_t* iters", "uint64_t* residual", "size_t r_wpr"]


@pytest.mark.parametrize("name", sorted(NARGS))
def test_exported_and_listed(name):
    lib = pybic.load()
    assert name in pybic.EXPORTS
    f = getattr(lib, name)  # AttributeError if libbic.so does not export it
    assert len(f.argtypes) == NARGS[name]


@pytest.mark.parametrize("method", ["patches_gather", "patches_scatter", "mosaic_dims", "mosaic", "bsvd_learn_image"])
def test_bound_as_context_method(method):
    assert callable(getattr(pybic.Context, method, None)), method


def test_python_signatures():
    sig = {m: list(inspect.signature(getattr(pybic.Context, m)).parameters)[1:]
           for m in ("patches_gather", "patches_scatter", "mosaic_dims", "mosaic")}
    assert sig == {"patches_gather": ["plane", "cols", "W", "out"], "patches_scatter": ["X", "W", "rows", "cols", "out"],
                   "mosaic_dims": ["n", "m"], "mosaic": ["D", "m", "out"]}
    par = inspect.signature(pybic.Context.bsvd_learn_image).parameters
    assert (par["mi"].default, par["lm"].default, par["du"].default, par["residual"].default) == (0, 0, 0, None)


@pytest.mark.parametrize("n,m,dims", [(1, 1, (2, 2)), (5, 25, (12, 18)), (7, 70, (27, 27)), (512, 256, (391, 391)),
                                      (3, 4500, (136, 136))])
def test_mosaic_dims_on_the_host(n, m, dims):
    f = pybic.load().bic_mosaic_dims
    r, c = C.c_size_t(0), C.c_size_t(0)
    assert f(n, m, C.byref(r), C.byref(c)) == pybic.BIC_OK
    assert (r.value, c.value) == dims


def test_mosaic_dims_domain():
    f = pybic.load().bic_mosaic_dims
    r, c = C.c_size_t(7), C.c_size_t(7)
    for n, m in ((0, 4), (4, 0), (4, 1048577), (1 << 31, 4)):
        assert f(n, m, C.byref(r), C.byref(c)) == pybic.BIC_EINVAL, (n, m)
    assert f(4, 4, None, C.byref(c)) == pybic.BIC_EINVAL and f(4, 4, C.byref(r), None) == pybic.BIC_EINVAL
    assert (r.value, c.value) == (7, 7)
    assert f(4, 1048576, C.byref(r), C.byref(c)) == pybic.BIC_OK and (r.value, c.value) == (2050, 2050)


def test_header_states_the_reads_and_the_padding():
    src = " ".join(re.sub(r"\n \* ?", "\n", _header()).split())  # comment text without its line starts
    i = src.index("image mode (bsvd_test.cpp:78-151, util.cpp:53-82)")
    own = src[i:src.index("int bic_patches_gather(")]
    assert "is the plane's FLAT bit at row ti W + r, column tj W + c" in own
    assert "the word after them is the next row's first word" in own
    assert "pad bits of a row's last word are read as stored" in own
    assert "anything past the last row reads 0" in own
    assert "words between ceil(cols/64) and wpr are never read" in own
    assert "first ceil(W^2/64) words of every row of X are written, with pad bits 0" in own
    assert "the plane is written, never read" in own
    assert "first ceil(cols/64) words of every row, with pad bits 0; the pitch words are left untouched" in own
    assert "set_submatrix leaves an edge tile's bits in the pad columns it covers" in own
    assert "this build writes zero padding, as the learners do" in own
    assert "every other bit of the rows' own words, pad bits included, is 0" in own
    assert "bits w^2 .. m - 1 of an atom are ignored" in own
    assert "integer arithmetic gives what the reference's" in own
    assert "1 <= W <= 1024" in own and "1 <= m <= 1048576" in own and "BIC_EINVAL before any launch" in own
    assert "no workgroup ever waits for another" in own
    assert "bit for bit those of the five separate calls, *rng_state and *iters included" in own
    assert "W <= 64 (the initialisers take m <= 4096)" in own and "adds no kernel of its own" in own


def test_bridge_defines_the_device_methods():
    lib = os.path.join(PKG, "lib", "libbicpp.so")
    if not os.path.exists(lib):
        subprocess.run(["make", "-C", PKG], check=True, stdout=subprocess.DEVNULL)
    syms = subprocess.run(["nm", "-DC", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    defined = {line.split(" ", 2)[2] for line in syms.splitlines() if line.count(" ") >= 2}
    want = ["bic::Device::patches(binary_matrix const&, unsigned int, binary_matrix&)",
            "bic::Device::unpatch(binary_matrix const&, unsigned int, binary_matrix&)",
            "bic::Device::mosaic(binary_matrix const&, binary_matrix&)",
            "bic::Device::bsvd_learn_image(int, int, int, binary_matrix const&, unsigned int, unsigned long, "
            "binary_matrix&, binary_matrix&, binary_matrix&, binary_matrix&, unsigned long*, unsigned long, "
            "unsigned long*, binary_matrix*)",
            "render_mosaic(binary_matrix const&, char const*)"]  # the host parity basis stays
    missing = [s for s in want if s not in defined]
    assert not missing, missing


def test_makefile_lists_the_new_objects():
    mk = open(os.path.join(PKG, "Makefile")).read()
    common = mk[mk.index("COMMON_OBJS :="):mk.index("LIB_OBJS :=")]
    assert "build/bic_patch.o" in common and "build/bic_capi_patch.o" in common


def test_design_no_longer_lists_patch_vectorisation_as_missing():
    doc = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "patch vectorisation on the device" not in doc
    sec8 = doc[doc.index("\n## 8"):]
    for piece in ("Overlapping patches", "bic_pbm_unpack", "one-call form of the MDL searches", "W > 64"):
        assert piece in sec8, piece
    assert "Image mode" in doc and "profiles/r17/time_bsvd_image.jsonl" in doc
