"""The MDL model-order entries exist at every layer (CPU only: nothing is computed on a device): declared in
include/bic.h with the documented argument counts, exported by libbic.so, listed in pybic.EXPORTS, bound as Context
methods, behind the C++ bridge and include/bsvd.h; and the header states the domain, the zero-padding decision and
each kept slip of bsvd.cpp:1438-1717."""
import inspect
import math
import os
import re
import subprocess

import pytest

import bsvd_mdl_ref as M
import pybic
from conftest import PKG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NARGS = {"bic_bsvd_model_weights": 13, "bic_bsvd_drop_weights": 11, "bic_bsvd_drop_atom": 9,
         "bic_bsvd_append_atom": 12, "bic_bsvd_model_codelength": 11, "bic_bsvd_learn_mdl": 23}


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


def test_signatures():
    decl = _declarations()
    lm = [a.strip() for a in decl["bic_bsvd_learn_mdl"].split(",")]
    assert lm[1:6] == ["int search", "int lmi", "int du", "int mi", "const uint64_t* X"]
    assert lm[12:15] == ["size_t p", "size_t p_cap", "size_t d_wpr"]
    assert lm[17:] == ["uint64_t* rng_state", "size_t* p_out", "uint64_t* best_len", "bic_bsvd_mdl_step* trace",
                       "size_t trace_cap", "size_t* trace_len"]
    assert [a.strip() for a in decl["bic_bsvd_model_weights"].split(",")][-3:] == ["uint64_t* we", "uint32_t* wd",
                                                                                  "uint32_t* wa"]
    assert decl["bic_bsvd_drop_atom"].split(",")[-1].strip() == "size_t k"
    assert re.search(r"\bdouble\s+bic_universal_codelength\s*\(unsigned n, unsigned r\)\s*;", _header())
    # the entries the searches stand on are declared as before
    assert len(decl["bic_bsvd_learn_lm"].split(",")) == 16 and len(decl["bic_bsvd_initialize"].split(",")) == 12


def test_constants_and_the_trace_record():
    src = _header()
    for i, name in enumerate(("FORWARD", "BACKWARD", "FULL")):
        assert re.search(r"#define\s+BIC_BSVD_MDL_%s\s+%d\b" % (name, i), src), name
    assert (pybic.BSVD_MDL_FORWARD, pybic.BSVD_MDL_BACKWARD, pybic.BSVD_MDL_FULL) == (0, 1, 2)
    rec = re.search(r"typedef struct bic_bsvd_mdl_step \{(.*?)\} bic_bsvd_mdl_step;", src, re.S).group(1)
    rec = re.sub(r"/\*.*?\*/", "", rec, flags=re.S)
    fields = [f.strip() for f in rec.split(";") if f.strip()]
    assert fields == ["uint64_t K, currL, bestK, bestL, stuck", "int32_t dif, dev", "uint32_t atom",
                      "uint32_t reserved", "uint64_t lens[10]"]
    assert [f[0] for f in pybic.MdlStep._fields_] == ["K", "currL", "bestK", "bestL", "stuck", "dif", "dev", "atom",
                                                      "reserved", "lens"]
    assert pybic.C.sizeof(pybic.MdlStep) == 5 * 8 + 4 * 4 + 10 * 8


@pytest.mark.parametrize("name", sorted(NARGS) + ["bic_universal_codelength"])
def test_exported_and_listed(name):
    lib = pybic.load()
    assert name in pybic.EXPORTS
    f = getattr(lib, name)  # AttributeError if libbic.so does not export it
    assert len(f.argtypes) == NARGS.get(name, 2)


@pytest.mark.parametrize("method", ["bsvd_model_weights", "bsvd_drop_weights", "bsvd_drop_atom", "bsvd_append_atom",
                                    "bsvd_model_codelength", "bsvd_learn_mdl"])
def test_bound_as_context_method(method):
    assert callable(getattr(pybic.Context, method, None)), method


def test_python_signatures():
    par = inspect.signature(pybic.Context.bsvd_learn_mdl).parameters
    assert list(par)[1:8] == ["search", "X", "E", "m", "D", "A", "p"]
    assert (par["lmi"].default, par["du"].default, par["mi"].default, par["state"].default) == (0, 0, 0, None)
    assert list(inspect.signature(pybic.Context.bsvd_drop_atom).parameters)[1:] == ["D", "m", "A", "p", "k"]


def test_universal_codelength_is_one_formula():
    """the helper behind bic_bsvd_model_codelength and coding.h's universal_codelength is the restatement's, bit for
    bit (host only)"""
    f = pybic.load().bic_universal_codelength
    for n, r in [(16, 4), (64, 0), (64, 64), (64, 70), (19200, 2345), (300, 1), (100, 99), (1 << 20, 12345), (4, 2)]:
        assert f(n, r) == M.universal_codelength(n, r), (n, r)
    assert f(16, 4) == 16 * (-0.25 * math.log2(0.25) - 0.75 * math.log2(0.75)) + 2.0


def test_header_states_the_domain_the_padding_and_the_slips():
    src = " ".join(re.sub(r"\n \* ?", "\n", _header()).split())  # comment text without its line starts
    i = src.index("MDL model order (bsvd.cpp:1438-1717)")
    own = src[i:src.index("int bic_bsvd_learn_mdl(")]
    assert "Domain: 1 <= m <= 1048576, 0 <= p <= 4096, 1 <= n < 2^31" in own
    assert "1 <= p <= p_cap <= 4096; m <= 4096 where an initialiser runs" in own
    assert "1 <= n, m <= 1048576 for lmi >= 1" in own
    assert "masked at the row's trailing word" in own and "dirty padding bits never count" in own
    assert "Words past a row's own are neither read nor written" in own
    assert "No workgroup ever waits for another".lower() in own.lower() and "run-to-run identical" in own
    assert "reference's padding is uninitialised memory; this build defines it as zero" in own
    assert "all padding bits inside the row's ceil(p/64) words become 0" in own
    assert "truncated to 32 bits" in own and "truncate toward zero on every term" in own
    assert "sumStuck += currL - bestL wraps" in own and "sign-extended in currL + dev < bestL" in own
    assert "grows every pass, accepted or not" in own and "BIC_ENOSPC" in own
    assert "the BEST model's residual and not the current one's" in own
    assert "the smallest k at the minimum wins (strict <)" in own and "0xFFFFFFFFFFFFFF7F" in own
    assert "shrinks every pass, accepted or not" in own
    assert "*best_len keeps its previous value (the break precedes the assignment)" in own
    assert "is the LAST repetition's, not the minimum's" in own and "bestL starts at 1 << 30" in own
    assert "p < 20 leaves E, D and A untouched, *p_out = 0 and *best_len = 1 << 30" in own
    assert "the generator is seeded once" in own
    assert "*trace_len is the number of passes run, even when trace_cap is smaller" in own


def test_bridge_exports_the_reference_functions():
    lib = os.path.join(PKG, "lib", "libbicpp.so")
    if not os.path.exists(lib):
        subprocess.run(["make", "-C", PKG], check=True, stdout=subprocess.DEVNULL)
    syms = subprocess.run(["nm", "-DC", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    defined = {line.split(" ", 2)[2] for line in syms.splitlines() if line.count(" ") >= 2}
    four = "(binary_matrix&, binary_matrix&, binary_matrix&, binary_matrix&)"
    want = ["learn_model_mdl_forward_selection" + four, "learn_model_mdl_backward_selection" + four,
            "learn_model_mdl_full_search" + four,
            "model_codelength(binary_matrix const&, binary_matrix const&, binary_matrix const&)",
            "learn_model_setup(int, int, int, int, int)", "learn_model", "learn_model_inner",
            "mi_algorithm_names", "cu_algorithm_names", "du_algorithm_names", "lm_algorithm_names",
            "bic::Device::bsvd_model_codelength(binary_matrix const&, binary_matrix const&, binary_matrix const&, "
            "unsigned long*)",
            "bic::Device::bsvd_learn_mdl(int, int, int, int, binary_matrix&, binary_matrix&, binary_matrix&, "
            "binary_matrix&, unsigned long*, bic::Device::MdlResult*, unsigned long)",
            "universal_codelength(unsigned int, unsigned int)"]
    missing = [s for s in want if s not in defined]
    assert not missing, missing
    hdr = open(os.path.join(ROOT, "include", "bsvd.h")).read()
    for name in ("learn_model_mdl_forward_selection", "learn_model_mdl_backward_selection",
                 "learn_model_mdl_full_search", "model_codelength"):
        assert re.search(r"\bidx_t\s+" + name + r"\s*\(", hdr), name
    assert re.search(r"extern\s+ml_algorithm_t\s+learn_model\s*,\s*learn_model_inner\s*;", hdr)
    assert re.search(r"void\s+learn_model_setup\s*\(int mi_algo, int cu_algo, int du_algo, int lm_algo, int lmi_algo\)", hdr)
    for t in ("mi", "cu", "du", "lm"):
        assert re.search(r"extern\s+const\s+char\s*\*\s*%s_algorithm_names\[\]\s*;" % t, hdr), t
    assert "both learn_model_traditional unless assigned" in hdr


def test_setup_refuses_what_this_build_lacks(tmp_path):
    """learn_model_setup on the host alone: the reference's range message, and the name of a missing piece"""
    src = tmp_path / "setup.cpp"
    src.write_text('#include <cstdlib>\n#include "bsvd.h"\nint main(int c, char** v) {\n'
                   "  learn_model_setup(std::atoi(v[1]), std::atoi(v[2]), std::atoi(v[3]), std::atoi(v[4]), "
                   "std::atoi(v[5]));\n  return learn_model == learn_model_mdl_full_search ? 0 : 3;\n}\n")
    exe = str(tmp_path / "setup")
    lib = os.path.join(PKG, "lib")
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src), "-L", lib,
                    "-lbicpp", "-lbic", "-Wl,-rpath," + lib], check=True)

    def run(*idx):
        return subprocess.run([exe] + [str(i) for i in idx], capture_output=True, text=True, timeout=60)

    r = run(3, 1, 3, 6, 2)
    assert r.returncode == 0 and r.stdout.splitlines() == [
        "Using Random centroids (in mod-2 algebra) initialization", "Using Basic coefficients update",
        "Using Proximus-like dictionary update (OMP)", "Using MDL/full search for outer learning loop.",
        "Using Role-switched learning 2: after convergence, the role of A and D are switched and traditional model "
        "is applied again for inner learning."]
    r = run(0, 0, 0, 0, 4)
    assert r.returncode != 0 and "Invalid inner model learning algorithm (0-3)" in r.stderr
    r = run(0, 0, 0, 7, 0)
    assert r.returncode != 0 and "Invalid model learning algorithm (0-6)" in r.stderr
    for idx, piece in (((4, 0, 0, 0, 0), "initialize_model_graph_grow"), ((0, 2, 0, 0, 0), "update_coefficients_fast"),
                       ((0, 0, 2, 0, 0), "update_dictionary_steepest_omp")):
        r = run(*idx)
        assert r.returncode != 0 and piece in r.stderr and "not part of this build" in r.stderr, idx
