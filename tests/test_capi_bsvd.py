"""bic_bsvd_update_coefficients / bic_bsvd_update_dictionary / bic_bsvd_learn exist at every layer (CPU only:
nothing is computed): declared in include/bic.h with the documented argument counts, exported by libbic.so,
listed in pybic.EXPORTS, bound as Context methods, behind the C++ bridge and include/bsvd.h."""
import os
import re
import subprocess

import pytest

import pybic
from conftest import PKG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NARGS = {"bic_bsvd_update_coefficients": 11, "bic_bsvd_update_dictionary": 11, "bic_bsvd_learn": 14}


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


@pytest.mark.parametrize("method", ["bsvd_update_coefficients", "bsvd_update_dictionary", "bsvd_learn"])
def test_bound_as_context_method(method):
    assert callable(getattr(pybic.Context, method, None)), method


def test_header_states_the_contracts():
    """the header says that bic_bsvd_learn blocks and cannot be captured, that the atoms are updated in order,
    that `changed` is written and `iters` is a host pointer"""
    src = open(os.path.join(ROOT, "include", "bic.h")).read()
    src = " ".join(re.sub(r"\n \* ?", "\n", src).split())  # comment text without its line starts
    assert "This call blocks" in src and "cannot be stream-captured" in src
    assert "The atoms are updated in order" in src
    assert "is written, not accumulated" in src
    assert "iters (HOST pointer, nullable)" in src
    assert "the smallest k that attains the minimum" in src


def test_bridge_exports_the_reference_functions():
    """libbicpp.so defines the four functions include/bsvd.h declares and the Device methods behind them"""
    lib = os.path.join(PKG, "lib", "libbicpp.so")
    if not os.path.exists(lib):
        subprocess.run(["make", "-C", PKG], check=True, stdout=subprocess.DEVNULL)
    syms = subprocess.run(["nm", "-DC", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    defined = {line.split(" ", 2)[2] for line in syms.splitlines() if line.count(" ") >= 2}
    want = ["update_coefficients_basic(binary_matrix&, binary_matrix const&, binary_matrix&)",
            "update_coefficients_omp(binary_matrix&, binary_matrix const&, binary_matrix&)",
            "update_dictionary_steepest(binary_matrix&, binary_matrix&, binary_matrix&)",
            "learn_model_traditional(binary_matrix&, binary_matrix&, binary_matrix&, binary_matrix&)",
            "bic::Device::bsvd_update_coefficients(binary_matrix&, binary_matrix const&, binary_matrix&, unsigned long*)",
            "bic::Device::bsvd_update_dictionary(binary_matrix&, binary_matrix&, binary_matrix const&, unsigned long*)",
            "bic::Device::bsvd_learn(binary_matrix&, binary_matrix&, binary_matrix&, binary_matrix&, unsigned long, "
            "unsigned long*)"]
    missing = [s for s in want if s not in defined]
    assert not missing, missing
    hdr = open(os.path.join(ROOT, "include", "bsvd.h")).read()
    for name in ("update_coefficients_basic", "update_coefficients_omp", "update_dictionary_steepest",
                 "learn_model_traditional"):
        assert re.search(r"\bidx_t\s+" + name + r"\s*\(", hdr), name
