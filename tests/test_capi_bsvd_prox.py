"""bic_bsvd_update_dictionary_proximus / bic_bsvd_learn_du / bic_set_bsvd_rounds exist at every layer (CPU only:
nothing is computed): declared in include/bic.h with the documented argument counts, exported by libbic.so,
listed in pybic.EXPORTS, bound as Context methods, behind the C++ bridge and include/bsvd.h."""
import inspect
import os
import re
import subprocess

import pytest

import pybic
from conftest import PKG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NARGS = {"bic_bsvd_update_dictionary_proximus": 12, "bic_bsvd_learn_du": 15, "bic_set_bsvd_rounds": 2}


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


def test_rule_constants():
    src = _header()
    assert re.search(r"#define\s+BIC_BSVD_DU_STEEPEST\s+0\b", src) and re.search(r"#define\s+BIC_BSVD_DU_PROXIMUS\s+1\b", src)
    assert (pybic.BSVD_DU_STEEPEST, pybic.BSVD_DU_PROXIMUS) == (0, 1)


@pytest.mark.parametrize("name", sorted(NARGS))
def test_exported_and_listed(name):
    lib = pybic.load()
    assert name in pybic.EXPORTS
    f = getattr(lib, name)  # AttributeError if libbic.so does not export it
    assert len(f.argtypes) == NARGS[name]


@pytest.mark.parametrize("method", ["bsvd_update_dictionary_proximus", "set_bsvd_rounds", "bsvd_learn"])
def test_bound_as_context_method(method):
    assert callable(getattr(pybic.Context, method, None)), method


def test_learn_takes_the_rule():
    par = inspect.signature(pybic.Context.bsvd_learn).parameters
    assert "du" in par and par["du"].default == 0


def test_header_states_the_contracts():
    """the header says that the PROXIMUS call blocks and cannot be captured, that `changed` does not count an
    atom whose users alone changed, that `rounds` is a host pointer and that every budget gives the same result"""
    src = " ".join(re.sub(r"\n \* ?", "\n", _header()).split())  # comment text without its line starts
    i = src.index("bic_bsvd_update_dictionary_proximus = update_dictionary_proximus")
    own = src[i:src.index("int bic_bsvd_update_dictionary_proximus(")]
    assert "bic_bsvd_update_dictionary_proximus therefore blocks" in own and "cannot be stream-captured" in own
    assert "rounds (HOST pointer, nullable)" in own
    assert "is not counted" in own and "for j < m only" in own
    assert "every value gives the same result" in own
    assert "No workgroup ever waits for another" in own


def test_bridge_exports_the_reference_functions():
    """libbicpp.so defines the two functions include/bsvd.h adds and the Device methods behind them, next to the
    earlier bsvd_learn, whose symbol is unchanged"""
    lib = os.path.join(PKG, "lib", "libbicpp.so")
    if not os.path.exists(lib):
        subprocess.run(["make", "-C", PKG], check=True, stdout=subprocess.DEVNULL)
    syms = subprocess.run(["nm", "-DC", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    defined = {line.split(" ", 2)[2] for line in syms.splitlines() if line.count(" ") >= 2}
    want = ["update_dictionary_proximus(binary_matrix&, binary_matrix&, binary_matrix&)",
            "update_dictionary_proximus_omp(binary_matrix&, binary_matrix&, binary_matrix&)",
            "bic::Device::bsvd_update_dictionary_proximus(binary_matrix&, binary_matrix&, binary_matrix&, "
            "unsigned long*, unsigned long*)",
            "bic::Device::bsvd_learn(binary_matrix&, binary_matrix&, binary_matrix&, binary_matrix&, int, "
            "unsigned long, unsigned long*)",
            "bic::Device::bsvd_learn(binary_matrix&, binary_matrix&, binary_matrix&, binary_matrix&, unsigned long, "
            "unsigned long*)"]
    missing = [s for s in want if s not in defined]
    assert not missing, missing
    hdr = open(os.path.join(ROOT, "include", "bsvd.h")).read()
    for name in ("update_dictionary_proximus", "update_dictionary_proximus_omp"):
        assert re.search(r"\bidx_t\s+" + name + r"\s*\(", hdr), name
