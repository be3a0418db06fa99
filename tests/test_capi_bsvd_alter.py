"""bic_bsvd_update_coefficients_wide / bic_bsvd_update_dictionary_wide / bic_bsvd_learn_lm exist at every layer (CPU
only: nothing is computed): declared in include/bic.h with the documented argument counts, exported by libbic.so,
listed in pybic.EXPORTS, bound as Context methods, behind the C++ bridge and include/bsvd.h."""
import inspect
import os
import re
import subprocess

import pytest

import pybic
from conftest import PKG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NARGS = {"bic_bsvd_update_coefficients_wide": 11, "bic_bsvd_update_dictionary_wide": 13, "bic_bsvd_learn_lm": 16}


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
    assert decl["bic_bsvd_update_dictionary_wide"].split(",")[1].strip() == "int du"
    assert decl["bic_bsvd_update_dictionary_wide"].split(",")[-1].strip() == "size_t* rounds"
    lm = [a.strip() for a in decl["bic_bsvd_learn_lm"].split(",")]
    assert lm[1:4] == ["int lm", "int du", "const uint64_t* X"] and lm[-2:] == ["size_t max_iter", "size_t* iters"]
    # the narrow entries are declared as before
    assert len(decl["bic_bsvd_update_coefficients"].split(",")) == 11 and len(decl["bic_bsvd_learn_du"].split(",")) == 15


def test_learner_constants():
    src = _header()
    for i, name in enumerate(("TRADITIONAL", "ALTER1", "ALTER2", "ALTER3")):
        assert re.search(r"#define\s+BIC_BSVD_LM_%s\s+%d\b" % (name, i), src), name
    assert (pybic.BSVD_LM_TRADITIONAL, pybic.BSVD_LM_ALTER1, pybic.BSVD_LM_ALTER2, pybic.BSVD_LM_ALTER3) == (0, 1, 2, 3)


@pytest.mark.parametrize("name", sorted(NARGS))
def test_exported_and_listed(name):
    lib = pybic.load()
    assert name in pybic.EXPORTS
    f = getattr(lib, name)  # AttributeError if libbic.so does not export it
    assert len(f.argtypes) == NARGS[name]


@pytest.mark.parametrize("method", ["bsvd_update_coefficients_wide", "bsvd_update_dictionary_wide", "bsvd_learn"])
def test_bound_as_context_method(method):
    assert callable(getattr(pybic.Context, method, None)), method


def test_python_signatures():
    par = inspect.signature(pybic.Context.bsvd_learn).parameters
    assert par["du"].default == 0 and par["lm"].default == 0
    par = inspect.signature(pybic.Context.bsvd_update_dictionary_wide).parameters
    assert list(par)[1:7] == ["E", "m", "D", "A", "p", "du"] and par["du"].default == 0


def test_header_states_the_domain_and_the_quirks():
    src = " ".join(re.sub(r"\n \* ?", "\n", _header()).split())  # comment text without its line starts
    i = src.index("wide rows and the role-switching learners")
    own = src[i:src.index("int bic_bsvd_learn_lm(")]
    assert "1 <= m <= 1048576, 1 <= p <= 4096, n < 2^31" in own
    assert "1 <= m <= 1048576, 1 <= n <= 1048576, 1 <= p <= 4096" in own
    assert "always run the wide kernels, whatever m" in own
    assert "No workgroup ever waits for another" in own
    assert "D_k's last word masked" in own and "padding bits of D and A never changed" in own
    assert "goes on only on the transposed dictionary step's count" in own
    assert "that loop is skipped" in own and "last transposed loop's count" in own
    assert "no sparse coding at all" in own and "only the direct one's count decides" in own
    assert "padding bits inside the words of E, D and A are zero" in own
    assert "max_iter (0 = none) caps the loop passes" in own and "The call blocks" in own
    # the narrow entries keep their domain
    assert "Domain: 1 <= m <= 4096, 1 <= p <= 4096, n < 2^31" in src


def test_bridge_exports_the_reference_functions():
    lib = os.path.join(PKG, "lib", "libbicpp.so")
    if not os.path.exists(lib):
        subprocess.run(["make", "-C", PKG], check=True, stdout=subprocess.DEVNULL)
    syms = subprocess.run(["nm", "-DC", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    defined = {line.split(" ", 2)[2] for line in syms.splitlines() if line.count(" ") >= 2}
    four = "(binary_matrix&, binary_matrix&, binary_matrix&, binary_matrix&)"
    want = ["learn_model_alter1" + four, "learn_model_alter2" + four, "learn_model_alter3" + four,
            "learn_model_traditional" + four, "update_coefficients", "update_dictionary",
            "bic::Device::bsvd_learn(int, int, binary_matrix&, binary_matrix&, binary_matrix&, binary_matrix&, "
            "unsigned long, unsigned long*)",
            # the earlier overloads keep their symbols
            "bic::Device::bsvd_learn(binary_matrix&, binary_matrix&, binary_matrix&, binary_matrix&, int, "
            "unsigned long, unsigned long*)",
            "bic::Device::bsvd_learn(binary_matrix&, binary_matrix&, binary_matrix&, binary_matrix&, unsigned long, "
            "unsigned long*)"]
    missing = [s for s in want if s not in defined]
    assert not missing, missing
    hdr = open(os.path.join(ROOT, "include", "bsvd.h")).read()
    for name in ("learn_model_alter1", "learn_model_alter2", "learn_model_alter3"):
        assert re.search(r"\bidx_t\s+" + name + r"\s*\(", hdr), name
    for t in ("cu_algorithm_t", "du_algorithm_t", "ml_algorithm_t"):
        assert re.search(r"typedef\s+idx_t\s*\(\*" + t + r"\)", hdr), t
    assert re.search(r"extern\s+cu_algorithm_t\s+update_coefficients\s*;", hdr)
    assert re.search(r"extern\s+du_algorithm_t\s+update_dictionary\s*;", hdr)
    assert "update_dictionary_steepest unless assigned" in hdr
