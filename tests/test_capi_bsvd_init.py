"""The model initialisers exist at every layer (CPU only: nothing runs on a device): the six entries are declared
in include/bic.h with the documented argument counts, exported by libbic.so, listed in pybic.EXPORTS and bound;
the C++ bridge defines the include/bsvd.h functions and the Device method; tests/cpp/bsvd_init_api_check.cpp
compiles and links against them. The two host-only generator entries need no device: their refusals are checked
here, their values in tests/test_bsvd_init_ref.py."""
import ctypes
import os
import re
import subprocess

import pytest

import pybic
from conftest import PKG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NARGS = {"bic_bsvd_rng_seed": 2, "bic_bsvd_rng_uniform": 4, "bic_bsvd_init_neighbor": 11,
         "bic_bsvd_init_partition": 10, "bic_bsvd_init_centroids": 12, "bic_bsvd_initialize": 12}
HOST_ONLY = {"bic_bsvd_rng_seed", "bic_bsvd_rng_uniform"}


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
    assert (args[0] == "bic_ctx* ctx") == (name not in HOST_ONLY)


def test_rule_constants():
    src = _header()
    for k, name in enumerate(("NEIGHBOR", "PARTITION", "CENTROIDS", "CENTROIDS_XOR")):
        assert re.search(r"#define\s+BIC_BSVD_MI_%s\s+%d\b" % (name, k), src), name
        assert getattr(pybic, "BSVD_MI_" + name) == k


@pytest.mark.parametrize("name", sorted(NARGS))
def test_exported_and_listed(name):
    lib = pybic.load()
    assert name in pybic.EXPORTS
    f = getattr(lib, name)  # AttributeError if libbic.so does not export it
    assert len(f.argtypes) == NARGS[name]


@pytest.mark.parametrize("method", ["bsvd_init_neighbor", "bsvd_init_partition", "bsvd_init_centroids",
                                    "bsvd_initialize"])
def test_bound_as_context_method(method):
    assert callable(getattr(pybic.Context, method, None)), method


def test_generator_bound_as_functions():
    assert callable(pybic.bsvd_rng_seed) and callable(pybic.bsvd_rng_uniform)
    assert pybic.bsvd_rng_seed(34503498) == (34503498 << 16) | 0x330E


def test_generator_refusals():
    """the two host-only entries need no device: bound 0, a null state, a null out with values to write"""
    lib = pybic.load()
    st, out = ctypes.c_uint64(5), (ctypes.c_uint32 * 4)()
    assert lib.bic_bsvd_rng_seed(1, None) == pybic.BIC_EINVAL
    assert lib.bic_bsvd_rng_uniform(ctypes.byref(st), 0, 4, out) == pybic.BIC_EINVAL  # bound 0
    assert lib.bic_bsvd_rng_uniform(None, 7, 4, out) == pybic.BIC_EINVAL
    assert lib.bic_bsvd_rng_uniform(ctypes.byref(st), 7, 4, None) == pybic.BIC_EINVAL
    assert st.value == 5
    assert lib.bic_bsvd_rng_uniform(ctypes.byref(st), 7, 0, None) == pybic.BIC_OK and st.value == 5
    assert lib.bic_bsvd_rng_uniform(ctypes.byref(st), 1, 4, out) == pybic.BIC_OK and list(out) == [0] * 4


def test_header_states_the_contracts():
    """which kinds block, what an index out of range does, the padding convention, what is refused"""
    src = " ".join(re.sub(r"\n \* ?", "\n", _header()).split())  # comment text without its line starts
    own = src[src.index("---- model initialisers"):src.index("#define BIC_BSVD_MI_NEIGHBOR")]
    assert "NEIGHBOR and both CENTROIDS kinds block" in own and "PARTITION does not block" in own
    assert "cannot be stream-captured" in own and "no workgroup ever waits for another" in own
    assert "which is skipped, never dereferenced" in own and "An entry >= p is skipped" in own
    assert "E's padding bits are ignored" in own and "with zero padding bits" in own
    assert "n = 0 too" in own and "if no row is non-zero it returns BIC_EINVAL" in own
    assert "a rejected output is used up" in own
    assert "model initialisers are not part of this build" not in src


def _bridge():
    lib = os.path.join(PKG, "lib", "libbicpp.so")
    if not os.path.exists(lib):
        subprocess.run(["make", "-C", PKG], check=True, stdout=subprocess.DEVNULL)
    return lib


def test_bridge_exports_the_reference_functions():
    syms = subprocess.run(["nm", "-DC", "--defined-only", _bridge()], capture_output=True, text=True, check=True).stdout
    defined = {line.split(" ", 2)[2] for line in syms.splitlines() if line.count(" ") >= 2}
    sig = "(binary_matrix const&, binary_matrix&, binary_matrix&)"
    want = ["initialize_model_neighbor" + sig, "initialize_model_partition" + sig,
            "initialize_model_random_centroids" + sig, "initialize_model_random_centroids_xor" + sig,
            "initialize_model", "random_seed",
            "bic::Device::bsvd_initialize(int, binary_matrix const&, binary_matrix&, binary_matrix&, unsigned long*)"]
    missing = [s for s in want if s not in defined]
    assert not missing, missing
    hdr = open(os.path.join(ROOT, "include", "bsvd.h")).read()
    for name in want[:4]:
        assert re.search(r"\bvoid\s+" + name[:name.index("(")] + r"\s*\(", hdr), name
    assert re.search(r"extern\s+mi_algorithm_t\s+initialize_model\s*;", hdr)
    assert re.search(r"extern\s+long\s+random_seed\s*;", hdr) and "typedef void (*mi_algorithm_t)" in hdr
    assert "initialisers" in hdr and "The caller fills D and A" not in hdr


def test_api_check_compiles_and_links(tmp_path):
    """tests/cpp/bsvd_init_api_check.cpp takes the address of initialize_model and calls through it"""
    src = os.path.join(ROOT, "tests", "cpp", "bsvd_init_api_check.cpp")
    assert "&initialize_model" in open(src).read()
    exe = str(tmp_path / "bsvd_init_api_check")
    libdir = os.path.dirname(_bridge())
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", exe, src, "-L", libdir,
                    "-lbicpp", "-lbic", "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr  # (no device is touched without arguments)
