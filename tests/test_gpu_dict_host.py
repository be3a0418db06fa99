"""bic::Device::dict_encode through the C++ bridge (libbicpp.so): tests/cpp/dict_api_check.cpp runs the loop with
two fresh GolombCoders and requires them to end as host GolombCoders fed the same samples do; the bitcount,
samples and k it prints must be those of the oracle's coding of the restatement's samples (tests/dict_ref.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

import dict_cases
import dict_ref
import dropin_expect
from conftest import PKG, ROOT
from pnm_io import write_pbm

pytestmark = pytest.mark.gpu

SRC = os.path.join(ROOT, "tests", "cpp", "dict_api_check.cpp")
EXE = os.path.join(PKG, "build", "dict_api_check")


@pytest.fixture(scope="module")
def exe():
    lib = os.path.join(PKG, "lib", "libbicpp.so")
    if not os.path.exists(lib):
        subprocess.run(["make", "-C", PKG], check=True, stdout=subprocess.DEVNULL)
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(SRC), os.path.getmtime(lib)):
        os.makedirs(os.path.dirname(EXE), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", EXE, SRC,
                        "-L", os.path.join(PKG, "lib"), "-lbicpp", "-lbic",
                        "-Wl,-rpath," + os.path.join(PKG, "lib")], check=True)
    return EXE


def final_k(samples):
    """Golomb.h: after n samples with sum A, k = min{k >= 0 : n << k >= A}; a coder never used keeps k = 1"""
    n, a, k = len(samples), int(np.sum(samples, dtype=np.uint64)), 0
    if n == 0:
        return 1
    while (n << k) < a:
        k += 1
    return k


@pytest.mark.parametrize("name,variant,step", [("glyph", 3, 1), ("glyph", 3, 16), ("camera", 3, 1), ("glyph", 2, 16)])
def test_device_dict_encode(exe, oracle, tmp_path, name, variant, step):
    case = next(c for c in dict_cases.CASES if c["name"] == name)
    plane, rows, cols = dict_cases.make_input(case)
    W, T = case["W"], case["T"]
    step = W if step != 1 else 1
    # this build's enumL (bic_enum_codelength, what Device::dict_encode uses without a table)
    import pybic
    e = pybic.enum_table(W)
    exp = dict_ref.dict_encode(plane, cols, variant, W, T, step, e)
    # (read_pbm_header's height pattern would swallow a first raster byte that is white space)
    assert int(plane[0, 0] >> np.uint64(56)) not in (9, 10, 11, 12, 13, 32)
    path = write_pbm(str(tmp_path / "I.pbm"), plane, cols)
    r = subprocess.run([exe, path, str(variant), str(W), str(T), str(step)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {m.group(1): [int(x) for x in m.groups()[1:]] for m in
           re.finditer(r"^(match|nomatch) bitcount=(\d+) samples=(\d+) accumulated=(\d+) k=(\d+)$", r.stdout, re.M)}
    for key, s in (("match", exp["samples_match"]), ("nomatch", exp["samples_nomatch"])):
        bits = oracle.golomb_samples(s, False)[0]
        assert got[key] == [bits, len(s), int(s.sum()), final_k(s)], key
    m = re.search(r"tiles=(\d+) matches=(\d+) L=(\d+) D=(\d+) stream_bits=(\d+),(\d+)", r.stdout)
    assert [int(x) for x in m.groups()[:4]] == [len(exp["bestk"]), exp["matches"], exp["L"], exp["nD"]]
    assert [int(x) for x in m.groups()[4:]] == [got["match"][0], got["nomatch"][0]]
