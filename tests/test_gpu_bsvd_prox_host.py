"""include/bsvd.h's update_dictionary_proximus through the C++ bridge (libbicpp.so,
bic::Device::bsvd_update_dictionary_proximus): tests/cpp/bsvd_prox_api_check.cpp reads E, D and A as PBM files,
calls the function and writes them back, which must be what the restatement (tests/bsvd_prox_ref.py) gives."""
import os
import subprocess

import numpy as np
import pytest

import bsvd_ref as R
from conftest import PKG, ROOT
from pnm_io import read_pbm_bytes, write_pbm
from test_bsvd_prox_ref import case

pytestmark = pytest.mark.gpu

SRC = os.path.join(ROOT, "tests", "cpp", "bsvd_prox_api_check.cpp")
EXE = os.path.join(PKG, "build", "bsvd_prox_api_check")


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


@pytest.mark.parametrize("name", ["update_dictionary_proximus", "update_dictionary_proximus_omp"])
def test_update_dictionary_proximus(exe, tmp_path, name):
    n, m, p = 300, 64, 33
    c = case(n, m, p, 0.05)
    assert c["ch"] >= 1 and c["st"]["on"] >= 1 and c["st"]["off"] >= 1 and c["st"]["uncounted"] >= 1
    files = {}
    for key, M, cols in (("E", c["E0"], m), ("D", c["D0"], m), ("A", c["A0"], p)):
        W = R.pack(M)
        # (read_pbm_header's height pattern would swallow a first raster byte that is white space)
        assert int(W[0, 0] >> np.uint64(56)) not in (9, 10, 11, 12, 13, 32), key
        files[key] = write_pbm(str(tmp_path / f"{key}.pbm"), W, cols)
    outs = [str(tmp_path / f"out{key}.pbm") for key in "EDA"]
    args = (["omp"] if name.endswith("_omp") else []) + [files["E"], files["D"], files["A"]] + outs
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"changed={c['ch']}" in r.stdout, r.stdout
    for path, M, rows, cols in zip(outs, (c["E"], c["D"], c["A"]), (n, p, n), (m, m, p)):
        with open(path, "rb") as f:
            rr, cc, W = read_pbm_bytes(f.read())
        assert (rr, cc) == (rows, cols), path
        assert np.array_equal(W, R.pack(M)), path
