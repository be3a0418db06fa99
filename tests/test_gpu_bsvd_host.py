"""include/bsvd.h through the C++ bridge (libbicpp.so, bic::Device::bsvd_learn): tests/cpp/bsvd_api_check.cpp
reads X, D and A as PBM files, calls learn_model_traditional and writes E, D and A, which must be what the
restatement (tests/bsvd_ref.py) gives for the same planted data."""
import os
import subprocess

import numpy as np
import pytest

import bsvd_ref as R
from conftest import PKG, ROOT
from pnm_io import read_pbm_bytes, write_pbm

pytestmark = pytest.mark.gpu

SRC = os.path.join(ROOT, "tests", "cpp", "bsvd_api_check.cpp")
EXE = os.path.join(PKG, "build", "bsvd_api_check")


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


@pytest.mark.parametrize("seed,n,m,p", [(1, 257, 256, 64), (2, 300, 64, 33)])
def test_learn_model_traditional(exe, tmp_path, seed, n, m, p):
    X, D, A, E = R.planted(seed, n, m, p)
    files = {}
    for name, M, cols in (("X", X, m), ("D", D, m), ("A", A, p)):
        W = R.pack(M)
        # (read_pbm_header's height pattern would swallow a first raster byte that is white space)
        assert int(W[0, 0] >> np.uint64(56)) not in (9, 10, 11, 12, 13, 32), name
        files[name] = write_pbm(str(tmp_path / f"{name}.pbm"), W, cols)
    it = R.learn(X, E, D, A, m, p)
    assert it >= 2 and E.any()  # the loop did something and left something
    outs = [str(tmp_path / f"out{name}.pbm") for name in "EDA"]
    r = subprocess.run([exe, files["X"], files["D"], files["A"]] + outs, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"iters={it}" in r.stdout, r.stdout
    for path, M, rows, cols in zip(outs, (E, D, A), (n, p, n), (m, m, p)):
        with open(path, "rb") as f:
            rr, cc, W = read_pbm_bytes(f.read())
        assert (rr, cc) == (rows, cols), path
        assert np.array_equal(W, R.pack(M)), path
