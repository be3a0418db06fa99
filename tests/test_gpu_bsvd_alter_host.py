"""include/bsvd.h's role-switching learners, its update_dictionary global and its step functions on wide matrices
through the C++ bridge (libbicpp.so): tests/cpp/bsvd_alter_check.cpp reads its matrices as PBM files, calls the
function and writes E, D and A back, which must be what the restatements give (tests/bsvd_alter_ref.py and the
cases of tests/test_bsvd_alter_ref.py)."""
import os
import subprocess

import numpy as np
import pytest

import bsvd_alter_ref as L
import bsvd_ref as R
from conftest import PKG, ROOT
from pnm_io import read_pbm_bytes, write_pbm
from test_bsvd_alter_ref import SEED, alter_case, wide_case

pytestmark = pytest.mark.gpu

SRC = os.path.join(ROOT, "tests", "cpp", "bsvd_alter_check.cpp")
EXE = os.path.join(PKG, "build", "bsvd_alter_check")


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


def run(exe, tmp_path, mode, first, D, A, shape, want):
    """first, D, A in -> stdout; the three outputs must be `want` (E, D, A, unpacked)"""
    n, m, p = shape
    files = []
    for key, M, cols in (("F", first, m), ("D", D, m), ("A", A, p)):
        W = R.pack(M)
        # (read_pbm_header's height pattern would swallow a first raster byte that is white space)
        assert int(W[0, 0] >> np.uint64(56)) not in (9, 10, 11, 12, 13, 32), key
        files.append(write_pbm(str(tmp_path / f"{key}.pbm"), W, cols))
    outs = [str(tmp_path / f"out{key}.pbm") for key in "EDA"]
    r = subprocess.run([exe, mode] + files + outs, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for path, M, rows, cols in zip(outs, want, (n, p, n), (m, m, p)):
        with open(path, "rb") as f:
            rr, cc, W = read_pbm_bytes(f.read())
        assert (rr, cc) == (rows, cols), path
        assert np.array_equal(W, R.pack(M)), path
    return r.stdout


@pytest.mark.parametrize("lm", [1, 3])
def test_learners(exe, tmp_path, lm):
    shape = (4200, 100, 7)
    c = alter_case(lm, 0, *shape)
    out = run(exe, tmp_path, f"alter{lm}", c["X"], c["D0"], c["A0"], shape, (c["E"], c["D"], c["A"]))
    assert f"result={c['it']}\n" in out, out


def test_update_dictionary_switched_and_back(exe, tmp_path):
    """update_dictionary = update_dictionary_proximus_omp makes learn_model_alter3 run PROXIMUS; set back, a learner
    run afterwards is the steepest one again"""
    shape = (4200, 100, 7)
    c = alter_case(3, 1, *shape)
    assert not np.array_equal(c["E"], alter_case(3, 0, *shape)["E"])  # the rule matters
    # (alter3's start has a_flips, alter1's has not: the second run, from the same files, is restated here)
    X, D, A = c["X"].copy(), c["D0"].copy(), c["A0"].copy()
    after = L.learn_alter1(X, np.zeros_like(X), D, A, shape[1], shape[2])
    out = run(exe, tmp_path, "alter3_prox", c["X"], c["D0"], c["A0"], shape, (c["E"], c["D"], c["A"]))
    assert f"result={c['it']}\n" in out and f"after={after}\n" in out, out


def test_traditional_unchanged_with_the_default(exe, tmp_path):
    shape = (300, 64, 33)
    X, D0, A0, _ = R.planted(SEED, *shape)
    E, D, A = np.zeros_like(X), D0.copy(), A0.copy()
    it = R.learn(X, E, D, A, shape[1], shape[2])
    assert it >= 2
    out = run(exe, tmp_path, "traditional", X, D0, A0, shape, (E, D, A))
    assert f"result={it}\n" in out, out


def test_wide_steps(exe, tmp_path):
    """update_coefficients (the global: update_coefficients_omp), update_dictionary (the global: steepest) and
    update_dictionary_proximus on a matrix of 4,200 columns"""
    shape = (70, 4200, 33)
    c = wide_case(*shape)
    out = run(exe, tmp_path, "coef", c["E0"], c["D0"], c["A0"], shape, (c["E1"], c["D0"], c["A1"]))
    assert f"result={c['coef']}\n" in out, out
    out = run(exe, tmp_path, "steepest", c["E1"], c["D0"], c["A1"], shape, (c["E2"], c["D2"], c["A1"]))
    assert f"result={c['dict']}\n" in out, out
    out = run(exe, tmp_path, "proximus", c["Ep0"], c["Dp0"], c["Ap0"], shape, (c["Ep"], c["Dp"], c["Ap"]))
    assert f"result={c['prox'][0]}\n" in out, out
