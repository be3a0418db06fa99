"""include/bsvd.h's model_codelength, learn_model_mdl_* searches, learn_model / learn_model_inner globals and
learn_model_setup through the C++ bridge (libbicpp.so): tests/cpp/bsvd_mdl_check.cpp reads its matrices as PBM files,
calls the function and writes E, D and A back at their new sizes, which, with the lines it prints, must be what the
restatement gives (tests/bsvd_mdl_ref.py and the cases of tests/test_bsvd_mdl_ref.py)."""
import os
import subprocess

import numpy as np
import pytest

import bsvd_mdl_ref as M
import bsvd_ref as R
from bsvd_ref import words
from conftest import PKG, ROOT
from pnm_io import read_pbm_bytes, write_pbm
from test_bsvd_mdl_ref import nonvacuous, prim_case

pytestmark = pytest.mark.gpu

SRC = os.path.join(ROOT, "tests", "cpp", "bsvd_mdl_check.cpp")
EXE = os.path.join(PKG, "build", "bsvd_mdl_check")


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


def run(exe, tmp_path, mode, first, D, A, shape, want=None):
    """first, D, A in -> stdout; with `want` = (E, D, A, atoms), the outputs must be those"""
    n, m, p = shape
    files = []
    for key, B, cols in (("F", first, m), ("D", D, m), ("A", A, p)):
        W = R.pack(B)
        # (read_pbm_header's height pattern would swallow a first raster byte that is white space)
        assert int(W[0, 0] >> np.uint64(56)) not in (9, 10, 11, 12, 13, 32), key
        files.append(write_pbm(str(tmp_path / f"{key}.pbm"), W, cols))
    outs = [str(tmp_path / f"out{key}.pbm") for key in "EDA"]
    r = subprocess.run([exe, mode] + files + outs, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    if want is not None:
        atoms = want[3]
        assert f"atoms={atoms}\n" in r.stdout, r.stdout
        for path, B, rows, cols in list(zip(outs, want, (n, atoms, n), (m, m, atoms)))[:3 if atoms else 1]:
            with open(path, "rb") as f:
                rr, cc, W = read_pbm_bytes(f.read())
            assert (rr, cc) == (rows, cols), path
            assert np.array_equal(W, R.pack(B)[:rows, :words(cols)]), path
    return r.stdout


def start(c):
    p0 = c["p0"]
    return c["X"], c["D0"][:p0], c["A0"][:, :64 * words(p0)], (c["X"].shape[0], c["m"], p0)


def result(c):
    K = c["p"]
    return c["E"], c["D"][:K], c["A"][:, :64 * words(max(K, 1))], K


def printed(c):
    return "".join(line + "\n" for line in c["lines"])


@pytest.mark.parametrize("mode,name", [("backward", "backward"), ("forward", "forward_neighbor"),
                                       ("full_centroids", "full"), ("backward", "tiny")])
def test_searches(exe, tmp_path, mode, name):
    """E, D and A at their new sizes, the return value and the reference's lines; "tiny" ends in the empty model"""
    c = nonvacuous(name)
    X, D, A, shape = start(c)
    out = run(exe, tmp_path, mode, X, D, A, shape, result(c))
    assert out.startswith(printed(c)) and f"result={c['len']}\n" in out, out


def test_inner_learner_switched_and_back(exe, tmp_path):
    """learn_model_inner = learn_model_alter1 for one search; set back, the next search is the traditional one again"""
    c = nonvacuous("backward_alter1")
    X, D0, A0, shape = start(c)
    E, D, A = np.zeros_like(X), D0.copy(), A0.copy()
    r = M.backward(X, E, D, A, shape[1], shape[2], lmi=0)  # the second run, from the same files
    assert tuple(r["trace"]) != c["trace"]  # the inner learner matters
    out = run(exe, tmp_path, "backward_alter1", X, D0, A0, shape, result(c))
    lines = "".join(line + "\n" for line in r["lines"])
    assert out.startswith(printed(c) + lines + f"after={r['len']}\n") and f"result={c['len']}\n" in out, out


def test_setup_then_learn_model(exe, tmp_path):
    c = nonvacuous("backward")
    X, D, A, shape = start(c)
    out = run(exe, tmp_path, "setup_backward", X, D, A, shape, result(c))
    using = ("Using Neighbor initialization\nUsing OpenMP basic coefficients update\n"
             "Using Steepest descent (a la MOD)  dictionary update\n"
             "Using MDO/backward selection for outer learning loop.\n"
             "Using Model learning by traditional alternate descent for inner learning.\n")
    assert out.startswith(using + printed(c)) and f"result={c['len']}\n" in out, out


def test_model_codelength(exe, tmp_path):
    n, m, p = 300, 100, 7
    c = prim_case(n, m, p)
    out = run(exe, tmp_path, "codelength", c["E"], c["D"], c["A"], (n, m, p))
    assert f"result={M.codelength_from_weights(n, m, *c['weights'])}\n" in out, out
    assert f"empty={M.length_e(n, m, c['weights'][0])}\n" in out, out
