"""The image mode through the C++ bridge (libbicpp.so): tests/cpp/patch_api_check.cpp reads a PBM, calls
bic::Device::patches, unpatch, mosaic and bsvd_learn_image, runs the driver's loops over the host binary_matrix (and the
separate bridge calls) beside them, and writes both; the results must be equal, and equal to tests/patch_ref.py."""
import os
import subprocess

import numpy as np
import pytest

import patch_ref as P
from conftest import PKG, ROOT
from pnm_io import read_pbm_bytes
from test_patch_ref import pbm_file, random_plane, valid

pytestmark = pytest.mark.gpu

SRC = os.path.join(ROOT, "tests", "cpp", "patch_api_check.cpp")
HDR = os.path.join(ROOT, "tests", "cpp", "patch_host_loops.h")
EXE = os.path.join(PKG, "build", "patch_api_check")


@pytest.fixture(scope="module")
def exe():
    lib = os.path.join(PKG, "lib", "libbicpp.so")
    if not os.path.exists(lib):
        subprocess.run(["make", "-C", PKG], check=True, stdout=subprocess.DEVNULL)
    newest = max(os.path.getmtime(SRC), os.path.getmtime(HDR), os.path.getmtime(lib))
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < newest:
        os.makedirs(os.path.dirname(EXE), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", EXE, SRC,
                        "-L", os.path.join(PKG, "lib"), "-lbicpp", "-lbic",
                        "-Wl,-rpath," + os.path.join(PKG, "lib")], check=True)
    return EXE


def words_of(path, rows, cols):
    return np.fromfile(path, np.uint64).reshape(rows, P.words(cols))


def pbm_of(path):
    with open(path, "rb") as f:
        return read_pbm_bytes(f.read())


@pytest.mark.parametrize("rows,cols,W,p", [(37, 126, 5, 8), (64, 128, 16, 8)])
def test_bridge_equals_the_host_loops(exe, tmp_path, rows, cols, W, p):
    I = random_plane(rows + cols + W, rows, cols, dirty=False)
    src = pbm_file(tmp_path / "I.pbm", I, cols)
    if cols % 64:  # (the program sets every pad bit after reading the file)
        I[:, -1] |= np.uint64((1 << (64 - cols % 64)) - 1)
    run = subprocess.run([exe, src, str(W), str(p), "1", str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    ny, nx = P.tiles(rows, cols, W)
    n, m = ny * nx, W * W
    t = lambda name: str(tmp_path / name)
    # patches: the bridge, the host loop and the restatement agree over every own word
    X = words_of(t("X_dev.bin"), n, m)
    assert np.array_equal(X, words_of(t("X_host.bin"), n, m))
    assert np.array_equal(X, P.gather(I, cols, W))
    # unpatch: the valid pixels agree (set_submatrix leaves edge bits in the pad columns; PBM files hold none)
    rr, cc, R = pbm_of(t("R_dev.pbm"))
    assert (rr, cc) == (rows, cols)
    assert np.array_equal(valid(R, cols), valid(pbm_of(t("R_host.pbm"))[2], cols))
    assert np.array_equal(R, P.scatter(X, W, rows, cols))
    # mosaic: the same file
    with open(t("M_dev.pbm"), "rb") as a, open(t("M_host.pbm"), "rb") as b:
        assert a.read() == b.read()
    # the one call and its parts
    it1, it2 = run.stdout.split("iters=")[1].split()[0].split(",")
    s1, s2 = run.stdout.split("states=")[1].split()[0].split(",")
    assert it1 == it2 and int(it1) >= 1 and s1 == s2
    assert f"n={n} m={m}" in run.stdout
    for key, r_, c_ in (("X", n, m), ("E", n, m), ("D", p, m), ("A", n, p)):
        one = words_of(t(f"one_{key}.bin"), r_, c_)
        assert np.array_equal(one, words_of(t(f"sep_{key}.bin"), r_, c_)), key
    assert np.array_equal(words_of(t("one_X.bin"), n, m), X)
    E = words_of(t("one_E.bin"), n, m)
    assert P.unpack(E, P.words(m))[:, :m].sum() < P.unpack(X, P.words(m))[:, :m].sum()  # something was learned
    with open(t("one_R.pbm"), "rb") as a, open(t("sep_R.pbm"), "rb") as b:
        one_r = a.read()
        assert one_r == b.read()
    assert np.array_equal(read_pbm_bytes(one_r)[2], P.scatter(E, W, rows, cols))
