"""include/bsvd.h's model initialisers through the C++ bridge (libbicpp.so, bic::Device::bsvd_initialize):
tests/cpp/bsvd_init_api_check.cpp reads E as a PBM file, calls the functions named, all in one process, and writes
every D and A, which must be what the restatement (tests/bsvd_init_ref.py) gives from one generator seeded with
random_seed: consecutive calls share the process generator, and the partition rule leaves it alone."""
import os
import subprocess

import numpy as np
import pytest

import bsvd_init_ref as I
import bsvd_ref as R
from conftest import PKG, ROOT
from pnm_io import read_pbm_bytes, write_pbm
from test_bsvd_init_ref import case

pytestmark = pytest.mark.gpu

SRC = os.path.join(ROOT, "tests", "cpp", "bsvd_init_api_check.cpp")
EXE = os.path.join(PKG, "build", "bsvd_init_api_check")
RULE = {"neighbor": I.NEIGHBOR, "default": I.NEIGHBOR, "partition": I.PARTITION, "centroids": I.CENTROIDS,
        "xor": I.CENTROIDS_XOR}


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


@pytest.mark.parametrize("rules", [["neighbor", "centroids", "partition", "xor", "default"], ["xor", "neighbor"]])
def test_consecutive_calls_share_the_generator(exe, tmp_path, rules):
    n, m, p = 130, 320, 100
    c = case(n, m, p)
    W = R.pack(c["E"])
    # (read_pbm_header's height pattern would swallow a first raster byte that is white space)
    assert int(W[0, 0] >> np.uint64(56)) not in (9, 10, 11, 12, 13, 32)
    src = write_pbm(str(tmp_path / "E.pbm"), W, m)
    r, want, redraws = I.Rand48(), [], 0
    for name in rules:
        st = {}
        want.append(I.initialize(RULE[name], c["E"], m, p, r, st))
        redraws += st.get("redraws", 0)
    assert redraws >= 1 and r.outputs > n + p
    assert not np.array_equal(want[-1][0], c[RULE[rules[-1]]]["D"])  # a fresh generator would give other atoms
    run = subprocess.run([exe, src, str(p), str(tmp_path)] + rules, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert f"calls={len(rules)}" in run.stdout
    for t, (D, A) in enumerate(want):
        for key, M, rows, cols in (("D", D, p, m), ("A", A, n, p)):
            with open(str(tmp_path / f"{key}{t}.pbm"), "rb") as f:
                rr, cc, got = read_pbm_bytes(f.read())
            assert (rr, cc) == (rows, cols), (key, t)
            assert np.array_equal(got, R.pack(M)), (key, t)
