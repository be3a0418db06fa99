"""tests/bsvd_ref.py, the restatement the GPU dictionary-learning tests compare against, pinned two ways
(CPU only): hand-worked cases as literals, and on planted data the identity E == X ^ A D after every
step, computed with the oracle's mul() (tests/oracle_lib.py gf2_mul, itself pinned to the reference's
objects), with the weight of E never rising and a second sparse-coding pass reporting 0."""
import numpy as np
import pytest

import bsvd_ref as R
from pybic import GF2_AB

SHAPES = [(130, 100, 7), (257, 256, 64), (300, 64, 33), (130, 320, 300)]


def bits(*rows):
    """'11110000' strings -> 0/1 rows padded with zeros to a whole word"""
    out = np.zeros((len(rows), 64), np.uint8)
    for i, r in enumerate(rows):
        out[i, :len(r)] = [int(c) for c in r]
    return out


def test_coefficients_by_hand():
    """3 rows x 8 bits, 2 atoms. Row 0: both atoms at distance 4 = the weight: no step. Row 1: both at
    distance 4 < 6, the tie goes to k = 0, then k = 1 at distance 2 < 4: two steps. Row 2 starts with atom
    0 on and takes it again (distance 1 < 5): switched off."""
    D = bits("11110000", "00001111")
    E = bits("11000011", "11101110", "11110001")
    A = bits("00", "00", "10")
    st = {}
    assert R.update_coefficients(E, D, A, 2, st) == 2
    assert np.array_equal(E, bits("11000011", "00010001", "00000001"))
    assert np.array_equal(A, bits("00", "11", "00"))
    assert st == {"multi": 1, "ties": 1, "off": 1, "steps": 3}
    assert np.array_equal(D, bits("11110000", "00001111"))
    assert R.update_coefficients(E, D, A, 2) == 0  # a fixed point


def test_dictionary_by_hand():
    """3 rows x 8 bits, 3 atoms; atom 1 unused; row 1 uses atoms 0 and 2. Atom 0, U = 2: the counts of
    E ^ D_0 are 1 2 2 2 0 0 0 2, so bit 0 (1 > 1 is false) clears and bit 7 sets; row 1 carries that change
    (E_1 = 10000000) into atom 2's counts 2 0 0 0 2 2 2 2, which set bit 0 -- without the carry they would be
    1 0 0 0 2 2 2 1 and clear bit 7 instead."""
    D = bits("11110000", "10101010", "00001111")
    A = bits("100", "101", "001")
    E = bits("10000001", "00000001", "10000000")
    X = R.residual(E, D, A, 3)
    assert R.update_dictionary(E, D, A, 8, 3) == 2
    assert np.array_equal(D, bits("01110001", "10101010", "10001111"))
    assert not E.any()
    assert np.array_equal(A, bits("100", "101", "001"))
    assert np.array_equal(R.residual(X, D, A, 3), E)


def test_dictionary_keeps_padding_bits():
    """the vote runs over j < m; the atom's bits past m come from D_k (newDk starts as its copy)"""
    D = bits("1111000011")  # m = 8: two padding bits set
    A = bits("1", "1", "1")
    E = bits("1000000100", "1000000100", "0000000011")
    assert R.update_dictionary(E, D, A, 8, 1) == 1
    assert np.array_equal(D, bits("0111000111"))
    assert np.array_equal(E, bits("0000000000", "0000000000", "1000000111"))


def test_pack_round_trip():
    rng = np.random.default_rng(1)
    W = rng.integers(0, 1 << 63, (5, 3), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    assert np.array_equal(R.pack(R.unpack(W)), W)
    assert R.unpack(np.array([[1 << 63]], np.uint64))[0, 0] == 1  # MSB = column 0


def identity_holds(oracle, X, E, D, A, n, m, p):
    """E == X ^ A D with the product from the oracle's mul_AB (whole words of D)"""
    AD = oracle.gf2_mul(GF2_AB, R.pack(A), n, p, R.pack(D), p, m, np.zeros((n, R.words(m)), np.uint64), n, m)
    return np.array_equal(R.pack(E), R.pack(X) ^ AD)


@pytest.mark.parametrize("n,m,p", SHAPES)
def test_planted_model(oracle, n, m, p):
    """what the GPU tests rely on: the planted data moves (at least half the rows change, some in two
    steps, ties at the minimum in the first three shapes, atoms change), the identity holds after every
    step, the weight never rises, the loop over k and the one-reduction form agree, learning ends."""
    X, D, A, E = R.planted(1, n, m, p)
    assert identity_holds(oracle, X, E, D, A, n, m, p)
    E2, A2, st, st2 = E.copy(), A.copy(), {}, {}
    w0 = int(E.sum())
    c1 = R.update_coefficients(E, D, A, p, st)
    assert R.update_coefficients_argmin(E2, D, A2, p, st2) == c1 and st == st2
    assert np.array_equal(E, E2) and np.array_equal(A, A2)
    assert c1 >= n // 2 and st["multi"] >= 1
    if (n, m, p) != SHAPES[3]:
        assert st["ties"] >= 1
    w1 = int(E.sum())
    assert w1 < w0 and identity_holds(oracle, X, E, D, A, n, m, p)
    assert R.update_coefficients(E.copy(), D, A.copy(), p) == 0  # a second pass right after reports 0
    Dpad, Apad = D[:, m:].copy(), A[:, p:].copy()
    c2 = R.update_dictionary(E, D, A, m, p)
    assert c2 >= 1
    w2 = int(E.sum())
    assert w2 <= w1 and identity_holds(oracle, X, E, D, A, n, m, p)
    assert np.array_equal(D[:, m:], Dpad) and np.array_equal(A[:, p:], Apad)
    # the whole loop from the start, both forms of the sparse-coding step
    runs = []
    for coef in (R.update_coefficients, R.update_coefficients_argmin):
        Xl, Dl, Al, El = R.planted(1, n, m, p)
        it = R.learn(Xl, El, Dl, Al, m, p, coef=coef)
        assert 2 <= it <= 6 and identity_holds(oracle, Xl, El, Dl, Al, n, m, p)
        assert int(El.sum()) <= w2
        runs.append((it, El, Dl, Al))
    assert runs[0][0] == runs[1][0] and all(np.array_equal(a, b) for a, b in zip(runs[0][1:], runs[1][1:]))


@pytest.mark.parametrize("n,m,p,rows", [(64, 4096, 65, 64), (130, 320, 4096, 24)])
def test_argmin_form_on_the_tiled_shapes(n, m, p, rows):
    """the one-reduction form the GPU tests use against the loop over k, on the two shapes the planted test
    leaves out (the n = 70000 case runs no sparse-coding restatement): rows of 64 words, and 4096 atoms (its
    first `rows` rows: rows are independent)"""
    X, D, A, E = R.planted(1, n, m, p)
    E, A = E[:rows].copy(), A[:rows].copy()
    E2, A2, st, st2 = E.copy(), A.copy(), {}, {}
    c = R.update_coefficients(E, D, A, p, st)
    assert c >= rows // 2
    assert R.update_coefficients_argmin(E2, D, A2, p, st2) == c and st == st2
    assert np.array_equal(E, E2) and np.array_equal(A, A2)


def test_planted_start_with_coefficients(oracle):
    """the start from a non-zero A switches coefficients off again"""
    n, m, p = 257, 256, 64
    X, D, A, E = R.planted(77, n, m, p, a_flips=0.05)
    assert A.any() and identity_holds(oracle, X, E, D, A, n, m, p)
    st = {}
    assert R.update_coefficients(E, D, A, p, st) >= n // 2 and st["off"] >= 1
    assert identity_holds(oracle, X, E, D, A, n, m, p)


def test_learn_cap():
    X, D, A, E = R.planted(5, 130, 100, 7)
    X2, D2, A2, E2 = R.planted(5, 130, 100, 7)
    assert R.learn(X, E, D, A, 100, 7, max_iter=1) == 1
    R.update_coefficients(E2, D2, A2, 7)
    R.update_dictionary(E2, D2, A2, 100, 7)
    assert np.array_equal(E, E2) and np.array_equal(D, D2) and np.array_equal(A, A2)
