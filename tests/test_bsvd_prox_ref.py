"""tests/bsvd_prox_ref.py, the yardstick of the GPU PROXIMUS tests, pinned (CPU only): literals worked by hand
from bsvd.cpp:530-735, the invariants of the rule on planted data, and the conditions that keep the GPU
comparisons from being vacuous."""
import functools

import numpy as np
import pytest

import bsvd_prox_ref as P
import bsvd_ref as R

# the planted starts the GPU tests compare on (seed 5, taken WITHOUT a sparse-coding step first: after one the
# planted model gives exactly 2 rounds per atom and almost no coefficient moves)
SEED = 5
SHAPES = [(257, 256, 64), (300, 64, 33), (2500, 130, 40)]
STARTS = [0.05, 0.0]


def bits(rows, width=64):
    """'1100' strings, bits left to right -> unpacked whole-word rows"""
    B = np.zeros((len(rows), width), np.uint8)
    for i, s in enumerate(rows):
        B[i, :len(s)] = [int(c) for c in s]
    return B


def col(a):
    A = np.zeros((len(a), 64), np.uint8)
    A[:, 0] = a
    return A


def run(E, D, A, m=4, p=1):
    E, D, A, st = bits(E), bits(D), col(A), {}
    res = P.update_dictionary_proximus(E, D, A, m, p, st)
    return res, E, D, A, st


def test_l1_tie_switches_a_user_off():
    """round 1: U = 3, counts of E ^ D = 3, 2, 0, 0 > 1 give 1100 again; |S| = 2, the users' Aw = 2, 2, 1 and
    1 > 1 fails: row 2 leaves and takes 1100 back (E = 1000). round 2 confirms. The atom's bits never changed:
    not counted."""
    (ch, rounds), E, D, A, st = run(["0000", "0000", "0100"], ["1100"], [1, 1, 1])
    assert (ch, rounds) == (0, 2)
    assert A[:, 0].tolist() == [1, 1, 0]
    assert np.array_equal(E, bits(["0000", "0000", "1000"])) and np.array_equal(D, bits(["1100"]))
    assert st["ties"] >= 1 and st["off"] == 1 and st["on"] == 0 and st["uncounted"] == 1


def test_l2_recruits_then_follows_its_users():
    """round 1: no users, no vote; |S| = 3, Aw = 3, 2, 0 > 1: rows 0 and 1 join (E = 0000, 0010, 0001).
    round 2: U = 2, counts of E ^ D = 2, 2, 1, 0 > 1 give 1100; E = 0010, 0000, 0001; |S| = 2, the users'
    Aw = 2, 2, the other row's 0: nobody moves, but the atom did. round 3 confirms."""
    (ch, rounds), E, D, A, st = run(["1110", "1100", "0001"], ["1110"], [0, 0, 0])
    assert (ch, rounds) == (1, 3)
    assert np.array_equal(D, bits(["1100"])) and A[:, 0].tolist() == [1, 1, 0]
    assert np.array_equal(E, bits(["0010", "0000", "0001"]))
    assert st["recruited"] == 1 and st["on"] == 2 and st["uncounted"] == 0


def test_l3_zero_atom_formed_from_its_users():
    """round 1: U = 2, counts 2, 0, 2, 0 > 1 give 1010 and E = 0; the coefficient half then has |S| = 2,
    users' Aw = 2 - 0 = 2 > 1 stay, row 2's Aw = 0 stays out. round 2 confirms."""
    (ch, rounds), E, D, A, _ = run(["1010", "1010", "0000"], ["0000"], [1, 1, 0])
    assert (ch, rounds) == (1, 2)
    assert np.array_equal(D, bits(["1010"])) and not E.any() and A[:, 0].tolist() == [1, 1, 0]


def test_l5_even_tie_clears_the_atom_and_keeps_its_users():
    """U = 2, counts of E ^ D = 1, 0, 0, 0; 1 > 1 fails: D = 0000, E = 1000, 0000. |S| = 0 skips the
    coefficient half, so both rows stay users of a zero atom."""
    (ch, rounds), E, D, A, _ = run(["0000", "1000"], ["1000"], [1, 1])
    assert ch == 1 and rounds == 2
    assert not D.any() and np.array_equal(E, bits(["1000", "0000"])) and A[:, 0].tolist() == [1, 1]


@functools.lru_cache(maxsize=None)
def case(n, m, p, a_flips):
    """the planted start and the restatement's result with its stats; computed once, never modified"""
    X, D0, A0, E0 = R.planted(SEED, n, m, p, a_flips=a_flips)
    E, D, A, st = E0.copy(), D0.copy(), A0.copy(), {}
    ch, rounds = P.update_dictionary_proximus(E, D, A, m, p, st)
    for a in (X, D0, A0, E0, E, D, A):
        a.setflags(write=False)
    return dict(X=X, D0=D0, A0=A0, E0=E0, E=E, D=D, A=A, ch=ch, rounds=rounds, st=st)


def nonvacuous():
    """the conditions under which a comparison on these starts exercises the rule (asserted here and again
    by the GPU tests before they compare)"""
    c = {(s, f): case(*s, f) for s in SHAPES for f in STARTS}
    assert max(v["st"]["max_rounds"] for v in c.values()) >= 4
    assert sum(v["st"]["on"] for v in c.values()) > 0 and sum(v["st"]["off"] for v in c.values()) > 0
    for s in SHAPES:
        assert c[(s, 0.0)]["st"]["recruited"] >= (s[2] + 1) // 2, s
    assert c[((300, 64, 33), 0.05)]["st"]["uncounted"] >= 1
    for v in c.values():
        assert v["ch"] >= 1 and v["rounds"] > len(v["st"]["rounds_per_atom"])
    return c


def test_planted_starts_are_not_vacuous():
    c = nonvacuous()
    assert sum(v["st"]["on"] + v["st"]["off"] for k, v in c.items() if k[0][0] == 2500) >= 1000


@pytest.mark.parametrize("n,m,p,a_flips", [(300, 64, 33, 0.05), (300, 64, 33, 0.0), (130, 100, 7, 0.05)])
def test_invariants(n, m, p, a_flips):
    """E == X ^ A D after every half, |E| never rises, and a second call on the converged model runs one round
    per atom and changes nothing"""
    X, D, A, E = R.planted(SEED, n, m, p, a_flips=a_flips)
    weights = [int(E.sum())]

    def after_half(k, rk, half):
        assert np.array_equal(E, R.residual(X, D, A, p)), (k, rk, half)
        weights.append(int(E.sum()))

    ch, rounds = P.update_dictionary_proximus(E, D, A, m, p, after_half=after_half)
    assert ch >= 1 and all(b <= a for a, b in zip(weights, weights[1:])) and weights[-1] < weights[0]
    # (a later atom's moves may unsettle an earlier one: further calls go on until every atom takes one round)
    for _ in range(50):
        ch2, rounds2 = P.update_dictionary_proximus(E, D, A, m, p)
        if rounds2 == p:
            break
    assert (ch2, rounds2) == (0, p)
    assert np.array_equal(E, R.residual(X, D, A, p))


def test_second_call_on_a_converged_atom_runs_one_round():
    n, m, p = 200, 64, 1
    X, D, A, E = R.planted(SEED, n, m, p, a_flips=0.05)
    ch, rounds = P.update_dictionary_proximus(E, D, A, m, p)
    assert ch == 1 and rounds >= 2
    E1, D1, A1 = E.copy(), D.copy(), A.copy()
    assert P.update_dictionary_proximus(E, D, A, m, p) == (0, 1)
    assert np.array_equal(E, E1) and np.array_equal(D, D1) and np.array_equal(A, A1)


def test_dirty_padding_is_kept():
    """m = 100, p = 7 with dirty padding bits in E, D and A: the padding of all three comes back unchanged
    (the atom half's delta is 0 past m, the coefficient half runs over j < m only), and E stays X ^ A D there"""
    n, m, p = 130, 100, 7
    rng = np.random.default_rng(9)
    X, D, A, _ = (a.copy() for a in R.planted(SEED, n, m, p, a_flips=0.05))
    X[:, m:] = rng.random(X[:, m:].shape) < 0.3
    D[:, m:] = rng.random(D[:, m:].shape) < 0.3
    A[:, p:] = rng.random(A[:, p:].shape) < 0.3
    E = R.residual(X, D, A, p)
    E0, D0, A0 = E.copy(), D.copy(), A.copy()
    assert E[:, m:].any() and D[:, m:].any() and A[:, p:].any()
    st = {}
    ch, rounds = P.update_dictionary_proximus(E, D, A, m, p, st)
    assert ch >= 1 and st["on"] + st["off"] >= 1
    assert np.array_equal(E[:, m:], E0[:, m:]) and np.array_equal(D[:, m:], D0[:, m:])
    assert np.array_equal(A[:, p:], A0[:, p:])
    # (a coefficient that flips does not carry D_k's padding into E, so the identity holds for j < m only)
    assert np.array_equal(E[:, :m], R.residual(X, D, A, p)[:, :m])


def test_learn_swaps_the_dictionary_step_only():
    n, m, p = 300, 64, 33
    X, D, A, E = R.planted(SEED, n, m, p)
    it = P.learn(X, E, D, A, m, p)
    assert it >= 2 and np.array_equal(E, R.residual(X, D, A, p))
    assert R.update_dictionary.__name__ == "update_dictionary"  # the yardstick module is left as it was
    X1, D1, A1, E1 = R.planted(SEED, n, m, p)
    assert P.learn(X1, E1, D1, A1, m, p, max_iter=1) == 1
