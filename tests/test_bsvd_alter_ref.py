"""tests/bsvd_alter_ref.py, the yardstick of the GPU tests of the wide-row steps and the role-switching learners,
pinned (CPU only): a literal worked by hand per learner, each with the quirk the text of bsvd.cpp:1247-1434 has;
the column-locality of the steepest rule that the wide kernel is built on; and the conditions that keep the GPU
comparisons from being vacuous."""
import functools

import numpy as np
import pytest

import bsvd_alter_ref as L
import bsvd_prox_ref as P
import bsvd_ref as R
from test_bsvd_prox_ref import bits, col

SEED = 5
# (n, m, p) of tests/test_gpu_bsvd_wide.py: 66 ragged words; exactly 65 words, many atoms; two full 4,096-column
# chunks and a bit more; counts and distances past 2^15; and, added to the issue's list, more than 4,096 rows, so
# that an atom's users are listed in more than one batch
WIDE_SHAPES = [(70, 4200, 33), (130, 4160, 300), (257, 8256, 64), (40, 70000, 7)]
SMALL_SHAPES = [(70, 100, 7), (300, 64, 33)]
MANY_ROWS = (4200, 70, 3)
# (n, m, p) of tests/test_gpu_bsvd_alter.py: the transposed width just over 4,096, ragged and word-exact; both narrow
ALTER_WIDE = [(4200, 100, 7), (4100, 64, 33), (4160, 130, 40)]
ALTER_SHAPES = ALTER_WIDE + [(300, 64, 33)]


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def wide_case(n, m, p):
    """the planted starts and the restatements' results of the three steps; computed once, never modified:
    sparse coding from the plain start, the steepest rule on its output, PROXIMUS from the a_flips start"""
    X, D0, A0, E0 = R.planted(SEED, n, m, p)
    E1, A1, cst = E0.copy(), A0.copy(), {}
    coef = R.update_coefficients_argmin(E1, D0, A1, p, cst)
    E2, D2 = E1.copy(), D0.copy()
    D_before = D0.copy()
    dict_ = R.update_dictionary(E2, D2, A1, m, p)
    Xp, Dp0, Ap0, Ep0 = R.planted(SEED, n, m, p, a_flips=0.05)
    Ep, Dp, Ap, pst = Ep0.copy(), Dp0.copy(), Ap0.copy(), {}
    prox = P.update_dictionary_proximus(Ep, Dp, Ap, m, p, pst)
    frozen(D0, A0, E0, E1, A1, E2, D2, D_before, Dp0, Ap0, Ep0, Ep, Dp, Ap)
    return dict(D0=D0, A0=A0, E0=E0, E1=E1, A1=A1, coef=coef, cst=cst, E2=E2, D2=D2, dict=dict_,
                Dp0=Dp0, Ap0=Ap0, Ep0=Ep0, Ep=Ep, Dp=Dp, Ap=Ap, prox=prox, pst=pst)


def alter_start(n, m, p, lm):
    return R.planted(SEED, n, m, p, noise=0.1, flips=0.3, a_flips=0.05 if lm == 3 else 0.0)


@functools.lru_cache(maxsize=None)
def alter_case(lm, du, n, m, p, max_iter=0):
    X, D0, A0, _ = alter_start(n, m, p, lm)
    E, D, A, trace = np.zeros_like(X), D0.copy(), A0.copy(), []
    it = L.learn(lm, X, E, D, A, m, p, du, max_iter, trace)
    frozen(X, D0, A0, E, D, A)
    return dict(X=X, D0=D0, A0=A0, E=E, D=D, A=A, it=it, trace=tuple(trace))


def nonvacuous_wide():
    """what the issue measured on the four wide shapes, asserted before the GPU tests compare on them"""
    c = [wide_case(*s) for s in WIDE_SHAPES]
    assert [v["coef"] for v in c] == [46, 89, 169, 26]
    assert [v["dict"] for v in c] == [28, 93, 64, 7]
    assert [v["prox"][1] for v in c] == [91, 617, 191, 21]
    for s, v in zip(WIDE_SHAPES, c):
        assert v["coef"] >= 1 and v["cst"]["multi"] >= 1 and v["dict"] >= 1, s
        assert v["prox"][1] > s[2] and v["pst"]["on"] + v["pst"]["off"] >= 1, s
        both = s != (130, 4160, 300)
        assert (v["pst"]["on"] >= 1 and v["pst"]["off"] >= 1) == both, s
    v = c[1]["pst"]
    assert (v["on"], v["off"]) == (121, 0)
    v = wide_case(*MANY_ROWS)
    assert v["coef"] >= 1 and v["dict"] >= 1 and v["pst"]["on"] >= 1 and v["pst"]["off"] >= 1
    return c


def nonvacuous_alter():
    """alter1 on the wide shapes: the transposed sparse coding and the transposed dictionary step each moved
    something, the learners end in 2 to 11 passes, and (4200, 100, 7) with the steepest rule stops in a pass whose
    direct sparse coding still moved a row: the sum of a traditional loop would have gone on"""
    first = {0: [13, 24, 84], 1: [5, 9, 34]}
    for du in (0, 1):
        for s, want in zip(ALTER_WIDE, first[du]):
            c = alter_case(1, du, *s)
            tr = c["trace"]
            assert tr[2] == ("t", "c", want), (s, du)
            assert sum(x[2] for x in tr if x[:2] == ("t", "c")) >= 1 and sum(x[2] for x in tr if x[:2] == ("t", "u")) >= 1
            assert 2 <= c["it"] <= 11 and len(tr) == 4 * c["it"], (s, du)
    tr = alter_case(1, 0, 4200, 100, 7)["trace"]
    assert tr[-4][:2] == ("d", "c") and tr[-4][2] >= 1 and tr[-1] == ("t", "u", 0)


def test_wide_starts_are_not_vacuous():
    nonvacuous_wide()


def test_alter_starts_are_not_vacuous():
    nonvacuous_alter()
    for s in ALTER_SHAPES:  # every learner and rule runs its loop and ends; alter3 never codes
        for lm in (1, 2, 3):
            for du in (0, 1):
                c = alter_case(lm, du, *s)
                assert c["it"] >= 1 and np.array_equal(c["E"], R.residual(c["X"], c["D"], c["A"], s[2]))
                assert (lm == 3) == all(x[1] == "u" for x in c["trace"])


def test_transpose_crops_and_pads():
    B = bits(["1101", "0111"], 64)
    B[:, 40] = 1  # padding past c = 4
    t = L.T(B, 2, 4)
    assert t.shape == (4, 64) and np.array_equal(t, bits(["10", "11", "01", "11"]))
    assert np.array_equal(L.T(t, 4, 2), bits(["1101", "0111"]))
    assert L.T(np.ones((70, 128), np.uint8), 70, 65).shape == (65, 128)


LIT = dict(X=["0111", "0000", "0001"], D=["0101"], A=[0, 0, 1])


def run(lm, X, D, A, du=0, max_iter=0):
    X, D, A, tr = bits(X), bits(D), col(A), []
    E = np.zeros_like(X)
    it = L.learn(lm, X, E, D, A, 4, 1, du, max_iter, tr)
    return it, E, D, A, tr


def test_alter1_stops_on_the_transposed_dictionary_count_alone():
    """E = X ^ A D = 0111, 0000, 0100. Direct coding: row 0 (weight 3) is at distance 1 of 0101 and takes it
    (0010); rows 1 and 2 stay: 1 row. Direct dictionary: users 0 and 2, E ^ D = 0111, 0001, counts 0, 1, 1, 2 > 1
    give 0001; the users take delta 0100: E = 0110, 0000, 0000: 1 atom. Exchanged: Et = 000, 100, 100, 000, the
    atom At = 101, Dt = 0, 0, 0, 1. No row of Et gets lighter by 101: 0 rows. The atom's one user is row 3 = 000,
    E ^ D = 101 > 0 gives 101 again: 0 atoms, and :1297 keeps that 0 alone: one pass, although the direct steps moved."""
    it, E, D, A, tr = run(1, **LIT)
    assert it == 1 and tr == [("d", "c", 1), ("d", "u", 1), ("t", "c", 0), ("t", "u", 0)]
    assert np.array_equal(E, bits(["0110", "0000", "0000"])) and np.array_equal(D, bits(["0001"]))
    assert A[:, 0].tolist() == [1, 0, 1]


def test_alter2_skips_the_second_direct_loop_and_returns_the_last_transposed_count():
    """the same start: the direct loop runs twice (2, then 0), the transposed loop once (0); outer_changed is 2, so
    a second outer pass starts, whose direct loop is skipped (`changed` is still 0) and whose transposed loop runs
    once more; iter was reset to 0 before it: the return value is 1, not the 4 passes run."""
    it, E, D, A, tr = run(2, **LIT)
    assert it == 1 and [x[0] for x in tr] == list("ddddtttt") and [x[2] for x in tr] == [1, 1, 0, 0, 0, 0, 0, 0]
    assert np.array_equal(E, bits(["0110", "0000", "0000"])) and np.array_equal(D, bits(["0001"]))
    # the cap counts the passes over the whole call: 3 is reached in the first transposed loop
    it3, E3, D3, A3, tr3 = run(2, max_iter=3, **LIT)
    assert it3 == 1 and [x[0] for x in tr3] == list("ddddtt") and np.array_equal(E3, E)
    it1, _, _, _, tr1 = run(2, max_iter=1, **LIT)
    assert it1 == 1 and [x[0] for x in tr1] == list("dd")


def test_alter3_never_codes_and_only_the_direct_step_decides():
    """E = 1101, 0011, 0011. Exchanged first: Et = 100, 100, 011, 111, the atom At = 001, its users the rows 0 and 2
    of Et (D's bits); E ^ D = 101, 010, counts 1, 1, 1 > 1 fail: At = 000, 1 atom changed, the users take 001. Back:
    A = 0, E = X. The direct step finds no user: 0, and that alone ends the loop although the pass changed an atom."""
    it, E, D, A, tr = run(3, ["1101", "0011", "1001"], ["1010"], [0, 0, 1])
    assert it == 1 and tr == [("t", "u", 1), ("d", "u", 0)]
    assert not A.any() and np.array_equal(E, bits(["1101", "0011", "1001"])) and np.array_equal(D, bits(["1010"]))


def test_padding_comes_back_zero():
    n, m, p = 70, 100, 7
    rng = np.random.default_rng(9)
    X, D, A, _ = (a.copy() for a in alter_start(n, m, p, 1))
    X[:, m:] = rng.random(X[:, m:].shape) < 0.3
    D[:, m:] = rng.random(D[:, m:].shape) < 0.3
    A[:, p:] = rng.random(A[:, p:].shape) < 0.3
    E = np.zeros_like(X)
    assert L.learn_alter1(X, E, D, A, m, p) >= 1
    assert not E[:, m:].any() and not D[:, m:].any() and not A[:, p:].any()


@pytest.mark.parametrize("n,m,p", [(70, 4200, 33), (257, 8256, 64)])
def test_steepest_rule_is_local_to_its_columns(n, m, p):
    """the rule applied to the wide matrix equals the rule applied to each 4,096-column chunk on its own (E and D
    identical), and an atom changed iff it changed in some chunk: what lets a workgroup walk all the atoms by itself"""
    c = wide_case(n, m, p)
    E, D, A = c["E1"], c["D0"], c["A1"]
    changed_in = np.zeros(p, bool)
    for c0 in range(0, m, 4096):
        mc = min(4096, m - c0)
        wc = 64 * R.words(mc)
        Ec, Dc = E[:, c0:c0 + wc].copy(), D[:, c0:c0 + wc].copy()
        R.update_dictionary(Ec, Dc, A, mc, p)
        assert np.array_equal(Ec, c["E2"][:, c0:c0 + wc]) and np.array_equal(Dc, c["D2"][:, c0:c0 + wc])
        changed_in |= (Dc != D[:, c0:c0 + wc]).any(axis=1)
    assert np.array_equal(changed_in, (c["D2"] != D).any(axis=1)) and int(changed_in.sum()) == c["dict"]
