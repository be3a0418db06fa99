"""The wide-row steps on the device (bic_bsvd_wide.hip; include/bic.h bic_bsvd_update_coefficients_wide /
bic_bsvd_update_dictionary_wide) against the numpy restatements of bsvd.cpp:399-735 (tests/bsvd_ref.py,
tests/bsvd_prox_ref.py), whose stats on these starts tests/test_bsvd_alter_ref.py asserts. Bit-exact over every
word of E, D and A, with the changed counts and the rounds. The entries run the wide kernels whatever m, so the
shapes of a few words reach them too."""
import numpy as np
import pytest

import bsvd_prox_ref as P
import bsvd_ref as R
import pybic
from pybic import as_u64
from test_bsvd_alter_ref import MANY_ROWS, SEED, SMALL_SHAPES, WIDE_SHAPES, nonvacuous_wide, wide_case

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1)] + SMALL_SHAPES + WIDE_SHAPES + [MANY_ROWS]
STEEPEST, PROXIMUS = pybic.BSVD_DU_STEEPEST, pybic.BSVD_DU_PROXIMUS


def dev(ctx, B):
    return ctx.to_dev(R.pack(B))


def same(t, B):
    return np.array_equal(as_u64(t), R.pack(B))


def one_bit():
    """E = D = the one bit, A = 0: the row takes the atom (E = 0, A = 1); the steepest rule then votes the atom's one
    user, 0 ^ 1 = 1 > 0: unchanged; PROXIMUS from the start recruits the row in its first round and confirms"""
    B = np.zeros((1, 64), np.uint8)
    B[0, 0] = 1
    Z = np.zeros((1, 64), np.uint8)
    return dict(D0=B, A0=Z, E0=B, E1=Z, A1=B, coef=1, cst={"multi": 0}, E2=Z, D2=B, dict=0,
                Dp0=B, Ap0=Z, Ep0=B, Ep=Z, Dp=B, Ap=B, prox=(0, 2), pst={"on": 1, "off": 0})


def case(n, m, p):
    return one_bit() if (n, m, p) == (1, 1, 1) else wide_case(n, m, p)


@pytest.fixture(autouse=True)
def automatic_budget(ctx):
    nonvacuous_wide()
    ctx.set_bsvd_rounds(0)
    yield
    ctx.set_bsvd_rounds(0)


def test_one_bit_restated():
    c = one_bit()
    E, A = c["E0"].copy(), c["A0"].copy()
    assert R.update_coefficients(E, c["D0"], A, 1) == 1 and np.array_equal(E, c["E1"]) and np.array_equal(A, c["A1"])
    D = c["D0"].copy()
    assert R.update_dictionary(E, D, A, 1, 1) == 0 and np.array_equal(D, c["D2"])
    E, D, A = c["Ep0"].copy(), c["Dp0"].copy(), c["Ap0"].copy()
    assert P.update_dictionary_proximus(E, D, A, 1, 1) == c["prox"] and np.array_equal(A, c["Ap"]) and not E.any()


@pytest.mark.parametrize("n,m,p", SHAPES)
def test_sparse_coding_then_steepest(ctx, n, m, p):
    c = case(n, m, p)
    if n > 1:
        assert c["coef"] >= 1 and c["cst"]["multi"] >= 1 and c["dict"] >= 1
    E, D, A = dev(ctx, c["E0"]), dev(ctx, c["D0"]), dev(ctx, c["A0"])
    assert ctx.bsvd_update_coefficients_wide(E, m, D, A, p) == c["coef"]
    assert same(E, c["E1"]) and same(D, c["D0"]) and same(A, c["A1"])
    assert ctx.bsvd_update_dictionary_wide(E, m, D, A, p, du=STEEPEST) == c["dict"]
    assert same(E, c["E2"]) and same(D, c["D2"]) and same(A, c["A1"])


@pytest.mark.parametrize("n,m,p", SHAPES)
def test_proximus(ctx, n, m, p):
    c = case(n, m, p)
    if n > 1:
        assert c["prox"][0] >= 1 and c["prox"][1] > p and c["pst"]["on"] + c["pst"]["off"] >= 1
    E, D, A = dev(ctx, c["Ep0"]), dev(ctx, c["Dp0"]), dev(ctx, c["Ap0"])
    assert ctx.bsvd_update_dictionary_wide(E, m, D, A, p, du=PROXIMUS) == c["prox"]
    assert same(E, c["Ep"]) and same(D, c["Dp"]) and same(A, c["Ap"])


def test_widest_row(ctx):
    """m = 1,048,576, n = 2, p = 2: E_0 all ones, E_1 zero, D_0 zero, D_1 all ones but one bit. Row 0 is at distance
    2^20 of atom 0 and 1 of atom 1 (a key of more than 32 bits) and takes atom 1; row 1 takes nothing. Then the
    steepest rule: atom 1's one user has E ^ D = all ones, so the atom becomes all ones and E_0 zero."""
    m, hole = 1 << 20, 777_777
    E = np.zeros((2, m), np.uint8)
    E[0] = 1
    D = np.zeros((2, m), np.uint8)
    D[1] = 1
    D[1, hole] = 0
    A = np.zeros((2, 64), np.uint8)
    dE, dD, dA = dev(ctx, E), dev(ctx, D), dev(ctx, A)
    assert ctx.bsvd_update_coefficients_wide(dE, m, dD, dA, 2) == 1
    E[0] = 0
    E[0, hole] = 1
    A[0, 1] = 1
    assert same(dE, E) and same(dD, D) and same(dA, A)
    assert ctx.bsvd_update_dictionary_wide(dE, m, dD, dA, 2) == 1
    E[0, hole] = 0
    D[1, hole] = 1
    assert same(dE, E) and same(dD, D) and same(dA, A)


@pytest.mark.parametrize("n,m,p", SMALL_SHAPES + [(257, 256, 64), (2500, 130, 40)])
def test_narrow_entries_agree(ctx, n, m, p):
    """at m <= 4096 the wide entries give the narrow entries' outputs (which have their own tests)"""
    X, D0, A0, E0 = R.planted(SEED, n, m, p, a_flips=0.05)
    got = []
    for wide in (False, True):
        E, D, A = dev(ctx, E0), dev(ctx, D0), dev(ctx, A0)
        if wide:
            r = (ctx.bsvd_update_coefficients_wide(E, m, D, A, p), ctx.bsvd_update_dictionary_wide(E, m, D, A, p),
                 ctx.bsvd_update_dictionary_wide(E, m, D, A, p, du=PROXIMUS))
        else:
            r = (ctx.bsvd_update_coefficients(E, m, D, A, p), ctx.bsvd_update_dictionary(E, m, D, A, p),
                 ctx.bsvd_update_dictionary_proximus(E, m, D, A, p))
        got.append((r, as_u64(E).copy(), as_u64(D).copy(), as_u64(A).copy()))
    assert got[0][0] == got[1][0] and got[0][0][0] >= 1 and got[0][0][2][1] > p
    assert all(np.array_equal(a, b) for a, b in zip(got[0][1:], got[1][1:]))


@pytest.mark.parametrize("a_flips", [0.0, 0.05])
def test_padding_and_pitch(ctx, a_flips):
    """(130, 4200, 7) with dirty padding bits in E, D and A and pitched rows filled with random words: the padding
    bits of D and A and the words past every row's own come back unchanged; sparse coding then the steepest rule
    from the plain start, PROXIMUS from the start with flipped coefficients"""
    n, m, p = 130, 4200, 7
    rng = np.random.default_rng(9)
    X, D, A, _ = (a.copy() for a in R.planted(SEED, n, m, p, a_flips=a_flips))
    X[:, m:] = rng.random(X[:, m:].shape) < 0.3
    D[:, m:] = rng.random(D[:, m:].shape) < 0.3
    A[:, p:] = rng.random(A[:, p:].shape) < 0.3
    E = R.residual(X, D, A, p)
    assert E[:, m:].any() and D[:, m:].any() and A[:, p:].any()
    D0, A0 = D.copy(), A.copy()

    def pitched(B, extra):
        W = R.pack(B)
        tail = rng.integers(0, 1 << 63, (W.shape[0], extra), dtype=np.uint64)
        return ctx.to_dev(np.concatenate([W, tail], axis=1)), tail

    def check(t, B, tail):
        got = as_u64(t)
        w = got.shape[1] - tail.shape[1]
        return np.array_equal(got[:, :w], R.pack(B)) and np.array_equal(got[:, w:], tail)

    (dE, tE), (dD, tD), (dA, tA) = pitched(E, 3), pitched(D, 1), pitched(A, 2)
    if a_flips:
        st = {}
        res = P.update_dictionary_proximus(E, D, A, m, p, st)
        assert res[0] >= 1 and st["on"] + st["off"] >= 1
        assert ctx.bsvd_update_dictionary_wide(dE, m, dD, dA, p, du=PROXIMUS) == res
    else:
        c1 = R.update_coefficients_argmin(E, D, A, p)
        assert c1 >= 1
        assert ctx.bsvd_update_coefficients_wide(dE, m, dD, dA, p) == c1
        assert check(dE, E, tE) and check(dD, D, tD) and check(dA, A, tA)
        c2 = R.update_dictionary(E, D, A, m, p)
        assert c2 >= 1
        assert ctx.bsvd_update_dictionary_wide(dE, m, dD, dA, p) == c2
    assert check(dE, E, tE) and check(dD, D, tD) and check(dA, A, tA)
    assert np.array_equal(D[:, m:], D0[:, m:]) and np.array_equal(A[:, p:], A0[:, p:])


def test_round_budget(ctx):
    """budgets 1, 2 and automatic give the same PROXIMUS result; some atom needs more than two rounds, so 1 and 2
    both take an atom up again"""
    n, m, p = 257, 8256, 64
    c = wide_case(n, m, p)
    assert c["pst"]["max_rounds"] > 2
    for budget in (1, 2, 0):
        ctx.set_bsvd_rounds(budget)
        E, D, A = dev(ctx, c["Ep0"]), dev(ctx, c["Dp0"]), dev(ctx, c["Ap0"])
        assert ctx.bsvd_update_dictionary_wide(E, m, D, A, p, du=PROXIMUS) == c["prox"], budget
        assert same(E, c["Ep"]) and same(D, c["Dp"]) and same(A, c["Ap"]), budget


def test_arguments(ctx):
    lib, h, C = ctx.lib, ctx.h, pybic.C
    E, D, A = ctx.empty_i64(4, 2), ctx.empty_i64(7, 2), ctx.empty_i64(4, 1)
    big_a = ctx.empty_i64(4, 65)
    ch = ctx.empty_i64(1)
    p_ = lambda t: None if t is None else pybic._p(t)
    ctx._bind_stream()

    def calls(e, n, m, e_wpr, d, p, d_wpr, a, a_wpr):
        r = C.c_size_t(0)
        return (lib.bic_bsvd_update_coefficients_wide(h, p_(e), n, m, e_wpr, p_(d), p, d_wpr, p_(a), a_wpr, p_(ch)),
                lib.bic_bsvd_update_dictionary_wide(h, 0, p_(e), n, m, e_wpr, p_(d), p, d_wpr, p_(a), a_wpr, p_(ch), None),
                lib.bic_bsvd_update_dictionary_wide(h, 1, p_(e), n, m, e_wpr, p_(d), p, d_wpr, p_(a), a_wpr, p_(ch),
                                                    C.byref(r)))

    bad = (pybic.BIC_EINVAL,) * 3
    assert calls(E, 4, 0, 2, D, 7, 2, A, 1) == bad                    # m = 0
    assert calls(E, 4, 1048577, 16385, D, 7, 16385, A, 1) == bad      # m = 1,048,577 (refused before any access)
    assert calls(E, 4, 100, 2, D, 0, 2, A, 1) == bad                  # p = 0
    assert calls(E, 4, 100, 2, D, 4097, 2, big_a, 65) == bad          # p = 4097
    assert calls(E, 4, 100, 1, D, 7, 2, A, 1) == bad                  # short pitches
    assert calls(E, 4, 100, 2, D, 7, 1, A, 1) == bad
    assert calls(E, 4, 100, 2, D, 65, 2, A, 1) == bad
    assert calls(E, 1 << 31, 100, 2, D, 7, 2, A, 1) == bad            # n = 2^31
    assert calls(None, 4, 100, 2, D, 7, 2, A, 1) == bad               # null matrices with n > 0
    assert calls(E, 4, 100, 2, None, 7, 2, A, 1) == bad
    assert calls(E, 4, 100, 2, D, 7, 2, None, 1) == bad
    for du in (2, -1):
        assert lib.bic_bsvd_update_dictionary_wide(h, du, p_(E), 4, 100, 2, p_(D), 7, 2, p_(A), 1, p_(ch),
                                                   None) == pybic.BIC_EINVAL
    # n = 0: nothing to do, changed = 0 and rounds = 0
    for du in (0, 1):
        ch.fill_(-1)
        rounds = C.c_size_t(7)
        assert lib.bic_bsvd_update_dictionary_wide(h, du, None, 0, 100, 2, p_(D), 7, 2, None, 1, p_(ch),
                                                   C.byref(rounds)) == pybic.BIC_OK
        assert int(as_u64(ch)[0]) == 0 and rounds.value == 0
    ch.fill_(-1)
    assert lib.bic_bsvd_update_coefficients_wide(h, None, 0, 100, 2, p_(D), 7, 2, None, 1, p_(ch)) == pybic.BIC_OK
    assert int(as_u64(ch)[0]) == 0
    ctx.sync()
