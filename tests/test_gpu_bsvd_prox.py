"""The PROXIMUS dictionary update on the device (bic_bsvd.hip k_bsvd_dict<true> / k_bsvd_prox_coef, include/bic.h
bic_bsvd_update_dictionary_proximus / bic_bsvd_learn_du / bic_set_bsvd_rounds) against the numpy restatement of
bsvd.cpp:530-735 (tests/bsvd_prox_ref.py, pinned by tests/test_bsvd_prox_ref.py). Bit-exact over every word of
E, D and A, with the changed count and the number of rounds, on planted starts taken without a sparse-coding
step first, whose restatement stats are asserted before they are used."""
import functools

import numpy as np
import pytest

import bsvd_prox_ref as P
import bsvd_ref as R
import pybic
from pybic import as_u64
from test_bsvd_prox_ref import SEED, bits, case, col, nonvacuous

pytestmark = pytest.mark.gpu

# (n, m, p): one bit; one workgroup, m no multiple of 64; whole words, p on a word boundary; one word, ragged
# p; three workgroups in the atom half, three words per row with the last masked
SHAPES = [(1, 1, 1), (70, 100, 7), (257, 256, 64), (300, 64, 33), (2500, 130, 40)]


def dev(ctx, B):
    return ctx.to_dev(R.pack(B))


def same(t, B):
    return np.array_equal(as_u64(t), R.pack(B))


@functools.lru_cache(maxsize=None)
def small(n, m, p, a_flips):
    if (n, m, p) == (1, 1, 1):  # the one bit set, the one atom equal to it: a_flips > 0 starts as its user
        X = np.zeros((1, 64), np.uint8)
        X[0, 0] = 1
        A0 = np.zeros((1, 64), np.uint8)
        A0[0, 0] = a_flips > 0
        D0, E0 = X.copy(), R.residual(X, X, A0, 1)
        E, D, A, st = E0.copy(), D0.copy(), A0.copy(), {}
        ch, rounds = P.update_dictionary_proximus(E, D, A, m, p, st)
        return dict(X=X, D0=D0, A0=A0, E0=E0, E=E, D=D, A=A, ch=ch, rounds=rounds, st=st)
    return case(n, m, p, a_flips)


@pytest.fixture(autouse=True)
def automatic_budget(ctx):
    """every test: the planted starts exercise the rule (cached after the first), the budget is the automatic one"""
    nonvacuous()
    ctx.set_bsvd_rounds(0)
    yield
    ctx.set_bsvd_rounds(0)


@pytest.mark.parametrize("a_flips", [0.05, 0.0])
@pytest.mark.parametrize("n,m,p", SHAPES)
def test_proximus(ctx, n, m, p, a_flips):
    c = small(n, m, p, a_flips)
    if n == 1:  # a non-user whose one bit the atom explains joins (2 rounds); a user stays (1 round)
        assert (c["ch"], c["rounds"], int(c["A"][0, 0])) == ((0, 2, 1) if a_flips == 0 else (0, 1, 1))
    else:
        assert c["ch"] >= 1 and c["rounds"] > p and c["st"]["on"] + c["st"]["off"] >= 1
    E, D, A = dev(ctx, c["E0"]), dev(ctx, c["D0"]), dev(ctx, c["A0"])
    assert ctx.bsvd_update_dictionary_proximus(E, m, D, A, p) == (c["ch"], c["rounds"])
    assert same(E, c["E"]) and same(D, c["D"]) and same(A, c["A"])


@pytest.mark.parametrize("E,D,A,want", [
    (["0000", "0000", "0100"], ["1100"], [1, 1, 1], (0, 2)),  # L1: a tie switches a user off, the atom uncounted
    (["1110", "1100", "0001"], ["1110"], [0, 0, 0], (1, 3)),  # L2: recruits, then the atom follows its users
    (["1010", "1010", "0000"], ["0000"], [1, 1, 0], (1, 2)),  # L3: a zero atom formed from its users
    (["0000", "1000"], ["1000"], [1, 1], (1, 2)),             # L5: the atom cleared with its change still pending
])
def test_hand_worked_cases(ctx, E, D, A, want):
    """the literals of tests/test_bsvd_prox_ref.py on the device (m = 4, p = 1): among them the coefficient
    launch that only delivers the atom half's change because the atom has become zero"""
    E, D, A = bits(E), bits(D), col(A)
    dE, dD, dA = dev(ctx, E), dev(ctx, D), dev(ctx, A)
    assert P.update_dictionary_proximus(E, D, A, 4, 1) == want
    assert ctx.bsvd_update_dictionary_proximus(dE, 4, dD, dA, 1) == want
    assert same(dE, E) and same(dD, D) and same(dA, A)


def test_padding_and_pitch(ctx):
    """m = 100, p = 7 with dirty padding bits in E, D and A and pitched rows filled with random words: the
    padding bits of all three and the words past each row's own come back unchanged"""
    n, m, p = 130, 100, 7
    rng = np.random.default_rng(9)
    X, D, A, _ = (a.copy() for a in R.planted(SEED, n, m, p, a_flips=0.05))
    X[:, m:] = rng.random(X[:, m:].shape) < 0.3
    D[:, m:] = rng.random(D[:, m:].shape) < 0.3
    A[:, p:] = rng.random(A[:, p:].shape) < 0.3
    E = R.residual(X, D, A, p)
    assert E[:, m:].any() and D[:, m:].any() and A[:, p:].any()

    def pitched(B, extra):
        W = R.pack(B)
        tail = rng.integers(0, 1 << 63, (W.shape[0], extra), dtype=np.uint64)
        return ctx.to_dev(np.concatenate([W, tail], axis=1)), tail

    def check(t, B, tail):
        got = as_u64(t)
        w = got.shape[1] - tail.shape[1]
        return np.array_equal(got[:, :w], R.pack(B)) and np.array_equal(got[:, w:], tail)

    (dE, tE), (dD, tD), (dA, tA) = pitched(E, 3), pitched(D, 1), pitched(A, 2)
    E1, D1, A1, st = E.copy(), D.copy(), A.copy(), {}
    res = P.update_dictionary_proximus(E1, D1, A1, m, p, st)
    assert res[0] >= 1 and st["on"] + st["off"] >= 1
    assert np.array_equal(E1[:, m:], E[:, m:]) and np.array_equal(D1[:, m:], D[:, m:])
    assert np.array_equal(A1[:, p:], A[:, p:])
    assert ctx.bsvd_update_dictionary_proximus(dE, m, dD, dA, p) == res
    assert check(dE, E1, tE) and check(dD, D1, tD) and check(dA, A1, tA)


def test_counts_across_workgroups(ctx):
    """n = 70000, m = 64, p = 5 with atom 0 used by every row (the columns of test_gpu_bsvd's large case):
    usage and column counts pass 16 bits and are summed over many workgroups, the coefficient kernel covers
    rows past one workgroup's share, and the last word of A's transpose holds 48 rows"""
    n, m, p = 70000, 64, 5
    X, D, A, _ = R.planted(3, n, m, p, a_flips=0.05)
    A[:, 0] = 1
    X[:, 0], X[:, 1], D[:, 0], D[:, 1], D[0, 1] = 1, 0, 0, 0, 1
    E = R.residual(X, D, A, p)
    dE, dD, dA = dev(ctx, E), dev(ctx, D), dev(ctx, A)
    st = {}
    res = P.update_dictionary_proximus(E, D, A, m, p, st)
    assert n % 64 and res[0] >= 1 and st["on"] >= 1 and st["off"] >= 1 and st["max_rounds"] >= 2
    assert ctx.bsvd_update_dictionary_proximus(dE, m, dD, dA, p) == res
    assert same(dE, E) and same(dD, D) and same(dA, A)


def test_round_budget(ctx):
    """every budget gives the same bits: with 1 the host takes every changing atom up again, and some atom
    needs more than 5 rounds, so 1, 2 and 5 all stall at least once"""
    n, m, p = 2500, 130, 40
    c = case(n, m, p, 0.0)
    assert c["st"]["max_rounds"] > 5 and sum(r > 1 for r in c["st"]["rounds_per_atom"]) >= p // 2
    for budget in (1, 2, 5, 0):
        ctx.set_bsvd_rounds(budget)
        E, D, A = dev(ctx, c["E0"]), dev(ctx, c["D0"]), dev(ctx, c["A0"])
        assert ctx.bsvd_update_dictionary_proximus(E, m, D, A, p) == (c["ch"], c["rounds"]), budget
        assert same(E, c["E"]) and same(D, c["D"]) and same(A, c["A"]), budget


@pytest.mark.parametrize("n,m,p", [(300, 64, 33), (2500, 130, 40)])
def test_transpose_stays_consistent(ctx, n, m, p):
    """the coefficient kernel rewrites the transposed A the atom half reads; a steepest step right after reads
    A itself: both must see the same users. Also a second PROXIMUS call from the first one's output."""
    c = case(n, m, p, 0.05)
    E, D, A = dev(ctx, c["E0"]), dev(ctx, c["D0"]), dev(ctx, c["A0"])
    assert ctx.bsvd_update_dictionary_proximus(E, m, D, A, p) == (c["ch"], c["rounds"])
    E2, D2, A2 = c["E"].copy(), c["D"].copy(), c["A"].copy()
    c2 = R.update_dictionary(E2, D2, A2, m, p)
    assert ctx.bsvd_update_dictionary(E, m, D, A, p) == c2
    assert same(E, E2) and same(D, D2) and same(A, A2)
    res = P.update_dictionary_proximus(E2, D2, A2, m, p)
    assert ctx.bsvd_update_dictionary_proximus(E, m, D, A, p) == res
    assert same(E, E2) and same(D, D2) and same(A, A2)


@pytest.mark.parametrize("n,m,p", [(257, 256, 64), (2500, 130, 40)])
def test_learn_du(ctx, n, m, p):
    c = case(n, m, p, 0.0)
    X, D, A, E = (c[k].copy() for k in ("X", "D0", "A0", "E0"))
    it = P.learn(X, E, D, A, m, p)
    assert it >= 2
    dX, dD, dA = dev(ctx, c["X"]), dev(ctx, c["D0"]), dev(ctx, c["A0"])
    dE = ctx.to_dev(np.full((n, R.words(m)), 0x5555555555555555, np.uint64))  # E is formed by the call
    assert ctx.bsvd_learn(dX, dE, m, dD, dA, p, du=pybic.BSVD_DU_PROXIMUS) == it
    assert same(dE, E) and same(dD, D) and same(dA, A) and same(dX, c["X"])


def test_learn_du_steepest_is_bsvd_learn(ctx):
    n, m, p = 257, 256, 64
    c = case(n, m, p, 0.0)
    out = []
    for entry in ("bic_bsvd_learn", "bic_bsvd_learn_du"):
        dX, dD, dA, dE = dev(ctx, c["X"]), dev(ctx, c["D0"]), dev(ctx, c["A0"]), ctx.empty_i64(n, R.words(m))
        it = pybic.C.c_size_t(0)
        args = (pybic._p(dX), dX.shape[1], pybic._p(dE), n, m, dE.shape[1], pybic._p(dD), p, dD.shape[1],
                pybic._p(dA), dA.shape[1], 0, pybic.C.byref(it))
        ctx._bind_stream()
        if entry == "bic_bsvd_learn":
            assert ctx.lib.bic_bsvd_learn(ctx.h, *args) == pybic.BIC_OK
        else:
            assert ctx.lib.bic_bsvd_learn_du(ctx.h, pybic.BSVD_DU_STEEPEST, *args) == pybic.BIC_OK
        out.append((it.value, as_u64(dE).copy(), as_u64(dD).copy(), as_u64(dA).copy()))
    assert out[0][0] == out[1][0] >= 2
    assert all(np.array_equal(a, b) for a, b in zip(out[0][1:], out[1][1:]))


def test_learn_du_max_iter(ctx):
    """max_iter = 1 stops after one sparse-coding step and one PROXIMUS step"""
    n, m, p = 257, 256, 64
    c = case(n, m, p, 0.0)
    E, D, A = c["E0"].copy(), c["D0"].copy(), c["A0"].copy()
    c1 = R.update_coefficients_argmin(E, D, A, p)
    ch, _ = P.update_dictionary_proximus(E, D, A, m, p)
    assert c1 + ch > 0  # the uncapped loop would go on
    dX, dD, dA, dE = dev(ctx, c["X"]), dev(ctx, c["D0"]), dev(ctx, c["A0"]), ctx.empty_i64(n, R.words(m))
    assert ctx.bsvd_learn(dX, dE, m, dD, dA, p, max_iter=1, du=pybic.BSVD_DU_PROXIMUS) == 1
    assert same(dE, E) and same(dD, D) and same(dA, A)


def test_arguments(ctx):
    lib, h = ctx.lib, ctx.h
    E, D, A = ctx.empty_i64(4, 2), ctx.empty_i64(7, 2), ctx.empty_i64(4, 1)
    big_e, big_d, big_a = ctx.empty_i64(4, 65), ctx.empty_i64(7, 65), ctx.empty_i64(4, 65)
    ch = ctx.empty_i64(1)
    p_ = lambda t: None if t is None else pybic._p(t)
    ctx._bind_stream()

    def calls(e, n, m, e_wpr, d, p, d_wpr, a, a_wpr):
        it, rounds = pybic.C.c_size_t(0), pybic.C.c_size_t(0)
        return (lib.bic_bsvd_update_dictionary_proximus(h, p_(e), n, m, e_wpr, p_(d), p, d_wpr, p_(a), a_wpr, p_(ch),
                                                        pybic.C.byref(rounds)),
                lib.bic_bsvd_learn_du(h, 1, p_(e), e_wpr, p_(e), n, m, e_wpr, p_(d), p, d_wpr, p_(a), a_wpr, 1,
                                      pybic.C.byref(it)))

    bad = (pybic.BIC_EINVAL,) * 2
    assert calls(E, 4, 0, 2, D, 7, 2, A, 1) == bad            # m = 0
    assert calls(big_e, 4, 4097, 65, big_d, 7, 65, A, 1) == bad  # m = 4097
    assert calls(E, 4, 100, 2, D, 0, 2, A, 1) == bad          # p = 0
    assert calls(E, 4, 100, 2, D, 4097, 2, big_a, 65) == bad  # p = 4097
    assert calls(E, 4, 100, 1, D, 7, 2, A, 1) == bad          # e_wpr < ceil(m / 64)
    assert calls(E, 4, 100, 2, D, 7, 1, A, 1) == bad          # d_wpr < ceil(m / 64)
    assert calls(E, 4, 100, 2, D, 65, 2, A, 1) == bad         # a_wpr < ceil(p / 64)
    assert calls(E, 1 << 31, 100, 2, D, 7, 2, A, 1) == bad    # n = 2^31
    assert calls(None, 4, 100, 2, D, 7, 2, A, 1) == bad       # null matrices with n > 0
    assert calls(E, 4, 100, 2, None, 7, 2, A, 1) == bad
    assert calls(E, 4, 100, 2, D, 7, 2, None, 1) == bad
    it = pybic.C.c_size_t(0)
    assert lib.bic_bsvd_learn_du(h, 2, p_(E), 2, p_(E), 4, 100, 2, p_(D), 7, 2, p_(A), 1, 1,
                                 pybic.C.byref(it)) == pybic.BIC_EINVAL  # du = 2
    assert lib.bic_bsvd_learn_du(h, -1, p_(E), 2, p_(E), 4, 100, 2, p_(D), 7, 2, p_(A), 1, 1,
                                 pybic.C.byref(it)) == pybic.BIC_EINVAL
    assert lib.bic_set_bsvd_rounds(h, 65) == pybic.BIC_EINVAL
    assert lib.bic_set_bsvd_rounds(h, 64) == pybic.BIC_OK and lib.bic_set_bsvd_rounds(h, 0) == pybic.BIC_OK
    # n = 0: nothing to do, changed = 0 and rounds = 0
    ch.fill_(-1)
    rounds = pybic.C.c_size_t(7)
    assert lib.bic_bsvd_update_dictionary_proximus(h, None, 0, 100, 2, p_(D), 7, 2, None, 1, p_(ch),
                                                   pybic.C.byref(rounds)) == pybic.BIC_OK
    assert int(as_u64(ch)[0]) == 0 and rounds.value == 0
    assert lib.bic_bsvd_update_dictionary_proximus(h, None, 0, 100, 2, p_(D), 7, 2, None, 1, None,
                                                   None) == pybic.BIC_OK
    ctx.sync()
