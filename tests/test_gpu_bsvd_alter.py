"""The role-switching learners on the device (include/bic.h bic_bsvd_learn_lm: learn_model_alter1 / 2 / 3 of
bsvd.cpp:1247-1434 over the narrow and the wide steps and bic_gf2_transpose) against the numpy restatement
(tests/bsvd_alter_ref.py, pinned by tests/test_bsvd_alter_ref.py). Bit-exact over every word of E, D and A, with
the reference's return value. The transposed width of the first three shapes is just over 4,096, so the exchanged
role runs the wide kernels and the direct one the narrow ones; the fourth runs the narrow ones in both."""
import numpy as np
import pytest

import bsvd_alter_ref as L
import bsvd_ref as R
import pybic
from pybic import as_u64
from test_bsvd_alter_ref import ALTER_SHAPES, ALTER_WIDE, SEED, alter_case, alter_start, nonvacuous_alter

pytestmark = pytest.mark.gpu


def dev(ctx, B):
    return ctx.to_dev(R.pack(B))


def same(t, B):
    return np.array_equal(as_u64(t), R.pack(B))


def scratch_e(ctx, n, m):
    return ctx.to_dev(np.full((n, R.words(m)), 0x5555555555555555, np.uint64))  # E is formed by the call


@pytest.fixture(autouse=True)
def automatic_budget(ctx):
    ctx.set_bsvd_rounds(0)
    yield
    ctx.set_bsvd_rounds(0)


@pytest.mark.parametrize("du", [0, 1])
@pytest.mark.parametrize("lm", [1, 2, 3])
@pytest.mark.parametrize("n,m,p", ALTER_SHAPES)
def test_learners(ctx, n, m, p, lm, du):
    c = alter_case(lm, du, n, m, p)
    if lm == 1:
        nonvacuous_alter()
        tr = c["trace"]
        assert sum(x[2] for x in tr if x[:2] == ("t", "c")) >= 1 and sum(x[2] for x in tr if x[:2] == ("t", "u")) >= 1
        if (n, m, p, du) == (4200, 100, 7, 0):  # alter1's quirk: it stops although the direct coding still moved
            assert tr[-4][:2] == ("d", "c") and tr[-4][2] >= 1 and tr[-1] == ("t", "u", 0)
    dX, dD, dA, dE = dev(ctx, c["X"]), dev(ctx, c["D0"]), dev(ctx, c["A0"]), scratch_e(ctx, n, m)
    assert ctx.bsvd_learn(dX, dE, m, dD, dA, p, du=du, lm=lm) == c["it"]
    assert same(dE, c["E"]) and same(dD, c["D"]) and same(dA, c["A"]) and same(dX, c["X"])


@pytest.mark.parametrize("lm", [1, 2, 3])
def test_max_iter(ctx, lm):
    """max_iter = 1: one pass of the text, finished with its transposes back (alter2: one direct pass)"""
    n, m, p = ALTER_WIDE[0]
    c = alter_case(lm, 0, n, m, p, 1)
    assert c["it"] == 1 and len(alter_case(lm, 0, n, m, p)["trace"]) > len(c["trace"])  # uncapped: more passes
    dX, dD, dA, dE = dev(ctx, c["X"]), dev(ctx, c["D0"]), dev(ctx, c["A0"]), scratch_e(ctx, n, m)
    assert ctx.bsvd_learn(dX, dE, m, dD, dA, p, max_iter=1, lm=lm) == 1
    assert same(dE, c["E"]) and same(dD, c["D"]) and same(dA, c["A"])


@pytest.mark.parametrize("lm,du", [(1, 0), (3, 1)])
def test_dirty_padding_comes_back_zero(ctx, lm, du):
    """dirty padding bits in X, D and A and pitched rows: the first direct steps see them, the transposes clear
    them, and the words past every row's own come back as they were"""
    n, m, p = 4200, 100, 7
    rng = np.random.default_rng(9)
    X, D, A, _ = (a.copy() for a in alter_start(n, m, p, lm))
    X[:, m:] = rng.random(X[:, m:].shape) < 0.3
    D[:, m:] = rng.random(D[:, m:].shape) < 0.3
    A[:, p:] = rng.random(A[:, p:].shape) < 0.3

    def pitched(B, extra):
        W = R.pack(B)
        tail = rng.integers(0, 1 << 63, (W.shape[0], extra), dtype=np.uint64)
        return ctx.to_dev(np.concatenate([W, tail], axis=1)), tail

    def check(t, B, tail):
        got = as_u64(t)
        w = got.shape[1] - tail.shape[1]
        return np.array_equal(got[:, :w], R.pack(B)) and np.array_equal(got[:, w:], tail)

    (dX, tX), (dD, tD), (dA, tA) = pitched(X, 1), pitched(D, 1), pitched(A, 2)
    dE, tE = pitched(np.ones_like(X), 3)
    X0, E = X.copy(), np.zeros_like(X)
    it = L.learn(lm, X, E, D, A, m, p, du)
    assert not E[:, m:].any() and not D[:, m:].any() and not A[:, p:].any()
    assert ctx.bsvd_learn(dX, dE, m, dD, dA, p, du=du, lm=lm) == it
    assert check(dE, E, tE) and check(dD, D, tD) and check(dA, A, tA) and check(dX, X0, tX)


@pytest.mark.parametrize("du", [0, 1])
def test_traditional_on_wide_rows(ctx, du):
    """lm = 0 at m = 4200: the traditional loop over the wide steps equals the restatement's learn"""
    n, m, p = 70, 4200, 33
    X, D, A, _ = R.planted(SEED, n, m, p)
    D0, A0, E = D.copy(), A.copy(), np.zeros_like(X)
    it = L.learn(0, X, E, D, A, m, p, du)
    assert it >= 2
    dX, dD, dA, dE = dev(ctx, X), dev(ctx, D0), dev(ctx, A0), scratch_e(ctx, n, m)
    assert ctx.bsvd_learn(dX, dE, m, dD, dA, p, du=du, lm=0) == it
    assert same(dE, E) and same(dD, D) and same(dA, A)


def test_traditional_is_bsvd_learn_du(ctx):
    """lm = 0 at m <= 4096 is bic_bsvd_learn_du"""
    n, m, p = 300, 64, 33
    X, D0, A0, _ = R.planted(SEED, n, m, p)
    out = []
    for lm_entry in (False, True):
        dX, dD, dA, dE = dev(ctx, X), dev(ctx, D0), dev(ctx, A0), scratch_e(ctx, n, m)
        it = pybic.C.c_size_t(0)
        args = (pybic._p(dX), dX.shape[1], pybic._p(dE), n, m, dE.shape[1], pybic._p(dD), p, dD.shape[1],
                pybic._p(dA), dA.shape[1], 0, pybic.C.byref(it))
        ctx._bind_stream()
        if lm_entry:
            assert ctx.lib.bic_bsvd_learn_lm(ctx.h, 0, 1, *args) == pybic.BIC_OK
        else:
            assert ctx.lib.bic_bsvd_learn_du(ctx.h, 1, *args) == pybic.BIC_OK
        out.append((it.value, as_u64(dE).copy(), as_u64(dD).copy(), as_u64(dA).copy()))
    assert out[0][0] == out[1][0] >= 2
    assert all(np.array_equal(a, b) for a, b in zip(out[0][1:], out[1][1:]))


def test_arguments(ctx):
    lib, h, C = ctx.lib, ctx.h, pybic.C
    X, E, D, A = ctx.empty_i64(4, 2), ctx.empty_i64(4, 2), ctx.empty_i64(7, 2), ctx.empty_i64(4, 1)
    p_ = lambda t: None if t is None else pybic._p(t)
    ctx._bind_stream()

    def call(lm, du, x, e, n, m, wpr, d, p, a):
        it = C.c_size_t(0)
        return lib.bic_bsvd_learn_lm(h, lm, du, p_(x), wpr, p_(e), n, m, wpr, p_(d), p, wpr, p_(a), 1, 1, C.byref(it))

    bad = pybic.BIC_EINVAL
    assert call(4, 0, X, E, 4, 100, 2, D, 7, A) == bad and call(-1, 0, X, E, 4, 100, 2, D, 7, A) == bad  # lm
    for lm in (0, 1, 2, 3):
        assert call(lm, 2, X, E, 4, 100, 2, D, 7, A) == bad               # du
        assert call(lm, 0, X, E, 4, 0, 2, D, 7, A) == bad                 # m = 0
        assert call(lm, 0, X, E, 4, 1048577, 16385, D, 7, A) == bad       # m = 1,048,577
        assert call(lm, 0, X, E, 4, 100, 2, D, 4097, A) == bad            # p = 4097
        assert call(lm, 0, X, E, 4, 100, 1, D, 7, A) == bad               # short pitches
        assert call(lm, 0, None, E, 4, 100, 2, D, 7, A) == bad            # null matrices
        assert call(lm, 0, X, E, 4, 100, 2, None, 7, A) == bad
    for lm in (1, 2, 3):
        assert call(lm, 0, X, E, 1048577, 100, 2, D, 7, A) == bad         # n = 1,048,577 for lm >= 1
        assert call(lm, 0, X, E, 0, 100, 2, D, 7, A) == bad               # n = 0 for lm >= 1
    assert call(0, 0, X, E, 0, 100, 2, D, 7, A) == pybic.BIC_OK           # the traditional loop takes n = 0
    ctx.sync()
