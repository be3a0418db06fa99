"""Binary dictionary learning on the device (bic_bsvd.hip, include/bic.h bic_bsvd_update_coefficients /
bic_bsvd_update_dictionary / bic_bsvd_learn) against the numpy restatement of bsvd.cpp's three functions
(tests/bsvd_ref.py, pinned by tests/test_bsvd_ref.py). Bit-exact over every word of E, D and A, on planted
data (bsvd_ref.planted) whose restatement counts are asserted before they are used, so no comparison can
pass on a step that does nothing."""
import functools

import numpy as np
import pytest

import bsvd_ref as R
import pybic
from pybic import GF2_AB, as_u64

pytestmark = pytest.mark.gpu

# (n, m, p): one bit; ragged words; whole words and p on a word boundary; one word, ragged p; five words
# and p past 256; rows of 64 words with D streamed in two tiles of which the second holds one atom; the
# shape whose atoms (160 KiB) cannot be resident in LDS
SHAPES = [(1, 1, 1), (130, 100, 7), (257, 256, 64), (300, 64, 33), (130, 320, 300), (64, 4096, 65), (130, 320, 4096)]
TIES = {(130, 100, 7), (257, 256, 64), (300, 64, 33)}  # shapes whose first pass meets ties at the minimum


def start(n, m, p, a_flips=0.0):
    if (n, m, p) == (1, 1, 1):  # the one bit set and the one atom equal to it: a step to weight 0
        X = np.zeros((1, 64), np.uint8)
        X[0, 0] = 1
        return X, X.copy(), np.zeros((1, 64), np.uint8), X.copy()
    return R.planted(1, n, m, p, a_flips=a_flips)


@functools.lru_cache(maxsize=None)
def case(n, m, p, a_flips=0.0):
    """the planted start, the restatement's state after the sparse-coding step and after the dictionary
    step that follows it, with their counts; computed once, never modified (callers copy)"""
    X, D0, A0, E0 = start(n, m, p, a_flips)
    E1, A1, st = E0.copy(), A0.copy(), {}
    c1 = R.update_coefficients_argmin(E1, D0, A1, p, st)
    E2, D2 = E1.copy(), D0.copy()
    c2 = R.update_dictionary(E2, D2, A1, m, p)
    for a in (X, D0, A0, E0, E1, A1, E2, D2):
        a.setflags(write=False)
    return dict(X=X, D0=D0, A0=A0, E0=E0, E1=E1, A1=A1, c1=c1, st=st, E2=E2, D2=D2, c2=c2)


def dev(ctx, B):
    return ctx.to_dev(R.pack(B))


def same(t, B):
    return np.array_equal(as_u64(t), R.pack(B))


@pytest.mark.parametrize("n,m,p", SHAPES)
def test_coefficients(ctx, n, m, p):
    c = case(n, m, p)
    assert c["c1"] >= max(1, n // 2)  # at least half the rows change
    if (n, m, p) in TIES:
        assert c["st"]["ties"] >= 1
    if n > 1:
        assert c["st"]["multi"] >= 1  # rows that take more than one step
    E, D, A = dev(ctx, c["E0"]), dev(ctx, c["D0"]), dev(ctx, c["A0"])
    assert ctx.bsvd_update_coefficients(E, m, D, A, p) == c["c1"]
    assert same(E, c["E1"]) and same(A, c["A1"]) and same(D, c["D0"])
    assert ctx.bsvd_update_coefficients(E, m, D, A, p) == 0  # a second pass right after changes nothing
    assert same(E, c["E1"]) and same(A, c["A1"])


def test_coefficients_switch_atoms_off(ctx, oracle):
    """a start from a non-zero A (A0 with 5 % of its bits flipped, E = X ^ A D): coefficients go 1 -> 0"""
    n, m, p = 257, 256, 64
    c = case(n, m, p, 0.05)
    assert c["A0"].any() and c["st"]["off"] >= 1 and c["c1"] >= n // 2
    E, D, A = dev(ctx, c["E0"]), dev(ctx, c["D0"]), dev(ctx, c["A0"])
    assert ctx.bsvd_update_coefficients(E, m, D, A, p) == c["c1"]
    assert same(E, c["E1"]) and same(A, c["A1"])
    # the identity E == X ^ A D on the device's output, the product from the oracle's mul_AB
    AD = oracle.gf2_mul(GF2_AB, as_u64(A), n, p, as_u64(D), p, m, np.zeros((n, R.words(m)), np.uint64), n, m)
    assert np.array_equal(as_u64(E), R.pack(c["X"]) ^ AD)
    assert int(c["E1"].sum()) < int(c["E0"].sum())


@pytest.mark.parametrize("n,m,p", SHAPES + [(2500, 130, 40)])
def test_dictionary(ctx, n, m, p):
    """on the sparse-coding step's output. (2500, 130, 40): rows spread over three workgroups, one launch
    per atom, three words per row. (1, 1, 1): the vote of the one user reproduces the atom, nothing changes."""
    c = case(n, m, p)
    assert c["c2"] >= 1 or (n, m, p) == (1, 1, 1)
    E, D, A = dev(ctx, c["E1"]), dev(ctx, c["D0"]), dev(ctx, c["A1"])
    assert ctx.bsvd_update_dictionary(E, m, D, A, p) == c["c2"]
    assert same(E, c["E2"]) and same(D, c["D2"]) and same(A, c["A1"])


def test_dictionary_counts_across_workgroups(ctx):
    """n = 70000, m = 64, p = 5 with atom 0 used by every row: its usage and column counts pass 16 bits and
    are summed over many workgroups. Column 0 is 1 in every sample and 0 in every atom, column 1 is 0 in every
    sample and 1 in atom 0 alone: E's count is 70000 in both, read as it is where D_0's bit is 0 and as
    U - count where it is 1."""
    n, m, p = 70000, 64, 5
    X, D, A, _ = R.planted(3, n, m, p, a_flips=0.05)
    A[:, 0] = 1
    X[:, 0], X[:, 1], D[:, 0], D[:, 1], D[0, 1] = 1, 0, 0, 0, 1
    E = R.residual(X, D, A, p)
    dE, dD, dA = dev(ctx, E), dev(ctx, D), dev(ctx, A)
    st = {}
    c2 = R.update_dictionary(E, D, A, m, p, st)
    assert c2 >= 1 and st["max_usage"] == n and st["max_count"] > 65535
    assert ctx.bsvd_update_dictionary(dE, m, dD, dA, p) == c2
    assert same(dE, E) and same(dD, D) and same(dA, A)


@pytest.mark.parametrize("n,m,p", [(257, 256, 64), (300, 64, 33)])
def test_learn(ctx, n, m, p):
    c = case(n, m, p)
    X, D, A, E = (c[k].copy() for k in ("X", "D0", "A0", "E0"))
    it = R.learn(X, E, D, A, m, p)
    assert 2 <= it <= 6
    dX, dD, dA = dev(ctx, c["X"]), dev(ctx, c["D0"]), dev(ctx, c["A0"])
    dE = ctx.to_dev(np.full((n, R.words(m)), 0x5555555555555555, np.uint64))  # E is formed by the call
    assert ctx.bsvd_learn(dX, dE, m, dD, dA, p) == it
    assert same(dE, E) and same(dD, D) and same(dA, A) and same(dX, c["X"])


def test_learn_max_iter(ctx):
    """max_iter = 1 stops after one iteration, in the state one sparse-coding and one dictionary step leave"""
    n, m, p = 257, 256, 64
    c = case(n, m, p)
    assert c["c1"] + c["c2"] > 0  # the uncapped loop would go on
    dX, dD, dA, dE = dev(ctx, c["X"]), dev(ctx, c["D0"]), dev(ctx, c["A0"]), ctx.empty_i64(n, R.words(m))
    assert ctx.bsvd_learn(dX, dE, m, dD, dA, p, max_iter=1) == 1
    assert same(dE, c["E2"]) and same(dD, c["D2"]) and same(dA, c["A1"])


def test_padding_and_pitch(ctx):
    """m = 100, p = 7 with dirty padding bits in X, E, D and A and pitched rows filled with random words: the
    steps run over whole words (the restatement on its 128-bit rows), the padding bits of D and A and the
    words past each row's own come back unchanged"""
    n, m, p = 130, 100, 7
    rng = np.random.default_rng(9)
    X, D, A, _ = (a.copy() for a in R.planted(1, n, m, p))
    X[:, m:] = rng.random(X[:, m:].shape) < 0.3
    D[:, m:] = rng.random(D[:, m:].shape) < 0.3
    A[:, p:] = rng.random(A[:, p:].shape) < 0.3
    E = R.residual(X, D, A, p)  # (A's padding takes no part in the product)
    assert E[:, m:].any() and D[:, m:].any() and A[:, p:].any()

    def pitched(B, extra):
        W = R.pack(B)
        tail = rng.integers(0, 1 << 63, (W.shape[0], extra), dtype=np.uint64)
        return ctx.to_dev(np.concatenate([W, tail], axis=1)), tail

    def check(t, B, tail):
        got = as_u64(t)
        w = got.shape[1] - tail.shape[1]
        return np.array_equal(got[:, :w], R.pack(B)) and np.array_equal(got[:, w:], tail)

    (dE, tE), (dD, tD), (dA, tA), (dX, tX) = pitched(E, 3), pitched(D, 1), pitched(A, 2), pitched(X, 5)
    E1, A1, st = E.copy(), A.copy(), {}
    c1 = R.update_coefficients(E1, D, A1, p, st)
    assert c1 >= n // 2 and np.array_equal(A1[:, p:], A[:, p:])
    assert ctx.bsvd_update_coefficients(dE, m, dD, dA, p) == c1
    assert check(dE, E1, tE) and check(dA, A1, tA) and check(dD, D, tD)
    E2, D2 = E1.copy(), D.copy()
    c2 = R.update_dictionary(E2, D2, A1, m, p)
    assert c2 >= 1 and np.array_equal(D2[:, m:], D[:, m:])
    assert ctx.bsvd_update_dictionary(dE, m, dD, dA, p) == c2
    assert check(dE, E2, tE) and check(dD, D2, tD) and check(dA, A1, tA)
    # the whole loop from the same start, E formed by the call
    (dE, tE), (dD, tD), (dA, tA) = pitched(np.ones_like(E), 3), pitched(D, 1), pitched(A, 2)
    El, Dl, Al = E.copy(), D.copy(), A.copy()
    it = R.learn(X, El, Dl, Al, m, p, coef=R.update_coefficients)
    assert ctx.bsvd_learn(dX, dE, m, dD, dA, p) == it
    assert check(dE, El, tE) and check(dD, Dl, tD) and check(dA, Al, tA) and check(dX, X, tX)


def test_rows_past_one_grid(ctx):
    """n = 16,777,025: 65 rows more than one launch of the transpose (65,535 x 4 blocks of 64 rows) or of the
    product (65,535 x 256 rows) holds, so both go in two row chunks, the second of two words of A's transpose
    with one row in the last. 200 planted rows (m = 64, p = 3) sit at the matrix's first row, on both sides of
    the chunk boundary, at its last row and at random places; every other row of X is zero, has weight 0 under
    A = 0, takes no step and is nobody's user, so the restatement of the 200 rows is that of the whole."""
    torch = ctx.torch
    n, m, p, ns = 65535 * 256 + 65, 64, 3, 200
    X, D, A, E = R.planted(4, ns, m, p)
    Xs = X.copy()
    it = R.learn(X, E, D, A, m, p)
    moved = np.flatnonzero(A[:, :p].any(axis=1))
    assert it >= 2 and len(moved) >= ns // 2
    rng = np.random.default_rng(11)
    where = rng.choice(n, ns + 4, replace=False)
    edge = [0, 65535 * 256 - 1, 65535 * 256, n - 1]
    where = where[~np.isin(where, edge)][:ns]
    where[moved[:4]] = edge  # rows that take steps and end up as users
    idx = torch.from_numpy(where).to(ctx.dev)

    def full(B, wpr):
        t = torch.zeros(n, wpr, dtype=torch.int64, device=ctx.dev)
        t[idx] = dev(ctx, B)
        return t

    dX, dA, dE, dD = full(Xs, 1), full(np.zeros_like(A), 1), ctx.empty_i64(n, 1), dev(ctx, R.planted(4, ns, m, p)[1])
    assert ctx.bsvd_learn(dX, dE, m, dD, dA, p) == it
    assert same(dD, D)
    assert torch.equal(dE, full(E, 1)) and torch.equal(dA, full(A, 1)) and torch.equal(dX, full(Xs, 1))


def test_arguments(ctx):
    lib, h = ctx.lib, ctx.h
    E, D, A = ctx.empty_i64(4, 2), ctx.empty_i64(7, 2), ctx.empty_i64(4, 1)
    big_e, big_d, big_a = ctx.empty_i64(4, 65), ctx.empty_i64(7, 65), ctx.empty_i64(4, 65)
    ch = ctx.empty_i64(1)
    p_ = lambda t: pybic._p(t)
    ctx._bind_stream()

    def calls(e, n, m, e_wpr, d, p, d_wpr, a, a_wpr):
        it = pybic.C.c_size_t(0)
        return (lib.bic_bsvd_update_coefficients(h, p_(e), n, m, e_wpr, p_(d), p, d_wpr, p_(a), a_wpr, p_(ch)),
                lib.bic_bsvd_update_dictionary(h, p_(e), n, m, e_wpr, p_(d), p, d_wpr, p_(a), a_wpr, p_(ch)),
                lib.bic_bsvd_learn(h, p_(e), e_wpr, p_(e), n, m, e_wpr, p_(d), p, d_wpr, p_(a), a_wpr, 1,
                                   pybic.C.byref(it)))

    bad = (pybic.BIC_EINVAL,) * 3
    assert calls(E, 4, 0, 2, D, 7, 2, A, 1) == bad            # m = 0
    assert calls(big_e, 4, 4097, 65, big_d, 7, 65, A, 1) == bad  # m = 4097
    assert calls(E, 4, 100, 2, D, 0, 2, A, 1) == bad          # p = 0
    assert calls(E, 4, 100, 2, D, 4097, 2, big_a, 65) == bad  # p = 4097
    assert calls(E, 4, 100, 1, D, 7, 2, A, 1) == bad          # e_wpr < ceil(m / 64)
    assert calls(E, 4, 100, 2, D, 7, 1, A, 1) == bad          # d_wpr < ceil(m / 64)
    assert calls(E, 4, 100, 2, D, 65, 2, A, 1) == bad         # a_wpr < ceil(p / 64)
    assert calls(E, 1 << 31, 100, 2, D, 7, 2, A, 1) == bad    # n = 2^31
    # n = 0: nothing to do, changed = 0
    ch.fill_(-1)
    assert lib.bic_bsvd_update_coefficients(h, None, 0, 100, 2, p_(D), 7, 2, None, 1, p_(ch)) == pybic.BIC_OK
    assert int(as_u64(ch)[0]) == 0
    ch.fill_(-1)
    assert lib.bic_bsvd_update_dictionary(h, None, 0, 100, 2, p_(D), 7, 2, None, 1, p_(ch)) == pybic.BIC_OK
    assert int(as_u64(ch)[0]) == 0
    assert lib.bic_bsvd_update_coefficients(h, None, 0, 100, 2, p_(D), 7, 2, None, 1, None) == pybic.BIC_OK
    ctx.sync()


def test_capture(ctx):
    """both steps take part in a stream capture once a first call has sized the scratch; every replay redoes
    them on the tensors' contents of the moment"""
    import torch
    n, m, p = 257, 256, 64
    c = case(n, m, p)
    E, D, A = dev(ctx, c["E0"]), dev(ctx, c["D0"]), dev(ctx, c["A0"])
    ch1, ch2 = ctx.empty_i64(1), ctx.empty_i64(1)
    ctx.bsvd_update_coefficients(E, m, D, A, p, changed=ch1)  # eager: the dictionary step's scratch gets its size
    ctx.bsvd_update_dictionary(E, m, D, A, p, changed=ch2)
    ctx.sync()
    torch.cuda.synchronize()
    assert same(E, c["E2"]) and same(D, c["D2"])
    side = torch.cuda.Stream(ctx.dev)
    side.wait_stream(torch.cuda.current_stream(ctx.dev))
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(gr, stream=side):
            ctx.bsvd_update_coefficients(E, m, D, A, p, changed=ch1)
            ctx.bsvd_update_dictionary(E, m, D, A, p, changed=ch2)
    torch.cuda.current_stream(ctx.dev).wait_stream(side)
    torch.cuda.synchronize()
    for rep in range(2):
        E.copy_(dev(ctx, c["E0"]))
        D.copy_(dev(ctx, c["D0"]))
        A.copy_(dev(ctx, c["A0"]))
        ch1.fill_(-1)
        ch2.fill_(-1)
        gr.replay()
        torch.cuda.synchronize()
        assert (int(as_u64(ch1)[0]), int(as_u64(ch2)[0])) == (c["c1"], c["c2"]), rep
        assert same(E, c["E2"]) and same(D, c["D2"]) and same(A, c["A1"]), rep
