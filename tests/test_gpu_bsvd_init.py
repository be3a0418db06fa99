"""The model initialisers on the device (bic_bsvd.hip k_bsvd_init*, include/bic.h "model initialisers") against the
numpy restatement of bsvd.cpp:99-267 (tests/bsvd_init_ref.py, pinned by tests/test_bsvd_init_ref.py). Bit-exact
over every word of D and A: their own words start as all ones, so the clears are tested, and their rows are
pitched, the words past a row's own holding a sentinel that must survive. E is pitched too and its padding bits
are all ones. Every comparison comes after the restatement's stats for the case have been asserted."""
import numpy as np
import pytest

import bsvd_init_ref as I
import bsvd_ref as R
import pybic
from pybic import as_u64
from test_bsvd_init_ref import SHAPES, case, nonvacuous

pytestmark = pytest.mark.gpu

RULES = [I.NEIGHBOR, I.PARTITION, I.CENTROIDS, I.CENTROIDS_XOR]
ONES, SENTINEL = np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(0x5A5A5A5A5A5A5A5A)


@pytest.fixture(autouse=True)
def cases_exercise_the_rules():
    nonvacuous()  # (cached after the first test)


def dev_E(ctx, E):
    """E with one more word per row than its own, all ones"""
    W = R.pack(E)
    return ctx.to_dev(np.concatenate([W, np.full((W.shape[0], 1), ONES)], axis=1))


def outputs(ctx, n, m, p, d_extra=2, a_extra=1):
    """D and A on the device: own words all ones, d_extra / a_extra sentinel words after them"""
    def make(rows, own, extra):
        W = np.full((rows, own + extra), ONES)
        W[:, own:] = SENTINEL
        return ctx.to_dev(W)
    return make(p, R.words(m), d_extra), make(n, R.words(p), a_extra)


def check(t, B):
    """every word of the device tensor: the restatement's bits, then the sentinel"""
    got, want = as_u64(t), R.pack(B)
    w = want.shape[1]
    assert np.array_equal(got[:, :w], want)
    assert (got[:, w:] == SENTINEL).all()


def u32(ctx, a):
    return ctx.to_dev(np.asarray(a, np.uint32))


def explicit(ctx, mi, dE, m, dD, dA, p, st):
    """the rule through its explicit entry with what the restatement drew"""
    if mi == I.NEIGHBOR:
        ctx.bsvd_init_neighbor(dE, m, dD, dA, p, u32(ctx, st["picks"]))
    elif mi == I.PARTITION:
        ctx.bsvd_init_partition(dE, m, dD, dA, p)
    else:
        ctx.bsvd_init_centroids(mi, dE, m, dD, dA, p, u32(ctx, st["assign"]))


@pytest.mark.parametrize("mi", RULES)
@pytest.mark.parametrize("n,m,p", SHAPES)
def test_explicit_entries(ctx, n, m, p, mi):
    c = case(n, m, p)
    want = c[mi]
    if mi == I.NEIGHBOR:
        assert len(want["st"]["picks"]) == p
    dE = dev_E(ctx, c["E"])
    dD, dA = outputs(ctx, n, m, p)
    explicit(ctx, mi, dE, m, dD, dA, p, want["st"])
    check(dD, want["D"])
    check(dA, want["A"])
    assert np.array_equal(as_u64(dE)[:, :-1], R.pack(c["E"]))  # E is const


def test_neighbor_picks_chosen_by_the_test(ctx):
    """the three lonely rows (u = 1: all ones), a zero row (the atom stays zero), the same row twice"""
    n, m = 257, 256
    c = case(n, m, 64)
    picks = c["lonely"] + [16, 40, 40]
    st = {}
    D, A = I.initialize_neighbor(c["E"], m, len(picks), picks=picks, stats=st)
    assert st["u1"] == 3 and D[:3, :m].all() and not c["E"][16, :m].any() and not D[3].any()
    assert D[4].any() and np.array_equal(D[4], D[5]) and st["max_u"] > 31
    dE = dev_E(ctx, c["E"])
    dD, dA = outputs(ctx, n, m, len(picks))
    ctx.bsvd_init_neighbor(dE, m, dD, dA, len(picks), u32(ctx, picks))
    check(dD, D)
    check(dA, A)


def test_partition_more_atoms_than_columns_and_a_zero_column(ctx):
    n, m, p = 130, 40, 70
    E = I.clustered(7, n, m)[0].copy()
    E[:, 7] = 0
    st = {}
    D, A = I.initialize_partition(E, m, p, stats=st)
    k7 = st["pivots"].index(7)
    assert st["zero_pivots"] >= 1 and D[k7, :m].all() and not D[m:].any() and D[:m].any(axis=1).all()
    dE = dev_E(ctx, E)
    dD, dA = outputs(ctx, n, m, p)
    ctx.bsvd_init_partition(dE, m, dD, dA, p)
    check(dD, D)
    check(dA, A)


@pytest.mark.parametrize("mi", RULES)
@pytest.mark.parametrize("n,m,p", SHAPES)
def test_initialize_draws_as_the_restatement(ctx, n, m, p, mi):
    """bic_bsvd_initialize from random_seed: the device result and the state afterwards"""
    c = case(n, m, p)
    want = c[mi]
    dE = dev_E(ctx, c["E"])
    dD, dA = outputs(ctx, n, m, p)
    state = ctx.bsvd_initialize(mi, dE, m, dD, dA, p, pybic.bsvd_rng_seed(I.RANDOM_SEED))
    assert state == want["state"]
    assert (state == I.Rand48().state) == (mi == I.PARTITION)  # the other rules drew
    check(dD, want["D"])
    check(dA, want["A"])


def test_initialize_continues_one_state(ctx):
    """two calls in sequence from one state, as two calls of the reference share its generator"""
    n, m, p = 300, 64, 33
    c = case(n, m, p)
    r, st1 = I.Rand48(), {}
    D1, A1 = I.initialize(I.NEIGHBOR, c["E"], m, p, r, st1)
    mid = r.state
    D2, A2 = I.initialize(I.CENTROIDS, c["E"], m, p, r)
    assert st1["redraws"] >= 1 and not np.array_equal(A2, c[I.CENTROIDS]["A"])  # not the draws of a fresh state
    dE = dev_E(ctx, c["E"])
    dD, dA = outputs(ctx, n, m, p)
    state = ctx.bsvd_initialize(I.NEIGHBOR, dE, m, dD, dA, p, pybic.bsvd_rng_seed(I.RANDOM_SEED))
    assert state == mid
    check(dD, D1)
    check(dA, A1)
    state = ctx.bsvd_initialize(I.CENTROIDS, dE, m, dD, dA, p, state)  # (over the first call's D and A)
    assert state == r.state
    check(dD, D2)
    check(dA, A2)
    assert ctx.bsvd_initialize(I.PARTITION, dE, m, dD, dA, p) is None  # no state needed
    check(dD, c[I.PARTITION]["D"])
    check(dA, c[I.PARTITION]["A"])


def test_index_out_of_range_is_skipped(ctx):
    """a pick equal to n leaves its atom zero; an atom index equal to p leaves its row of A zero and joins no
    atom: what include/bic.h documents, in arrays this test owns"""
    n, m, p = 300, 64, 33
    c = case(n, m, p)
    picks = list(c[I.NEIGHBOR]["st"]["picks"])
    picks[5] = n
    D, A = I.initialize_neighbor(c["E"], m, p, picks=picks)
    assert not D[5].any() and D[4].any()
    dE = dev_E(ctx, c["E"])
    dD, dA = outputs(ctx, n, m, p)
    ctx.bsvd_init_neighbor(dE, m, dD, dA, p, u32(ctx, picks))
    check(dD, D)
    check(dA, A)
    assign = c[I.CENTROIDS]["st"]["assign"].copy()
    assign[[0, 77]] = p
    for mi in (I.CENTROIDS, I.CENTROIDS_XOR):
        D, A = I.initialize_centroids(c["E"], m, p, assign=assign, xor=mi == I.CENTROIDS_XOR)
        assert not A[0].any() and not A[77].any() and A[1].any()
        dD, dA = outputs(ctx, n, m, p)
        ctx.bsvd_init_centroids(mi, dE, m, dD, dA, p, u32(ctx, assign))
        check(dD, D)
        check(dA, A)


@pytest.mark.parametrize("mi", [I.NEIGHBOR, I.CENTROIDS])
def test_initialize_then_learn(ctx, mi):
    """the reference's driver: E = X, initialize_model(E, D, A), learn_model(X, E, D, A)"""
    n, m, p = 257, 256, 64
    c = case(n, m, p)
    X = c["E"]
    D, A = (a.copy() for a in (c[mi]["D"], c[mi]["A"]))
    E = X.copy()
    it = R.learn(X, E, D, A, m, p)
    assert it >= 2 and E.sum() < X.sum()
    dX = ctx.to_dev(R.pack(X))
    dD, dA = outputs(ctx, n, m, p, 0, 0)
    state = ctx.bsvd_initialize(mi, dX, m, dD, dA, p, pybic.bsvd_rng_seed(I.RANDOM_SEED))
    assert state == c[mi]["state"]
    dE = dX.clone()
    assert ctx.bsvd_learn(dX, dE, m, dD, dA, p) == it
    assert np.array_equal(as_u64(dE), R.pack(E)) and np.array_equal(as_u64(dD), R.pack(D))
    assert np.array_equal(as_u64(dA), R.pack(A))


def test_arguments(ctx):
    lib, h, C = ctx.lib, ctx.h, pybic.C
    E, D, A = ctx.to_dev(np.full((4, 2), ONES)), ctx.empty_i64(7, 2), ctx.empty_i64(4, 1)
    big_e, big_d, big_a = ctx.empty_i64(4, 65), ctx.empty_i64(7, 65), ctx.empty_i64(4, 65)
    sel = u32(ctx, [0] * 8)
    p_ = lambda t: None if t is None else pybic._p(t)
    ctx._bind_stream()
    st = C.c_uint64(pybic.bsvd_rng_seed(1))

    def calls(e, n, m, e_wpr, d, p, d_wpr, a, a_wpr):
        g = (p_(e), n, m, e_wpr, p_(d), p, d_wpr, p_(a), a_wpr)
        return (lib.bic_bsvd_init_neighbor(h, *g, p_(sel)), lib.bic_bsvd_init_partition(h, *g),
                lib.bic_bsvd_init_centroids(h, 2, *g, p_(sel)), lib.bic_bsvd_init_centroids(h, 3, *g, p_(sel)),
                lib.bic_bsvd_initialize(h, 0, *g, C.byref(st)), lib.bic_bsvd_initialize(h, 1, *g, None),
                lib.bic_bsvd_initialize(h, 2, *g, C.byref(st)), lib.bic_bsvd_initialize(h, 3, *g, C.byref(st)))

    bad = (pybic.BIC_EINVAL,) * 8
    assert calls(E, 0, 100, 2, D, 7, 2, A, 1) == bad            # n = 0
    assert calls(E, 4, 0, 2, D, 7, 2, A, 1) == bad              # m = 0
    assert calls(big_e, 4, 4097, 65, big_d, 7, 65, A, 1) == bad  # m = 4097
    assert calls(E, 4, 100, 2, D, 0, 2, A, 1) == bad            # p = 0
    assert calls(E, 4, 100, 2, D, 4097, 2, big_a, 65) == bad    # p = 4097
    assert calls(E, 4, 100, 1, D, 7, 2, A, 1) == bad            # e_wpr < ceil(m / 64)
    assert calls(E, 4, 100, 2, D, 7, 1, A, 1) == bad            # d_wpr < ceil(m / 64)
    assert calls(E, 4, 100, 2, D, 65, 2, A, 1) == bad           # a_wpr < ceil(p / 64)
    assert calls(E, 1 << 31, 100, 2, D, 7, 2, A, 1) == bad      # n = 2^31
    assert calls(None, 4, 100, 2, D, 7, 2, A, 1) == bad         # null matrices
    assert calls(E, 4, 100, 2, None, 7, 2, A, 1) == bad
    assert calls(E, 4, 100, 2, D, 7, 2, None, 1) == bad
    good = (p_(E), 4, 100, 2, p_(D), 7, 2, p_(A), 1)
    for mi in (-1, 4):                                          # a bad mi
        assert lib.bic_bsvd_initialize(h, mi, *good, C.byref(st)) == pybic.BIC_EINVAL
    for mi in (0, 1, 4):
        assert lib.bic_bsvd_init_centroids(h, mi, *good, p_(sel)) == pybic.BIC_EINVAL
    for mi in (0, 2, 3):                                        # NULL state where one is needed
        assert lib.bic_bsvd_initialize(h, mi, *good, None) == pybic.BIC_EINVAL
    assert lib.bic_bsvd_init_neighbor(h, *good, None) == pybic.BIC_EINVAL  # null indices
    assert lib.bic_bsvd_init_centroids(h, 2, *good, None) == pybic.BIC_EINVAL
    assert st.value == pybic.bsvd_rng_seed(1)                   # no refused call drew
    # an all-zero E over j < m (its padding bits are set): the neighbour rule has nothing to pick, no draw is made
    Z = np.zeros((4, 128), np.uint8)
    Z[:, 100:] = 1
    dZ = ctx.to_dev(R.pack(Z))
    assert lib.bic_bsvd_initialize(h, 0, p_(dZ), 4, 100, 2, p_(D), 7, 2, p_(A), 1, C.byref(st)) == pybic.BIC_EINVAL
    assert st.value == pybic.bsvd_rng_seed(1)
    assert lib.bic_bsvd_initialize(h, 2, p_(dZ), 4, 100, 2, p_(D), 7, 2, p_(A), 1, C.byref(st)) == pybic.BIC_OK
    assert st.value != pybic.bsvd_rng_seed(1)
    ctx.sync()
