"""The MDL model-order searches on the device (include/bic.h "MDL model order": bic_bsvd_model_weights,
bic_bsvd_drop_weights, bic_bsvd_drop_atom, bic_bsvd_append_atom, bic_bsvd_model_codelength, bic_bsvd_learn_mdl)
against the restatement of bsvd.cpp:1438-1717 (tests/bsvd_mdl_ref.py, pinned by tests/test_bsvd_mdl_ref.py).
Bit-exact over every word, with the returned numbers, the generator's state and the full trace."""
import numpy as np
import pytest

import bsvd_init_ref as I
import bsvd_mdl_ref as M
import bsvd_ref as R
import pybic
from bsvd_ref import words
from pybic import as_u64
from test_bsvd_mdl_ref import PRIM_SHAPES, SEED, nonvacuous, prim_case

pytestmark = pytest.mark.gpu


def pitched(ctx, B, extra, seed=3):
    """B packed, with `extra` words of noise after every row -> (device tensor, the noise)"""
    W = R.pack(B)
    tail = np.random.default_rng(seed).integers(0, 1 << 63, (W.shape[0], extra), dtype=np.uint64)
    return ctx.to_dev(np.concatenate([W, tail], axis=1)), tail


def check(t, B, tail):
    """the device tensor holds B's words and its noise untouched"""
    got = as_u64(t)
    w = got.shape[1] - tail.shape[1]
    return np.array_equal(got[:, :w], R.pack(B)) and np.array_equal(got[:, w:], tail)


@pytest.mark.parametrize("n,m,p", PRIM_SHAPES)
def test_weights_and_removal_scores(ctx, n, m, p):
    """dirty padding in E, D and A and pitched rows; an unused atom and one that every row uses"""
    c = prim_case(n, m, p)
    assert all(B[:, c0:].any() for B, c0 in ((c["E"], m), (c["D"], m), (c["A"], p)) if c0 % 64)
    (dE, tE), (dD, tD), (dA, tA) = pitched(ctx, c["E"], 2), pitched(ctx, c["D"], 1), pitched(ctx, c["A"], 3)
    we, wd, wa = ctx.model_weights_host(ctx.bsvd_model_weights(dE, m, dD, dA, p), p)
    rwe, rwd, rwa = c["weights"]
    assert we == rwe and np.array_equal(wd, rwd) and np.array_equal(wa, rwa)
    assert wa[1] == 0 and wa[2] == n
    got = as_u64(ctx.bsvd_drop_weights(dE, m, dD, dA, p))
    assert got.tolist() == c["drop"]
    assert check(dE, c["E"], tE) and check(dD, c["D"], tD) and check(dA, c["A"], tA)  # only read


def test_weights_without_atoms(ctx):
    n, m, p = PRIM_SHAPES[3]
    c = prim_case(n, m, p)
    dE, _ = pitched(ctx, c["E"], 1)
    out = ctx.empty_i64(2)
    out.fill_(-1)
    ctx.bsvd_model_weights(dE, m, None, None, 0, out=out)
    got = as_u64(out)
    assert int(got[0]) == c["weights"][0] and int(got[1]) == (1 << 64) - 1
    assert ctx.bsvd_model_codelength(dE, m, None, None, 0) == M.length_e(n, m, c["weights"][0])


def test_removal_scores_many_wide_atoms(ctx):
    """p = 130 at m = 4200: 130 x 66 words of atoms, more than one workgroup's LDS could stage"""
    n, m, p = 70, 4200, 130
    X, D, A, E = (a.copy() for a in R.planted(SEED, n, m, p, a_flips=0.05))
    E[:, m:] = 1
    want = M.drop_weights(E, D, A, m, p)
    assert len(set(want)) > 10
    dE, dD, dA = (ctx.to_dev(R.pack(B)) for B in (E, D, A))
    assert as_u64(ctx.bsvd_drop_weights(dE, m, dD, dA, p)).tolist() == want
    we, wd, wa = ctx.model_weights_host(ctx.bsvd_model_weights(dE, m, dD, dA, p), p)
    rwe, rwd, rwa = M.model_weights(E, D, A, m, p)
    assert we == rwe and np.array_equal(wd, rwd) and np.array_equal(wa, rwa)


@pytest.mark.parametrize("n,m,p", [(300, 100, 7), (257, 130, 70)])
def test_model_codelength(ctx, n, m, p):
    """the blocking call with the reference's truncations (shapes whose doubles pass the restatement's guard)"""
    c = prim_case(n, m, p)
    dE, dD, dA = (ctx.to_dev(R.pack(c[k])) for k in "EDA")
    want = M.codelength_from_weights(n, m, *c["weights"])
    assert ctx.bsvd_model_codelength(dE, m, dD, dA, p) == want
    LD, LA = M.codelength_sums(n, m, c["weights"][1], c["weights"][2])
    assert want == M.length_e(n, m, c["weights"][0]) + LD + LA


def atom_model(p, cap, seed):
    n, m = 130, 100
    rng = np.random.default_rng(seed)
    D = np.zeros((cap, 128), np.uint8)
    A = np.zeros((n, 64 * words(cap)), np.uint8)
    D[:, :m] = rng.random((cap, m)) < 0.4
    D[:, m:] = rng.random((cap, 28)) < 0.4                 # padding travels with its row
    A[:, :] = rng.random(A.shape) < 0.4                    # dirty padding past p as well
    return n, m, D, A


@pytest.mark.parametrize("p,k", sorted({(p, k) for p in (64, 65, 70) for k in (0, 3, 63, 64, p - 1) if k < p}))
def test_drop_atom(ctx, p, k):
    """the word-boundary carries: columns move across words 0 | 1, the last word empties at p = 65"""
    n, m, D, A = atom_model(p, p, 11)
    (dD, tD), (dA, tA) = pitched(ctx, D, 1), pitched(ctx, A, 2)
    last = D[p - 1].copy()
    ctx.bsvd_drop_atom(dD, m, dA, p, k)
    M.drop_atom(D, A, p, k)
    assert np.array_equal(D[p - 1], last) and not A[:, p - 1:].any()
    assert check(dD, D, tD) and check(dA, A, tA)


@pytest.mark.parametrize("p", [63, 64])
def test_append_atom(ctx, p):
    n, m, D, A = atom_model(p, p + 1, 12)
    rng = np.random.default_rng(13)
    atom = (rng.random((1, 128)) < 0.5).astype(np.uint8)   # dirty past m: masked away
    coefs = (rng.random((n, 128)) < 0.5).astype(np.uint8)  # only bit 63 of each row's first word counts
    (dD, tD), (dA, tA) = pitched(ctx, D, 1), pitched(ctx, A, 1)
    d_atom, d_coefs = ctx.to_dev(R.pack(atom)), ctx.to_dev(R.pack(coefs))
    ctx.bsvd_append_atom(dD, m, dA, p, d_atom, d_coefs)
    before = A.copy()
    M.append_atom(D, A, m, p, atom[0], coefs[:, 0])
    assert atom[0, m:].any() and not D[p, m:].any() and np.array_equal(A[:, :p], before[:, :p])
    assert check(dD, D, tD) and check(dA, A, tA)
    # and out again: the identity on the model of p atoms
    ctx.bsvd_drop_atom(dD, m, dA, p + 1, p)
    M.drop_atom(D, A, p + 1, p)
    assert check(dD, D, tD) and check(dA, A, tA)


def test_capture(ctx):
    """the weights and the scores take part in a stream capture after one warm-up call; a replay recomputes them
    from the tensors' contents of the moment"""
    import torch
    n, m, p = PRIM_SHAPES[0]
    c = prim_case(n, m, p)
    dE, dD, dA = (ctx.to_dev(R.pack(c[k])) for k in "EDA")
    w, s = ctx.empty_i64(1 + p), ctx.empty_i64(p)
    ctx.bsvd_model_weights(dE, m, dD, dA, p, out=w)
    ctx.bsvd_drop_weights(dE, m, dD, dA, p, out=s)
    ctx.sync()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(ctx.dev)
    side.wait_stream(torch.cuda.current_stream(ctx.dev))
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(gr, stream=side):
            ctx.bsvd_model_weights(dE, m, dD, dA, p, out=w)
            ctx.bsvd_drop_weights(dE, m, dD, dA, p, out=s)
    torch.cuda.current_stream(ctx.dev).wait_stream(side)
    torch.cuda.synchronize()
    E2 = c["E"].copy()
    E2[::3, :m] ^= 1
    for E in (c["E"], E2):
        dE.copy_(ctx.to_dev(R.pack(E)))
        w.fill_(-1)
        s.fill_(-1)
        gr.replay()
        torch.cuda.synchronize()
        we, wd, wa = ctx.model_weights_host(w, p)
        rwe, rwd, rwa = M.model_weights(E, c["D"], c["A"], m, p)
        assert we == rwe and np.array_equal(wd, rwd) and np.array_equal(wa, rwa)
        assert as_u64(s).tolist() == M.drop_weights(E, c["D"], c["A"], m, p)


def run_search(ctx, name):
    c = nonvacuous(name)  # the conditions that keep the comparison from being vacuous, on the restatement
    m, p0 = c["m"], c["p0"]
    dX, dD, dA = ctx.to_dev(R.pack(c["X"])), ctx.to_dev(R.pack(c["D0"])), ctx.to_dev(R.pack(c["A0"]))
    dE = ctx.to_dev(np.full(R.pack(c["X"]).shape, 0x5555555555555555, np.uint64))  # E is formed by the call
    state = None if c["kind"] == M.BACKWARD else pybic.bsvd_rng_seed(I.RANDOM_SEED)
    p, length, trace, st, rc = ctx.bsvd_learn_mdl(c["kind"], dX, dE, m, dD, dA, p0, lmi=c["lmi"], du=0, mi=c["mi"],
                                                  state=state, status=True)
    assert (rc, p, length) == (c["rc"], c["p"], c["len"])
    assert trace == list(c["trace"])
    if state is not None:
        assert st == c["state"]
    assert np.array_equal(as_u64(dE), R.pack(c["E"])) and np.array_equal(as_u64(dX), R.pack(c["X"]))
    assert np.array_equal(as_u64(dD)[:p], R.pack(c["D"])[:p])
    assert np.array_equal(as_u64(dA)[:, :words(p)], R.pack(c["A"])[:, :words(p)])
    return c


@pytest.mark.parametrize("name", ["backward", "backward_alter1", "tiny"])
def test_backward_search(ctx, name):
    """planted 6 atoms from 12 (accepted and rejected passes, chosen atoms other than 0); the role-switching inner
    learner at 4,200 rows; and the input that ends in the empty model (E = X, the length keeps its value)"""
    run_search(ctx, name)


@pytest.mark.parametrize("name", ["forward_neighbor", "forward_partition"])
def test_forward_search(ctx, name):
    """from 2 atoms with room for 40: accepted passes, then ten rejected ones"""
    run_search(ctx, name)


def test_forward_search_out_of_room(ctx):
    """p_cap = 5: BIC_ENOSPC, the best model so far (5 atoms) in place"""
    assert run_search(ctx, "forward_nospc")["rc"] == pybic.BIC_ENOSPC


def test_full_search(ctx):
    """p = 40: two candidates, 22 initialisations and learns; the generator ends where the restatement's does"""
    run_search(ctx, "full")


def test_full_search_below_twenty_atoms(ctx):
    n, m, p = 30, 20, 19
    X = ctx.to_dev(np.zeros((n, 1), np.uint64))
    E, D, A = (ctx.to_dev(np.full(s, 7, np.uint64)) for s in ((n, 1), (p, 1), (n, 1)))
    st0 = pybic.bsvd_rng_seed(I.RANDOM_SEED)
    assert ctx.bsvd_learn_mdl(pybic.BSVD_MDL_FULL, X, E, m, D, A, p, mi=2, state=st0) == (0, 1 << 30, [], st0)
    assert all((as_u64(t) == 7).all() for t in (E, D, A))


def test_arguments(ctx):
    lib, h, C = ctx.lib, ctx.h, pybic.C
    X, E, D, A = ctx.empty_i64(4, 2), ctx.empty_i64(4, 2), ctx.empty_i64(7, 2), ctx.empty_i64(4, 1)
    w = ctx.empty_i64(16)
    p_ = lambda t: None if t is None else pybic._p(t)
    ctx._bind_stream()
    bad = pybic.BIC_EINVAL

    def weights(e, n, m, wpr, d, p, a, out=w):
        b = None if out is None else out.data_ptr()
        o = lambda off: None if b is None else C.c_void_p(b + off)
        return lib.bic_bsvd_model_weights(h, p_(e), n, m, wpr, p_(d), p, wpr, p_(a), 1, o(0), o(8), o(8 + 4 * p))

    assert weights(E, 4, 0, 2, D, 7, A) == bad and weights(E, 4, 1048577, 16385, D, 7, A) == bad     # m
    assert weights(E, 0, 100, 2, D, 7, A) == bad and weights(E, 1 << 31, 100, 2, D, 7, A) == bad     # n
    assert weights(E, 4, 100, 2, D, 4097, A) == bad and weights(E, 4, 100, 1, D, 7, A) == bad        # p, pitch
    assert weights(None, 4, 100, 2, D, 7, A) == bad and weights(E, 4, 100, 2, None, 7, A) == bad
    assert weights(E, 4, 100, 2, D, 7, A, out=None) == bad
    assert lib.bic_bsvd_drop_weights(h, p_(E), 4, 100, 2, p_(D), 0, 2, p_(A), 1, p_(w)) == bad       # p = 0
    assert lib.bic_bsvd_drop_atom(h, p_(D), 7, 100, 2, p_(A), 4, 1, 7) == bad                        # k = p
    assert lib.bic_bsvd_append_atom(h, p_(D), 4096, 100, 2, p_(A), 4, 65, p_(E), 2, p_(E), 2) == bad
    assert lib.bic_bsvd_append_atom(h, p_(D), 64, 100, 2, p_(A), 4, 1, p_(E), 2, p_(E), 2) == bad    # no word for it

    def learn(search, lmi, du, mi, n, m, p, p_cap, state=True, x=X):
        st, po, bl, nr = C.c_uint64(1), C.c_size_t(0), C.c_uint64(0), C.c_size_t(0)
        return lib.bic_bsvd_learn_mdl(h, search, lmi, du, mi, p_(x), 2, p_(E), n, m, 2, p_(D), p, p_cap, 2, p_(A), 1,
                                      C.byref(st) if state else None, C.byref(po), C.byref(bl), None, 0, C.byref(nr))

    for search in (0, 1, 2):
        assert learn(search, 4, 0, 0, 4, 100, 3, 7) == bad and learn(search, 0, 2, 0, 4, 100, 3, 7) == bad   # lmi, du
        assert learn(search, 0, 0, 0, 4, 100, 0, 7) == bad and learn(search, 0, 0, 0, 4, 100, 8, 7) == bad   # p
        assert learn(search, 0, 0, 0, 4, 100, 3, 65) == bad                                                  # a_wpr
        assert learn(search, 0, 0, 0, 4, 100, 3, 7, x=None) == bad
    assert learn(3, 0, 0, 0, 4, 100, 3, 7) == bad and learn(-1, 0, 0, 0, 4, 100, 3, 7) == bad
    for search in (0, 2):
        assert learn(search, 0, 0, 4, 4, 100, 3, 7) == bad                                                   # mi
        assert learn(search, 0, 0, 0, 4, 100, 3, 7, state=False) == bad
    ctx.sync()
