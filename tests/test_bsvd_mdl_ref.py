"""tests/bsvd_mdl_ref.py, the yardstick of the GPU tests of the MDL model-order searches, pinned (CPU only): literals
worked by hand for the code length and for each kept slip of bsvd.cpp:1438-1717, identities of the primitives on
planted data, and the cases the GPU tests compare on, with the conditions that keep those comparisons from being
vacuous. Every case here passes the restatement's guard: no truncated double within 1e-6 of an integer."""
import functools

import numpy as np
import pytest

import bsvd_init_ref as I
import bsvd_mdl_ref as M
import bsvd_ref as R
from bsvd_ref import words
from test_bsvd_prox_ref import bits

SEED = 4
PRIM_SHAPES = [(300, 64, 33), (4200, 100, 7), (70, 4200, 33), (257, 130, 70)]


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)


def mdl_start(seed, n, m, p_true, p_start, p_cap, noise=0.02, flips=0.05):
    """X from a planted model of p_true atoms; the start: its first min(p_true, p_start) atoms (with `flips` of
    their bits flipped), then random atoms at density 0.3 up to p_start, no coefficients. D and A are capacity
    arrays of p_cap atoms."""
    X, Dt, _, _ = R.planted(seed, n, m, p_true, noise=noise, flips=flips)
    rng = np.random.default_rng(seed + 1000)
    D = np.zeros((p_cap, X.shape[1]), np.uint8)
    k = min(p_true, p_start)
    D[:k] = Dt[:k]
    if p_start > p_true:
        D[p_true:p_start, :m] = rng.random((p_start - p_true, m)) < 0.3
    A = np.zeros((n, 64 * words(p_cap)), np.uint8)
    return X, D, A


def tiny_start():
    """40 x 20 of sparse noise with two atoms that explain nothing: the backward search ends in the empty model"""
    rng = np.random.default_rng(1)
    n, m = 40, 20
    X, D, A = np.zeros((n, 64), np.uint8), np.zeros((2, 64), np.uint8), np.zeros((n, 64), np.uint8)
    X[:, :m] = rng.random((n, m)) < 0.05
    D[:, :m] = rng.random((2, m)) < 0.4
    A[:, :2] = rng.random((n, 2)) < 0.1
    return X, D, A


# name -> (search, n, m, true atoms, start p, p_cap, lmi, mi, seed); the role-switching case starts from noisier
# data and atoms (noise 0.1, flips 0.3), where the inner learner changes the search's course
NOISY = {"backward_alter1": (0.1, 0.3)}
CASES = {
    "backward": (M.BACKWARD, 300, 64, 6, 12, 12, 0, 0, 4),
    "backward_alter1": (M.BACKWARD, 4200, 100, 5, 9, 9, 1, 0, 4),
    "forward_neighbor": (M.FORWARD, 300, 64, 6, 2, 40, 0, I.NEIGHBOR, 1),
    "forward_partition": (M.FORWARD, 300, 64, 6, 2, 40, 0, I.PARTITION, 1),
    "forward_nospc": (M.FORWARD, 300, 64, 6, 2, 5, 0, I.PARTITION, 1),
    "full": (M.FULL, 300, 64, 6, 40, 40, 0, I.CENTROIDS, 4),
}


@functools.lru_cache(maxsize=None)
def mdl_case(name):
    """a search of CASES (or "tiny") run by the restatement; computed once, never modified"""
    if name == "tiny":
        kind, m, p, lmi, mi = M.BACKWARD, 20, 2, 0, 0
        X, D0, A0 = tiny_start()
    else:
        kind, n, m, p_true, p, p_cap, lmi, mi, seed = CASES[name]
        X, D0, A0 = mdl_start(seed, n, m, p_true, p, p_cap, *NOISY.get(name, ()))
    E, D, A = np.zeros_like(X), D0.copy(), A0.copy()
    rng = I.Rand48()
    r = M.search(kind, X, E, D, A, m, p, lmi, 0, mi, rng)
    frozen(X, D0, A0, E, D, A)
    r.update(kind=kind, X=X, D0=D0, A0=A0, E=E, D=D, A=A, m=m, p0=p, lmi=lmi, mi=mi, state=rng.state,
             trace=tuple(r["trace"]), lines=tuple(r["lines"]))
    return r


def accepted(trace):
    """per pass but the last: whether it was accepted (the next record's stuck is 0 and its bestK moved)"""
    return [b[4] == 0 and b[2] != a[2] for a, b in zip(trace, trace[1:])]


def nonvacuous(name):
    c = mdl_case(name)
    tr = c["trace"]
    if name in ("backward", "backward_alter1"):
        acc = accepted(tr)
        assert any(acc) and not all(acc), name                       # accepted and rejected passes
        assert any(t[7] != 0 for t in tr), name                      # a chosen index other than 0
        assert 1 <= c["p"] < c["p0"] and c["rc"] == 0
    elif name == "tiny":
        assert c["p"] == 0 and c["lines"][-1] == "Resulted in empty model!" and np.array_equal(c["E"], c["X"])
        assert c["len"] == tr[-1][3]                                 # the length before the empty model
    elif name in ("forward_neighbor", "forward_partition"):
        assert any(accepted(tr)) and c["lines"][-1] == "No further improvement." and tr[-1][4] == 9
        assert c["p"] > c["p0"] and tr[-1][0] + 1 <= 40 and c["rc"] == 0
    elif name == "forward_nospc":
        assert c["rc"] == M.ENOSPC and c["p"] == 5 and tr[-1][0] == 5 and any(accepted(tr))
    else:
        assert len(tr) == 2 and [t[0] for t in tr] == [20, 40] and c["p"] in (20, 40)
        assert all(len(set(t[8])) > 1 for t in tr)                   # the ten repetitions differ
    return c


@pytest.mark.parametrize("name", sorted(CASES) + ["tiny"])
def test_cases_are_not_vacuous_and_pass_the_guard(name):
    c = nonvacuous(name)
    m, K = c["m"], c["p"]
    if K:  # the outputs are a model: E is its residual
        assert np.array_equal(c["E"], R.residual(c["X"], c["D"][:K], c["A"][:, :64 * words(K)], K))
        got = M.model_codelength(c["E"], c["D"], c["A"], m, K)
        if name == "full":  # the kept slip: the model is the last repetition's, the length the minimum's
            lens = next(t[8] for t in c["trace"] if t[0] == K)
            assert got == lens[-1] and c["len"] == min(lens) < got
        else:
            assert got == c["len"]


def test_inner_learner_matters():
    c = nonvacuous("backward_alter1")
    E, D, A = np.zeros_like(c["X"]), c["D0"].copy(), c["A0"].copy()
    r = M.backward(c["X"], E, D, A, c["m"], c["p0"], lmi=0)
    assert tuple(r["trace"]) != c["trace"] and (r["p"], r["len"]) != (c["p"], c["len"])


def test_full_search_draws_22_initialisations():
    """n draws per centroid initialisation (none rejected or a few), 11 initialisations per k"""
    c = mdl_case("full")
    rng = I.Rand48()
    rng.uniform(20, 300 * 11)
    rng.uniform(40, 300 * 11)
    assert rng.state == c["state"]


# ---- the code length, by hand ----------------------------------------------------------------------------------
def test_two_atom_model_by_hand():
    """n = m = 4. H(1/4) = 0.811278. E has 4 ones of 16: 16 H(1/4) + log2(16)/2 = 12.98 + 2 = 14.98 -> LE = 14.
    |D_0| = 1, |D_1| = 3: 4 H(1/4) + 1 = 4.245 each: LD = 4, then 4 + 4.245 = 8.245 -> 8. A's columns hold one
    user each: LA = 8 the same way. 14 + 8 + 8 = 30."""
    E = bits(["1000", "0100", "0010", "0001"])
    D = bits(["0100", "1110"])
    A = bits(["10", "01", "00", "00"])
    assert M.model_weights(E, D, A, 4, 2)[0] == 4
    assert M.model_codelength(E, D, A, 4, 2) == 30
    assert M.model_codelength(E, D, A, 4, 0) == 14           # p = 0: LE alone


def test_truncation_is_per_term():
    """n = m = 8, E = 0: LE = log2(64)/2 = 3. Two atoms of weight 1: 8 H(1/8) + 1.5 = 5.8485 each, so LD = 5, then
    5 + 5.8485 = 10.8485 -> 10, where truncating the sum 11.697 would give 11. LA the same: 3 + 10 + 10 = 23, not 25."""
    E = np.zeros((8, 64), np.uint8)
    D = bits(["10000000", "01000000"])
    A = np.zeros((8, 64), np.uint8)
    A[0, 0] = A[1, 1] = 1
    assert abs(M.universal_codelength(8, 1) - 5.8485) < 1e-4
    assert M.model_codelength(E, D, A, 8, 2) == 23
    assert int(2 * M.universal_codelength(8, 1)) == 11


def test_weights_ignore_padding_and_arguments_are_32_bit():
    E = bits(["1000", "0100", "0010", "0001"])
    D = bits(["0100", "1110"])
    A = bits(["10", "01", "00", "00"])
    E[:, 4:] = 1
    D[:, 4:] = 1
    A[:, 2:] = 1
    assert M.model_codelength(E, D, A, 4, 2) == 30
    assert M.universal_codelength((1 << 32) + 16, (1 << 32) + 4) == M.universal_codelength(16, 4)


def test_guard_refuses_a_double_next_to_an_integer():
    with pytest.raises(AssertionError):
        M.trunc(7.0000001)
    with pytest.raises(AssertionError):
        M.trunc(5.0)                                         # 4 H(1/2) + 1: an integer, but not the exempt case
    assert M.trunc(3.0, exact=True) == 3 and M.trunc(7.5) == 7
    assert M.exact_term(64, 0) and M.exact_term(64, 64) and not M.exact_term(100, 0) and not M.exact_term(64, 32)


# ---- the searches' control flow, by hand -----------------------------------------------------------------------
def run_backward(K, bestL, score_rows, next_lens):
    tr, lines, log = [], [], []
    rows, lens = iter(score_rows), iter(next_lens)
    out = M.backward_control(K, bestL, lambda k: next(rows), lambda k, a: next(lens), lambda k: log.append(("accept", k)),
                             lambda: log.append(("empty",)), tr, lines)
    return out, tr, lines, log


def test_backward_tie_goes_to_the_smaller_k():
    """scores 7, 5, 5: atom 1 (strict <); all scores above the start value 0xFFFFFFFFFFFFFF7F would leave atom 0"""
    (bestK, bestL), tr, lines, log = run_backward(3, 100, [[7, 5, 5], [M.START, M.START + 1], [9]], [90, 95, 200])
    assert [t[7] for t in tr] == [1, 0, 0]
    # 90 accepted (K = 2); 95 rejected (sum 5); the empty model at 200 rejected with dev = 5
    assert (bestK, bestL) == (2, 90) and log == [("accept", 2)]
    assert [(t[0], t[1], t[2], t[3], t[4], t[5], t[6]) for t in tr] == [
        (3, 100, 3, 100, 0, 0, 0), (2, 90, 2, 90, 0, 0, 0), (1, 95, 2, 90, 1, 5, 5)]
    assert lines[0] == "currK=3 currL=100 bestK=3 bestL=100 stuck=0 dif=0 dev=0"


def test_empty_model_branch():
    """K = 1 taken: the result has no atoms and the length keeps its previous value (the break precedes the
    assignment); not taken: the one-atom model stays"""
    (bestK, bestL), tr, lines, log = run_backward(1, 100, [[50]], [60])
    assert (bestK, bestL) == (0, 100) and log == [("empty",)] and lines[-1] == "Resulted in empty model!"
    (bestK, bestL), tr, lines, log = run_backward(1, 100, [[50]], [100])
    assert (bestK, bestL) == (1, 100) and log == [] and len(tr) == 1


def test_backward_stops_after_ten_rejections():
    (bestK, bestL), tr, lines, _ = run_backward(12, 100, [[1]] * 12, [101] * 12)
    assert (bestK, bestL) == (12, 100) and len(tr) == 10 and lines[-1] == "No further improvement."
    assert [t[6] for t in tr] == [0] + [1] * 9


def test_forward_sum_stuck_wraps():
    """bestL = 100. Pass 1 gives 104: rejected, sumStuck = 4. Pass 2 (dev = 4) gives 97: 97 + 4 = 101 is not below
    100, rejected although 97 < 100, and sumStuck += 97 - 100 in unsigned 64 bits: 4 + (2^64 - 3) wraps to 1.
    Pass 3: dev = 1 / 2 = 0, dif = int(97) - int(100) = -3; it gives 99: accepted with K = 5."""
    lens = iter([100, 104, 104, 97, 97, 99] + [99, 200] * 10)
    tr, lines, log = [], [], []
    bestK, bestL, rc = M.forward_control(2, 100, lambda: next(lens), lambda k: 0, lambda k: log.append(k), 40, tr, lines)
    assert [(t[0], t[4], t[5], t[6]) for t in tr[:4]] == [(2, 0, 0, 0), (3, 1, 4, 4), (4, 2, -3, 0), (5, 0, 0, 0)]
    assert log == [5] and (bestK, bestL, rc) == (5, 99, 0)
    # ten rejections of 200 follow: dev = (1 + 101 j) / (2 + j), and K grows every pass
    assert len(tr) == 13 and tr[-1][0] == 14 and tr[-1][4] == 9 and lines[-1] == "No further improvement."
    assert tr[5][6] == (1 + 101 * 2) // 4
    # a wrapped sum that stays huge: dev keeps its low 32 bits as an int
    s = M._Stuck()
    s.reject(90, 100)
    assert s.sum == (1 << 64) - 10 and s.dev() == M.c_int((1 << 64) - 10) == -10
    assert M.better(105, -10, 100) and not M.better(110, -10, 100)


def test_forward_stops_at_capacity():
    lens = iter([100, 90, 90, 80, 80])
    tr, lines, log = [], [], []
    assert M.forward_control(2, 100, lambda: next(lens), lambda k: 0, log.append, 4, tr, lines) == (4, 80, M.ENOSPC)
    assert log == [3, 4] and [t[0] for t in tr] == [2, 3, 4]


def test_full_search_below_twenty_atoms():
    X, D, A = mdl_start(SEED, 30, 20, 3, 19, 19)
    E = np.full_like(X, 1)
    D0, A0 = D.copy(), A.copy()
    rng = I.Rand48()
    r = M.full_search(X, E, D, A, 20, 19, mi=I.CENTROIDS, rng=rng)
    assert (r["p"], r["len"], r["trace"], r["lines"]) == (0, 1 << 30, [], ["bestL=1073741824 bestk=0"])
    assert E.all() and np.array_equal(D, D0) and np.array_equal(A, A0) and rng.outputs == 0


def test_full_search_keeps_the_last_repetition():
    """ten lengths whose minimum is not the last: candL is the minimum, the model copied out the last one's"""
    tr, lines, log = [], [], []
    reps = {20: [9, 8, 7, 6, 5, 6, 7, 8, 9, 10], 40: [9] * 10}
    assert M.full_control(45, lambda k: reps[k], log.append, tr, lines) == (20, 5)
    assert log == [20] and tr[0][:4] == (20, 5, 20, 5) and tr[1][:4] == (40, 9, 20, 5)
    assert lines == ["K=20 9 8 7 6 5 6 7 8 9 10 5", "K=40 " + "9 " * 10 + "9", "bestL=5 bestk=20"]


# ---- the primitives on planted data ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def prim_case(n, m, p):
    """a planted model after one sparse-coding step, with dirty padding in E, D and A; weights and scores"""
    X, D, A, E = (a.copy() for a in R.planted(SEED, n, m, p, a_flips=0.02))
    R.update_coefficients_argmin(E, D, A, p)
    rng = np.random.default_rng(7)
    E[:, m:] = rng.random(E[:, m:].shape) < 0.5
    D[:, m:] = rng.random(D[:, m:].shape) < 0.5
    A[:, p:] = rng.random(A[:, p:].shape) < 0.5
    if p >= 3:
        A[:, 1] = 0                                          # an unused atom
        A[:, 2] = 1                                          # an atom every row uses
    frozen(E, D, A)
    return dict(E=E, D=D, A=A, weights=M.model_weights(E, D, A, m, p), drop=M.drop_weights(E, D, A, m, p))


@pytest.mark.parametrize("n,m,p", PRIM_SHAPES)
def test_drop_weights_is_the_weight_without_the_atom(n, m, p):
    c = prim_case(n, m, p)
    E, D, A = c["E"], c["D"], c["A"]
    for k in range(p):
        assert c["drop"][k] == int((E ^ np.outer(A[:, k], D[k]))[:, :m].sum()), k
    we, wd, wa = c["weights"]
    assert c["drop"][1] == we and wa[1] == 0 and wa[2] == n


@pytest.mark.parametrize("p", [63, 64, 70])
def test_append_then_drop_is_the_identity(p):
    n, m = 50, 100
    rng = np.random.default_rng(p)
    D = np.zeros((p + 1, 128), np.uint8)
    A = np.zeros((n, 64 * words(p + 1)), np.uint8)
    D[:p, :m] = rng.random((p, m)) < 0.3
    A[:, :p] = rng.random((n, p)) < 0.3
    D0, A0 = D.copy(), A.copy()
    atom, coefs = np.ones(128, np.uint8), (rng.random(n) < 0.5).astype(np.uint8)
    M.append_atom(D, A, m, p, atom, coefs)
    assert D[p, :m].all() and not D[p, m:].any() and np.array_equal(A[:, p], coefs) and not A[:, p + 1:].any()
    M.drop_atom(D, A, p + 1, p)
    assert np.array_equal(D[:p], D0[:p]) and np.array_equal(A, A0)
    # dropping an inner atom moves the later ones up
    M.drop_atom(D, A, p, 3)
    assert np.array_equal(D[:p - 1], np.delete(D0[:p], 3, axis=0)) and np.array_equal(A[:, :p - 1], np.delete(A0[:, :p], 3, 1))
    assert not A[:, p - 1:].any()
