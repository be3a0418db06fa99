"""Python restatement of the reference's MDL model-order searches, bsvd.cpp:1438-1717 (model_codelength,
learn_model_mdl_forward_selection, _backward_selection, _full_search), over the learners of tests/bsvd_alter_ref.py
and the initialisers of tests/bsvd_init_ref.py, on their unpacked whole-word arrays (test infrastructure: the
yardstick of tests/test_gpu_bsvd_mdl.py and tests/test_gpu_bsvd_mdl_host.py, pinned by tests/test_bsvd_mdl_ref.py;
bsvd.cpp itself cannot be built here, it needs GSL).

The arithmetic follows the text: idx_t is an unsigned 64-bit integer, universal_codelength takes two 32-bit
unsigned arguments and returns a double (math.log2: the C library's log2, as the build under test calls it),
`idx_t += double` converts the running sum to double, adds, and truncates toward zero, `int dev = idx_t`
keeps the low 32 bits as a signed number, and `idx_t + int` sign-extends the int.

Every double that gets truncated goes through trunc(), which asserts that it does not lie within GUARD of an
integer, so that a last-bit difference between two log2 implementations cannot change a result. One case is let
through: a value that IS an integer and whose last term was 0.5 log2(n) for n a power of two (an atom or a column
of weight 0 or n in a row of 4, 16, 64, .. bits), where log2 is exact and so is the sum.

A model lives in capacity arrays: D [p_cap, 64 ceil(m/64)], A [n, 64 ceil(p_cap/64)], of which the first K rows and
the first 64 ceil(K/64) columns are the current model's. The searches work in place on E, D and A and return
a dict: p (the result's atoms), len (the reference's return value), trace (one tuple per pass, in the layout of
pybic.MdlStep.astuple(): K, currL, bestK, bestL, stuck, dif, dev, atom, the ten lengths), rc (0, or what
bic_bsvd_learn_mdl returns where the reference has no answer: ENOSPC, EINVAL) and lines (the reference's stdout).
"""
import math

import numpy as np

import bsvd_alter_ref as L
import bsvd_init_ref as I
from bsvd_ref import words

GUARD = 1e-6
MASK = (1 << 64) - 1
START = 0xFFFFFFFFFFFFFF7F          # ~(1UL << (sizeof(idx_t) - 1)), bsvd.cpp:1576
FULL_START = 1 << 30                # bsvd.cpp:1674
OK, EINVAL, ENOSPC = 0, 1, 4        # include/bic.h
FORWARD, BACKWARD, FULL = 0, 1, 2   # include/bic.h BIC_BSVD_MDL_*
NOLENS = (0,) * 10


def c_int(v):
    """conversion to a 32-bit int: the low 32 bits, two's complement"""
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= 1 << 31 else v


def universal_codelength(n, r):
    """coding.cpp:24-32 with its unsigned arguments"""
    n &= 0xFFFFFFFF
    r &= 0xFFFFFFFF
    half_log = 0.5 * math.log2(n)
    if r == 0 or r >= n:
        return half_log
    p = r / n
    return float(n) * (-p * math.log2(p) - (1.0 - p) * math.log2(1.0 - p)) + half_log


def exact_term(n, r):
    n &= 0xFFFFFFFF
    r &= 0xFFFFFFFF
    return (r == 0 or r >= n) and n & (n - 1) == 0


def trunc(x, exact=False):
    """double -> idx_t, guarded (see the module's head)"""
    assert x >= 0.0, x
    f = x - math.floor(x)
    if not (exact and f == 0.0):
        assert GUARD < f < 1.0 - GUARD, f"{x!r} is within {GUARD} of an integer"
    return int(x)


def plus(s, n, r):
    """idx_t s += universal_codelength(n, r)"""
    return trunc(float(s) + universal_codelength(n, r), exact_term(n, r))


def minus(s, n, r):
    """idx_t s -= universal_codelength(n, r)"""
    return trunc(float(s) - universal_codelength(n, r), exact_term(n, r))


def length_e(n, m, we):
    """bsvd.cpp:1450: rows * cols and the weight truncated to unsigned"""
    return trunc(universal_codelength(n * m, we), exact_term(n * m, we))


def model_weights(E, D, A, m, p):
    """|E|, |D_k| and |A_k| for k < p, every read masked at the row's last word (get_block, binmat.h:188-190)"""
    return (int(E[:, :m].sum(dtype=np.int64)), D[:p, :m].sum(axis=1, dtype=np.int64).astype(np.uint32),
            A[:, :p].sum(axis=0, dtype=np.int64).astype(np.uint32))


def codelength_sums(n, m, wd, wa):
    LD = LA = 0                                            # :1451
    for k in range(len(wd)):                               # :1452
        LD = plus(LD, m, int(wd[k]))                       # :1455
        LA = plus(LA, n, int(wa[k]))                       # :1456
    return LD, LA


def codelength_from_weights(n, m, we, wd, wa):
    LD, LA = codelength_sums(n, m, wd, wa)
    return (length_e(n, m, we) + LD + LA) & MASK           # :1460


def model_codelength(E, D, A, m, p):
    """bsvd.cpp:1438-1461"""
    return codelength_from_weights(E.shape[0], m, *model_weights(E, D, A, m, p))


def drop_weights(E, D, A, m, p):
    """for every k < p the masked weight of E ^ (A_k^t D_k) (mul(Ak, true, Dk, false, AkDk); add(AkDk, E, nextE),
    :1580-1582), as the weight of E plus what the users of atom k gain or lose"""
    Em = E[:, :m]
    we = int(Em.sum(dtype=np.int64))
    out = []
    for k in range(p):
        users = A[:, k] == 1
        out.append(we + int((Em[users] ^ D[k, :m]).sum(dtype=np.int64)) - int(Em[users].sum(dtype=np.int64)))
    return out


def drop_atom(D, A, p, k):
    """row k of D and column k of A out, in place (:1594-1610); column p - 1 and A's padding inside ceil(p/64) words
    become 0 (this build's decision: the reference allocates without clearing)"""
    D[k:p - 1] = D[k + 1:p].copy()
    A[:, k:p - 1] = A[:, k + 1:p].copy()
    A[:, p - 1:64 * words(p)] = 0


def append_atom(D, A, m, p, atom, coefs):
    """atom as row p of D, coefs as column p of A (:1497-1513), the new row's and A's padding zero"""
    D[p] = 0
    D[p, :m] = atom[:m]
    A[:, p] = coefs
    A[:, p + 1:64 * words(p + 1)] = 0


def view(D, A, K):
    """the model of K atoms inside its capacity arrays"""
    return D[:K], A[:, :64 * words(K)]


def header(K, currL, bestK, bestL, stuck, dif, dev):
    return f"currK={K} currL={currL} bestK={bestK} bestL={bestL} stuck={stuck} dif={dif} dev={dev}"


class _Stuck:
    def __init__(self):
        self.stuck = self.sum = self.all = 0

    def dev(self):
        return c_int(self.sum // self.all) if self.all > 0 else 0  # :1486 (unsigned division, then int)

    def reject(self, length, best):
        self.stuck += 1
        self.all += 1
        self.sum = (self.sum + length - best) & MASK       # :1531


def better(length, dev, best):
    return (length + dev) & MASK < best                    # :1517: the int is sign-extended


def forward_control(K, bestL, measure, grow, accept, p_cap, trace, lines):
    """the loop of :1480-1538. measure() -> the current model's length; grow(K) -> 0 after it initialised one atom,
    appended it and learned, or an error code; accept(K) when the current model of K atoms becomes the best."""
    bestK, st = K, _Stuck()
    while True:
        currL = measure()                                  # :1484
        dif, dev = c_int(currL - bestL), st.dev()          # :1485-1486
        trace.append((K, currL, bestK, bestL, st.stuck, dif, dev, 0, NOLENS))
        lines.append(header(K, currL, bestK, bestL, st.stuck, dif, dev))
        if K + 1 > p_cap:
            return bestK, bestL, ENOSPC
        rc = grow(K)                                       # :1488-1515
        if rc:
            return bestK, bestL, rc
        currL = measure()                                  # :1516
        if better(currL, dev, bestL):                      # :1517
            st.stuck = 0
            bestL = currL
            accept(K + 1)
            bestK = K + 1
        else:
            st.reject(currL, bestL)
            if st.stuck >= 10:                             # :1532
                lines.append("No further improvement.")
                break
        K += 1                                             # :1537
    return bestK, bestL, OK


def backward_control(K, bestL, scores, shrink, accept, empty, trace, lines):
    """the loop of :1571-1654. scores(K) -> the K values tmpL; shrink(K, k) -> the length of the model without atom
    k after learning (K = 1: of the empty model); accept(K) / empty() copy the result out."""
    bestK, currL, st = K, bestL, _Stuck()
    while K > 0:
        dif, dev = c_int(currL - bestL), st.dev()          # :1572-1573
        nextk, nextL = 0, START                            # :1575-1576
        for k, tmpL in enumerate(scores(K)):
            if tmpL < nextL:                               # :1586 strict: the smallest k among equals
                nextL, nextk = tmpL, k
        trace.append((K, currL, bestK, bestL, st.stuck, dif, dev, nextk, NOLENS))
        lines.append(header(K, currL, bestK, bestL, st.stuck, dif, dev))
        nextL = shrink(K, nextk)                           # :1596-1615
        if better(nextL, dev, bestL):                      # :1617
            if K == 1:                                     # :1619-1625: the break precedes bestL = nextL
                lines.append("Resulted in empty model!")
                empty()
                return 0, bestL
            st.stuck = 0
            bestK, bestL = K - 1, nextL
            accept(K - 1)
        else:
            st.reject(nextL, bestL)
            if st.stuck >= 10:
                lines.append("No further improvement.")
                break
        currL = nextL                                      # :1653
        K -= 1
    return bestK, bestL


def full_control(p, lengths, accept, trace, lines):
    """the loop of :1676-1713. lengths(k) -> the ten lengths of k (after the run that is thrown away); accept(k)
    copies the LAST repetition's model out."""
    bestL, bestk = FULL_START, 0
    for k in range(20, p + 1, 20):
        aux = tuple(lengths(k))
        candL = min(aux)                                   # :1692
        lines.append(f"K={k} " + " ".join(str(a) for a in aux) + f" {candL}")
        if candL < bestL:                                  # :1698
            bestL, bestk = candL, k
            accept(k)
        trace.append((k, candL, bestk, bestL, 0, 0, 0, 0, aux))
    lines.append(f"bestL={bestL} bestk={bestk}")
    return bestk, bestL


class _Work:
    """the working copies of a search and what the three share"""

    def __init__(self, X, E, D, A, m, lmi, du, mi, rng):
        self.X, self.E, self.D, self.A, self.m, self.n = X, E, D, A, m, X.shape[0]
        self.lmi, self.du, self.mi, self.rng = lmi, du, mi, rng
        self.cE, self.cD, self.cA = E.copy(), D.copy(), A.copy()

    def learn(self, E, D, A, K):
        d, a = view(D, A, K)
        L.learn(self.lmi, self.X, E, d, a, self.m, K, self.du)

    def length(self, E, D, A, K):
        return model_codelength(E, D, A, self.m, K)

    def accept(self, K):
        self.E[:] = self.cE
        self.D[:K] = self.cD[:K]
        self.A[:, :64 * words(K)] = self.cA[:, :64 * words(K)]


def forward(X, E, D, A, m, p, lmi=0, du=0, mi=0, rng=None):
    """bsvd.cpp:1463-1546; p_cap = D's rows"""
    w = _Work(X, E, D, A, m, lmi, du, mi, rng)
    w.learn(E, D, A, p)                                    # :1470
    w.cE, w.cD, w.cA = E.copy(), D.copy(), A.copy()        # :1473
    trace, lines = [], []

    def grow(K):
        if mi == I.NEIGHBOR and not w.cE[:, :m].any():     # (bic_bsvd_initialize: the reference would not return)
            return EINVAL
        d1, a1 = I.initialize(mi, w.cE, m, 1, rng)         # :1488
        append_atom(w.cD, w.cA, m, K, d1[0], a1[:, 0])     # :1497-1513
        w.learn(w.cE, w.cD, w.cA, K + 1)                   # :1515
        return OK

    K = {"K": p}

    def measure():
        return w.length(w.cE, w.cD, w.cA, K["K"])

    def grow_counted(k):
        rc = grow(k)
        if not rc:
            K["K"] = k + 1
        return rc

    bestK, bestL, rc = forward_control(p, w.length(E, D, A, p), measure, grow_counted, w.accept, D.shape[0], trace,
                                       lines)
    return dict(p=bestK, len=bestL, trace=trace, rc=rc, lines=lines)


def backward(X, E, D, A, m, p, lmi=0, du=0):
    """bsvd.cpp:1548-1663"""
    w = _Work(X, E, D, A, m, lmi, du, 0, None)
    n = w.n
    w.learn(E, D, A, p)                                    # :1555
    w.cD, w.cA = D.copy(), A.copy()                        # :1563-1564
    trace, lines, kept = [], [], {}

    def scores(K):
        we, wd, wa = model_weights(E, w.cD, w.cA, m, K)
        LD, LA = codelength_sums(n, m, wd, wa)
        dw = drop_weights(E, w.cD, w.cA, m, K)             # the caller-visible E, the current D and A
        kept["first"] = dw[0]
        out = []
        for k in range(K):
            tmpL = (length_e(n, m, dw[k]) + LD + LA) & MASK  # :1583
            tmpL = minus(tmpL, m, int(wd[k]))              # :1584
            tmpL = minus(tmpL, n, int(wa[k]))              # :1585
            out.append(tmpL)
        return out

    def shrink(K, k):
        if K == 1:
            return length_e(n, m, kept["first"])           # :1614 nextE as the k = 0 score left it, no atoms
        drop_atom(w.cD, w.cA, K, k)                        # :1597-1610
        w.learn(w.cE, w.cD, w.cA, K - 1)                   # :1611
        return w.length(w.cE, w.cD, w.cA, K - 1)           # :1612

    def empty():
        E[:] = X                                           # :1623

    bestK, bestL = backward_control(p, w.length(E, D, A, p), scores, shrink, w.accept, empty, trace, lines)
    return dict(p=bestK, len=bestL, trace=trace, rc=OK, lines=lines)


def full_search(X, E, D, A, m, p, lmi=0, du=0, mi=0, rng=None):
    """bsvd.cpp:1665-1717"""
    w = _Work(X, E, D, A, m, lmi, du, mi, rng)
    trace, lines = [], []

    def one(k):
        d, a = I.initialize(mi, X, m, k, rng)              # :1679 / :1687
        w.cD[:k], w.cA[:, :64 * words(k)] = d, a
        w.learn(w.cE, w.cD, w.cA, k)                       # :1680 / :1688

    def lengths(k):
        one(k)                                             # thrown away, its draws used up
        out = []
        for _ in range(10):                                # :1685
            one(k)
            out.append(w.length(w.cE, w.cD, w.cA, k))      # :1689
        return out

    bestk, bestL = full_control(p, lengths, w.accept, trace, lines)
    return dict(p=bestk, len=bestL, trace=trace, rc=OK, lines=lines)


def search(kind, X, E, D, A, m, p, lmi=0, du=0, mi=0, rng=None):
    if kind == FORWARD:
        return forward(X, E, D, A, m, p, lmi, du, mi, rng)
    if kind == BACKWARD:
        return backward(X, E, D, A, m, p, lmi, du)
    return full_search(X, E, D, A, m, p, lmi, du, mi, rng)
