"""Numpy restatement of the reference's model initialisers and of the generator they draw from (test
infrastructure: the yardstick of tests/test_gpu_bsvd_init.py, pinned by tests/test_bsvd_init_ref.py; bsvd.cpp
itself cannot be built here, it needs GSL).

Matrices are unpacked 0/1 uint8 arrays over the WHOLE words of a row, as in tests/bsvd_ref.py: E [n, 64 ceil(m/64)]
in, D [p, 64 ceil(m/64)] and A [n, 64 ceil(p/64)] out. Unlike the steps, every read of E here is masked at the
trailing word (get(i, j) with j < m; weight, bool_and and add through get_block, binmat.h:188-190), so only
E[:, :m] is looked at, and D and A come back with zero padding (A.clear(), D.clear(), then set(k, j) with j < m).

  initialize_neighbor    bsvd.cpp:227-267 initialize_model_neighbor
  initialize_partition   bsvd.cpp:173-219 initialize_model_partition (binmat.cpp:80-92 col_weight, util.cpp:7-51)
  initialize_centroids   bsvd.cpp:128-166 initialize_model_random_centroids, :99-126 _xor
  Rand48                 gsl_rng_rand48 with gsl_rng_set, gsl_rng_get and gsl_rng_uniform_int

Each initialiser takes either what the reference draws (picks, assignments: then nothing is drawn, and an index
out of range or a zero pick does what include/bic.h documents for the explicit entries) or a Rand48, which it
advances as the reference advances its process-wide generator. stats (a dict, optional) receives what the tests
want to have seen.
"""
import numpy as np

from bsvd_ref import words

RANDOM_SEED = 34503498  # bsvd.cpp:23
NEIGHBOR, PARTITION, CENTROIDS, CENTROIDS_XOR = 0, 1, 2, 3  # include/bic.h BIC_BSVD_MI_*


class Rand48:
    """gsl_rng_rand48 (the Unix rand48 sequence): a 48-bit state, 32-bit outputs"""

    def __init__(self, seed=RANDOM_SEED, state=None):
        if state is not None:
            self.state = state
        else:                                              # rand48_set: the low 32 bits of the seed
            s = seed & 0xFFFFFFFF
            self.state = (s << 16) | 0x330E if s else 0x1234ABCD330E
        self.outputs = 0                                   # how many outputs were taken, rejected ones included

    def get(self):                                         # rand48_advance, rand48_get
        self.state = (0x5DEECE66D * self.state + 0xB) & ((1 << 48) - 1)
        self.outputs += 1
        return self.state >> 16

    def uniform_int(self, bound):                          # gsl_rng_uniform_int (rng/rng.c)
        scale = 0xFFFFFFFF // bound                        # range = max - min = 0xffffffff
        while True:
            k = self.get() // scale
            if k < bound:
                return k

    def uniform(self, bound, count):
        return np.array([self.uniform_int(bound) for _ in range(count)], np.uint32)


def initialize_neighbor(E, m, p, picks=None, rng=None, stats=None):
    """bsvd.cpp:227-267 -> D, A"""
    n = E.shape[0]
    D = np.zeros((p, E.shape[1]), np.uint8)                # :238 D.clear()
    A = np.zeros((n, 64 * words(p)), np.uint8)             # :237 A.clear()
    st = {"redraws": 0, "u1": 0, "ties": 0, "max_u": 0, "picks": []}
    Em = E[:, :m]
    k = 0
    while k < p:                                           # :239
        if picks is None:
            i = rng.uniform_int(n)                         # :241
            if not Em[i].any():                            # :243 a zero row: drawn again, the draw is used up
                st["redraws"] += 1
                continue
        else:
            i = int(picks[k])
            if i >= n or not Em[i].any():                  # (bic.h: skipped / a zero pick, the atom stays zero)
                st["picks"].append(i)
                k += 1
                continue
        st["picks"].append(i)
        Ei = Em[i]                                         # :242
        both = Em & Ei                                     # :248-249 bool_and(Ej, Ei, Ej)
        near = both.any(axis=1)                            # :250 weight > 0
        u = int(near.sum())                                # :251
        s = both[near].sum(axis=0, dtype=np.int64)         # :252-255
        # :258 u > 0 always: the pick meets itself
        D[k, :m] = s >= u // 2                             # :259-260
        st["u1"] += u == 1
        st["ties"] += int(((s == u // 2) & (Ei == 1)).sum()) if u >= 2 else 0
        st["max_u"] = max(st["max_u"], u)
        k += 1                                             # :261
    if stats is not None:
        stats.update(st)
    return D, A


def col_weight(E, m, c):
    """binmat.cpp:80-92 as written: pd = &data[c / 64]; for (i = 0; i < rows; i += blocks_per_row) pd[i] & mask.
    Word c / 64 + i of the matrix is word c / 64 of row i / blocks_per_row (i is a multiple of blocks_per_row)."""
    n, mw = E.shape[0], words(m)
    w = 0
    for i in range(0, n, mw):                              # :87
        if E[i // mw, c]:                                  # :88
            w += 1
    return w


def counting_sort(s):
    """util.cpp:7-51 on a list of (first, second) pairs, in place"""
    n = len(s)
    maxs = max([f for f, _ in s] + [0])                    # :8-15
    count = [0] * (maxs + 2)                               # :17-19
    scratch = [None] * n
    for i in range(n):                                     # :23-25
        count[s[i][0] + 1] += 1
    for i in range(1, maxs + 2):                           # :29-30
        count[i] += count[i - 1]
    for i in range(n - 1, -1, -1):                         # :34-43 (from the end: equal weights come out reversed)
        c = s[i][0]
        scratch[count[c]] = s[i]
        count[c] += 1
    s[:] = scratch                                         # :45-46


def initialize_partition(E, m, p, stats=None):
    """bsvd.cpp:173-219 -> D, A"""
    n = E.shape[0]
    D = np.zeros((p, E.shape[1]), np.uint8)                # :188
    A = np.zeros((n, 64 * words(p)), np.uint8)             # :187
    Em = E[:, :m]
    ranking = [(col_weight(E, m, k), k) for k in range(m)]  # :191-194
    full = Em.sum(axis=0, dtype=np.int64)
    weights = [w for w, _ in ranking]
    st = {"sampled_differs": int(sum(w != f for w, f in zip(weights, full))),
          "rank_ties": len(weights) - len(set(weights)), "small_pivots": 0, "zero_pivots": 0, "pivots": []}
    counting_sort(ranking)                                 # :195
    for k in range(min(p, m)):                             # :198
        pivot = ranking[m - k - 1][1]                      # :201
        members = Em[:, pivot] == 1                        # :204 over all n rows
        u = int(members.sum())                             # :205
        s = Em[members].sum(axis=0, dtype=np.int64)        # :206-210
        D[k, :m] = s >= u // 2                             # :213-214
        st["small_pivots"] += u <= 1
        st["zero_pivots"] += u == 0
        st["pivots"].append(pivot)
    if stats is not None:
        stats.update(st)
    return D, A


def initialize_centroids(E, m, p, assign=None, rng=None, xor=False, stats=None):
    """bsvd.cpp:128-166 (xor: :99-126) -> D, A"""
    n = E.shape[0]
    D = np.zeros((p, E.shape[1]), np.uint8)                # :144 / :115
    A = np.zeros((n, 64 * words(p)), np.uint8)             # :143 / :114
    Em = E[:, :m]
    s = np.zeros((p, m), np.int64)                         # :145-148
    u = np.zeros(p, np.int64)
    ks = []
    for i in range(n):                                     # :150 / :116
        k = rng.uniform_int(p) if assign is None else int(assign[i])  # :151 / :117
        ks.append(k)
        if k >= p:                                         # (bic.h: skipped, the row joins no atom)
            continue
        A[i, k] = 1                                        # :152 / :118
        u[k] += 1                                          # :153
        if xor:
            D[k, :m] ^= Em[i]                              # :119-122 add(Dk, Ei, Dk)
        else:
            s[k] += Em[i]                                  # :155-156
    if not xor:
        D[:, :m] = 2 * s >= u[:, None]                     # :159-163
    st = {"empty": int((u == 0).sum()), "ties": int(((2 * s == u[:, None]) & (u[:, None] > 0)).sum()),
          "max_u": int(u.max()), "assign": np.array(ks, np.uint32)}
    if stats is not None:
        stats.update(st)
    return D, A


def initialize(mi, E, m, p, rng, stats=None):
    """the rule mi from the generator rng, as bic_bsvd_initialize"""
    if mi == NEIGHBOR:
        return initialize_neighbor(E, m, p, rng=rng, stats=stats)
    if mi == PARTITION:
        return initialize_partition(E, m, p, stats=stats)
    return initialize_centroids(E, m, p, rng=rng, xor=mi == CENTROIDS_XOR, stats=stats)


def clustered(seed, n, m):
    """The input the tests and tools/time_bsvd_init.py run on (dense random data leaves the neighbour atoms almost
    empty): the columns are split among c = max(2, min(8, m / 16)) clusters, a row takes one cluster's columns
    with probability 0.8 each, 0.2 % of all bits are flipped, every 17th row is zero, and, from 20 rows and 16
    columns on, rows 1, 2, 3 hold one column each that no other row has. E's padding bits are all ones.
    -> E (unpacked whole words), the three lonely rows (or [])"""
    rng = np.random.default_rng(seed)
    M = 64 * words(m)
    c = max(2, min(8, m // 16))
    cluster_of_col = np.arange(m) * c // m
    cluster_of_row = rng.integers(0, c, n)
    E = np.zeros((n, M), np.uint8)
    E[:, :m] = (cluster_of_col[None, :] == cluster_of_row[:, None]) & (rng.random((n, m)) < 0.8)
    E[:, :m] ^= rng.random((n, m)) < 0.002
    E[16::17, :m] = 0
    lonely = []
    if n >= 20 and m >= 16:
        lonely = [1, 2, 3]
        for r, col in zip(lonely, (0, m // 2, m - 1)):
            E[:, col] = 0
            E[r, :m] = 0
            E[r, col] = 1
    if not E[:, :m].any():
        E[0, 0] = 1
    E[:, m:] = 1
    return E, lonely
