"""Bit-serial numpy restatement of the reference's binary dictionary learning steps (test infrastructure:
the yardstick of tests/test_gpu_bsvd.py, pinned by tests/test_bsvd_ref.py; bsvd.cpp itself cannot be
built here, it needs GSL).

Matrices are unpacked 0/1 uint8 arrays over the WHOLE words of a row: E, X [n, 64 ceil(m/64)],
D [p, 64 ceil(m/64)], A [n, 64 ceil(p/64)]. dist, weight and add run over whole words in the reference
(binmat.cpp:57-67, 463-512), so a row here carries its padding bits and they take part; get/set/flip
address single bits j < m (k < p), so the padding of D and A never changes. All three functions work
in place and return what the reference returns.

  update_coefficients   bsvd.cpp:399-460 update_coefficients_basic (:1029-1107 _omp gives the same)
  update_dictionary     bsvd.cpp:463-527 update_dictionary_steepest
  learn                 bsvd.cpp:1215-1244 learn_model_traditional
"""
import numpy as np


def words(m):
    return (m + 63) // 64


def unpack(W, nwords=None):
    """uint64 words [rows, wpr] (column j at bit 63 - j % 64 of word j / 64) -> 0/1 uint8 [rows, 64 nwords]"""
    W = np.ascontiguousarray(W, np.uint64)
    nwords = W.shape[1] if nwords is None else nwords
    be = W[:, :nwords].astype(">u8").view(np.uint8).reshape(W.shape[0], -1)
    return np.unpackbits(be, axis=1)


def pack(B):
    """0/1 uint8 [rows, 64 w] -> uint64 words [rows, w]"""
    B = np.ascontiguousarray(B, np.uint8)
    return np.packbits(B, axis=1).view(">u8").astype(np.uint64).reshape(B.shape[0], -1)


def update_coefficients(E, D, A, p, stats=None):
    """bsvd.cpp:399-460. stats (a dict, optional) counts what the tests want to have seen: rows with more
    than one step, ties at the minimum, coefficients switched off."""
    n = E.shape[0]
    changed = 0                                            # :410
    st = {"multi": 0, "ties": 0, "off": 0, "steps": 0}
    for i in range(n):                                     # :414
        Ei = E[i].copy()                                   # :415
        Ai = A[i].copy()                                   # :416
        improved, ichanged, steps = True, False, 0         # :417-419
        while improved:                                    # :420
            w = int(Ei.sum())                              # :421 weight over whole words
            bestk, bestd = 0, int((Ei ^ D[0]).sum())       # :422-423
            tie = False
            for k in range(1, p):                          # :427
                dk = int((Ei ^ D[k]).sum())                # :429 dist over whole words
                if dk < bestd:                             # :433 strict: the first k among equals stays
                    bestd, bestk, tie = dk, k, False
                elif dk == bestd:
                    tie = True
            if bestd < w:                                  # :439
                st["off"] += int(Ai[bestk])
                Ai[bestk] ^= 1                             # :441 flip
                Ei ^= D[bestk]                             # :442
                ichanged = True                            # :444
                steps += 1
                st["ties"] += tie
            else:
                improved = False                           # :446
        if ichanged:                                       # :450
            changed += 1
            E[i] = Ei                                      # :452
            A[i] = Ai                                      # :453
        st["multi"] += steps > 1
        st["steps"] += steps
    if stats is not None:
        stats.update(st)
    return changed                                         # :459


def update_coefficients_argmin(E, D, A, p, stats=None):
    """update_coefficients with the scan over k as one numpy reduction (argmin returns the first minimum,
    the strict < of :433): the same function, for the shapes where the loop over k takes seconds (it is not
    the reference's update_coefficients_fast, which is broken and out of scope). tests/test_bsvd_ref.py holds
    the two equal on the planted shapes and on the shapes whose atoms the device streams in tiles."""
    n = E.shape[0]
    changed = 0
    st = {"multi": 0, "ties": 0, "off": 0, "steps": 0}
    Dp = D[:p].astype(np.int32)
    dw = Dp.sum(axis=1)
    for i in range(n):
        Ei, Ai, steps = E[i].copy(), A[i].copy(), 0
        while True:
            w = int(Ei.sum())
            d = w + dw - 2 * (Dp @ Ei.astype(np.int32))    # |e ^ d| = |e| + |d| - 2 |e & d|
            bestk = int(np.argmin(d))
            if not d[bestk] < w:
                break
            st["ties"] += int((d == d[bestk]).sum() > 1)
            st["off"] += int(Ai[bestk])
            Ai[bestk] ^= 1
            Ei ^= D[bestk]
            steps += 1
        if steps:
            changed += 1
            E[i], A[i] = Ei, Ai
        st["multi"] += steps > 1
        st["steps"] += steps
    if stats is not None:
        stats.update(st)
    return changed


def update_dictionary(E, D, A, m, p, stats=None):
    """bsvd.cpp:463-527, the atoms in order. stats (a dict, optional): the largest usage and column count."""
    changed = 0                                            # :480
    st = {"max_usage": 0, "max_count": 0}
    for k in range(p):                                     # :481
        Dk = D[k].copy()                                   # :482
        users = np.flatnonzero(A[:, k])                    # :487-488
        atom_usage = len(users)                            # :489
        # :490-496 add back the old atom, count column by column for j < m
        weights = (E[users] ^ Dk)[:, :m].sum(axis=0, dtype=np.int64)
        if not atom_usage:                                 # :499
            continue
        st["max_usage"] = max(st["max_usage"], atom_usage)
        st["max_count"] = max(st["max_count"], int(weights.max()))
        u = atom_usage // 2                                # :502
        newDk = Dk.copy()                                  # :503 (the padding bits come along)
        newDk[:m] = weights > u                            # :504-506
        if (newDk ^ Dk).any():                             # :507
            changed += 1                                   # :509
            D[k] = newDk                                   # :510
            E[users] ^= Dk ^ newDk                         # :512-520
    if stats is not None:
        stats.update(st)
    return changed                                         # :526


def residual(X, D, A, p):
    """mul(A, false, D, false, E); add(E, X, E) (bsvd.cpp:1219-1220; mul_AB runs over D's whole words)"""
    return ((A[:, :p].astype(np.int64) @ D[:p].astype(np.int64)) & 1).astype(np.uint8) ^ X


def learn(X, E, D, A, m, p, max_iter=0, coef=update_coefficients_argmin):
    """bsvd.cpp:1215-1244; max_iter (0: none) is bic_bsvd_learn's cap, not the reference's."""
    E[:] = residual(X, D, A, p)                            # :1219-1220
    changed, it = 1, 0                                     # :1222-1223
    while changed > 0:                                     # :1228
        it += 1                                            # :1229
        changed_coefs = coef(E, D, A, p)                   # :1230
        changed = changed_coefs + update_dictionary(E, D, A, m, p)  # :1236
        if max_iter and it >= max_iter:
            break
    return it                                              # :1243


def planted(seed, n, m, p, noise=0.02, flips=0.05, a_flips=0.0):
    """The planted model the tests run on (random matrices at density 0.5 barely move): D0 at density 0.3,
    0 to 2 atoms per row of A0, X = A0 D0 ^ noise, D = D0 ^ flips; A = 0, or A0 with a_flips of its bits
    flipped. Unpacked whole-word arrays with zero padding -> X, D, A, E = X ^ A D."""
    rng = np.random.default_rng(seed)
    M, P = 64 * words(m), 64 * words(p)
    D0 = np.zeros((p, M), np.uint8)
    D0[:, :m] = rng.random((p, m)) < 0.3
    A0 = np.zeros((n, P), np.uint8)
    if n <= 4096:
        for i in range(n):
            A0[i, rng.choice(p, size=min(int(rng.integers(0, 3)), p), replace=False)] = 1
    else:  # the same model drawn for all rows at once
        cnt, k1 = rng.integers(0, 3, n), rng.integers(0, p, n)
        k2 = (k1 + rng.integers(1, max(p, 2), n)) % p
        A0[np.flatnonzero(cnt >= 1), k1[cnt >= 1]] = 1
        A0[np.flatnonzero(cnt >= 2), k2[cnt >= 2]] = 1
    X = residual(np.zeros((n, M), np.uint8), D0, A0, p)
    X[:, :m] ^= rng.random((n, m)) < noise
    D = D0.copy()
    D[:, :m] ^= rng.random((p, m)) < flips
    A = np.zeros_like(A0)
    if a_flips:
        A[:, :p] = A0[:, :p] ^ (rng.random((n, p)) < a_flips)
    return X, D, A, residual(X, D, A, p)
