"""Bit-serial numpy restatement of the reference's second dictionary update rule, update_dictionary_proximus
(bsvd.cpp:530-735; update_dictionary_proximus_omp, :822-1027, is the same text), on the unpacked whole-word
arrays of tests/bsvd_ref.py (test infrastructure: the yardstick of tests/test_gpu_bsvd_prox.py, pinned by
tests/test_bsvd_prox_ref.py; bsvd.cpp itself cannot be built here, it needs GSL).

For every atom, rounds of two halves until a round changes nothing: the atom half is the steepest step for
this one atom (:628-671), the coefficient half votes every row's A(i,k) against the atom (:676-719). The
`#if 0` initialisation (:566-620) is not built. Works in place; returns (changed, rounds): the reference's
return value, the atoms whose D_k changed in some round (:659; :706 is commented out, so an atom whose users
alone changed is not counted), and the number of do-while rounds run over all atoms.

  update_dictionary_proximus   bsvd.cpp:530-735
  learn                        bsvd.cpp:1215-1244 with the dictionary step swapped
"""
import numpy as np

from bsvd_ref import pack, planted, residual, unpack, update_coefficients_argmin  # noqa: F401 (re-exported)
import bsvd_ref


def update_dictionary_proximus(E, D, A, m, p, stats=None, after_half=None):
    """stats (a dict, optional): what the tests want to have seen. after_half(k, round, half) is called after
    every half that ran (half 0 the atom's, 1 the coefficients'), for the invariants of the pinning test."""
    changed, rounds = 0, 0                                 # :551
    st = {"max_rounds": 0, "on": 0, "off": 0, "ties": 0, "recruited": 0, "uncounted": 0, "rounds_per_atom": []}
    for k in range(p):                                     # :555
        kchanged = False                                   # :559
        empty_at_entry = not A[:, k].any()
        users_changed = False
        rk = 0
        while True:                                        # :623 do
            converged = True                               # :624
            rk += 1
            # ---- the atom half, :628-671
            Dk = D[k].copy()                               # :631
            users = np.flatnonzero(A[:, k])                # :633-635
            u = len(users)                                 # :636
            Dw = (E[users] ^ Dk)[:, :m].sum(axis=0, dtype=np.int64)  # :637-643 add back the old atom, count j < m
            if u:                                          # :647
                u //= 2                                    # :649
                newDk = Dk.copy()                          # :650 (the padding bits come along)
                newDk[:m] = Dw > u                         # :651-653
                if (newDk ^ Dk).any():                     # :654-655 dist over whole words
                    D[k] = newDk                           # :657
                    converged = False                      # :658
                    kchanged = True                        # :659
                    E[users] ^= Dk ^ newDk                 # :661-669 whole rows
                if after_half:
                    after_half(k, rk, 0)
            # ---- the coefficient half, :676-719, with the D_k the atom half left
            S = np.flatnonzero(D[k, :m])                   # :681-683 dkj for j < m
            u = len(S)                                     # :684
            Ak = A[:, k].copy()                            # :677
            Aw = (E[:, S] ^ Ak[:, None]).sum(axis=1, dtype=np.int64)  # :685-691 every row, add back the old coefs
            if u:                                          # :694
                st["ties"] += int((2 * Aw == u).sum())     # Aw = |S| / 2 with |S| even: the vote gives 0
                u //= 2                                    # :696
                newAk = (Aw > u).astype(np.uint8)          # :698-700
                flip = np.flatnonzero(newAk ^ Ak)          # :701
                if len(flip):                              # :702
                    A[:, k] = newAk                        # :704
                    converged = False                      # :705 (:706 kchanged = true is commented out)
                    users_changed = True
                    st["on"] += int(newAk[flip].sum())
                    st["off"] += int(len(flip) - newAk[flip].sum())
                    E[np.ix_(flip, S)] ^= 1                # :708-716 the columns j < m with dkj set
                if after_half:
                    after_half(k, rk, 1)
            if converged:                                  # :720
                break
        rounds += rk
        st["rounds_per_atom"].append(rk)
        st["max_rounds"] = max(st["max_rounds"], rk)
        st["recruited"] += int(empty_at_entry and users_changed)
        st["uncounted"] += int(users_changed and not kchanged)
        if kchanged:                                       # :724
            changed += 1                                   # :725
    if stats is not None:
        stats.update(st)
    return changed, rounds                                 # :734


def learn(X, E, D, A, m, p, max_iter=0):
    """bsvd.cpp:1215-1244 with update_dictionary = update_dictionary_proximus: bsvd_ref.learn with the dictionary
    step swapped (the sum of :1236 takes this step's return value, the atoms whose bits changed)."""
    step = bsvd_ref.update_dictionary
    bsvd_ref.update_dictionary = lambda E, D, A, m, p: update_dictionary_proximus(E, D, A, m, p)[0]
    try:
        return bsvd_ref.learn(X, E, D, A, m, p, max_iter)
    finally:
        bsvd_ref.update_dictionary = step
