"""Numpy restatement of the reference's role-switching learners, learn_model_alter1 / 2 / 3 (bsvd.cpp:1247-1434),
over the steps of tests/bsvd_ref.py and tests/bsvd_prox_ref.py, on their unpacked whole-word arrays (test
infrastructure: the yardstick of tests/test_gpu_bsvd_wide.py and tests/test_gpu_bsvd_alter.py, pinned by
tests/test_bsvd_alter_ref.py; bsvd.cpp itself cannot be built here, it needs GSL).

The learners transpose A, D and E, run the same two steps with the roles exchanged -- update_coefficients(Et, At,
Dt), update_dictionary(Et, At, Dt): Et (m x n) the residual, At's p rows of n bits the atoms, Dt (m x p) the
coefficients -- and transpose back. transpose_to clears the padding (binmat.cpp:199-208): T crops, transposes and
zero-pads to whole words. Everything works in place and returns the reference's return value.

du: 0 update_dictionary_steepest, 1 update_dictionary_proximus (its changed count; the rounds are dropped).
max_iter (0: none) is bic_bsvd_learn_lm's cap, not the reference's: it counts every iter++ of the text over the
whole call, and the pass that reaches it is finished, transposes back included.
trace (a list, optional) receives one tuple per step run: (role, step, count) with role "d" / "t" and step
"c" (sparse coding) / "u" (dictionary).
"""
import numpy as np

import bsvd_prox_ref as P
import bsvd_ref as R
from bsvd_ref import words


def T(B, r, c):
    """B cropped to r x c, transposed, zero-padded to whole words: [c, 64 ceil(r/64)]"""
    out = np.zeros((c, 64 * words(r)), np.uint8)
    out[:, :r] = B[:r, :c].T
    return out


def dict_step(E, D, A, m, p, du):
    if du:
        return P.update_dictionary_proximus(E, D, A, m, p)[0]
    return R.update_dictionary(E, D, A, m, p)


class _Run:
    def __init__(self, E, D, A, m, p, du, max_iter, trace):
        self.E, self.D, self.A, self.n, self.m, self.p, self.du = E, D, A, E.shape[0], m, p, du
        self.max_iter, self.total, self.trace = max_iter, 0, trace

    def note(self, role, step, count):
        if self.trace is not None:
            self.trace.append((role, step, count))
        return count

    def coef(self):
        return self.note("d", "c", R.update_coefficients_argmin(self.E, self.D, self.A, self.p))

    def dict(self):
        return self.note("d", "u", dict_step(self.E, self.D, self.A, self.m, self.p, self.du))

    def there(self):
        self.At, self.Dt, self.Et = T(self.A, self.n, self.p), T(self.D, self.p, self.m), T(self.E, self.n, self.m)

    def coef_t(self):
        return self.note("t", "c", R.update_coefficients_argmin(self.Et, self.At, self.Dt, self.p))

    def dict_t(self):
        return self.note("t", "u", dict_step(self.Et, self.At, self.Dt, self.n, self.p, self.du))

    def back(self):
        self.A[:] = T(self.At, self.p, self.n)
        self.D[:] = T(self.Dt, self.m, self.p)
        self.E[:] = T(self.Et, self.m, self.n)

    def capped(self):
        self.total += 1
        return bool(self.max_iter) and self.total >= self.max_iter


def learn_alter1(X, E, D, A, m, p, du=0, max_iter=0, trace=None):
    """bsvd.cpp:1247-1312"""
    E[:] = R.residual(X, D, A, p)                          # :1256-1257
    r = _Run(E, D, A, m, p, du, max_iter, trace)
    changed, it = 1, 0                                     # :1265-1266
    while changed > 0:                                     # :1271
        it += 1                                            # :1272
        changed_coefs = r.coef()                           # :1273
        changed = changed_coefs + r.dict()                 # :1279
        r.there()                                          # :1286-1288
        changed_coefs = r.coef_t()                         # :1290
        changed = r.dict_t()                               # :1297 overwrites everything before it
        r.back()                                           # :1304-1306
        if r.capped():
            break
    return it                                              # :1311


def learn_alter2(X, E, D, A, m, p, du=0, max_iter=0, trace=None):
    """bsvd.cpp:1315-1385"""
    E[:] = R.residual(X, D, A, p)                          # :1324-1325
    r = _Run(E, D, A, m, p, du, max_iter, trace)
    changed, it = 1, 0                                     # :1329-1330
    outer_changed = 1                                      # :1336
    while outer_changed > 0:                               # :1337
        outer_changed = 0                                  # :1338
        while changed > 0:                                 # :1339 (0 on a second outer pass: skipped)
            it += 1                                        # :1340
            changed_coefs = r.coef()                       # :1341
            changed = changed_coefs + r.dict()             # :1347
            outer_changed += changed                       # :1353
            if r.capped():
                return it
        r.there()                                          # :1355-1357
        changed, it = 1, 0                                 # :1358-1359
        stop = False
        while changed > 0:                                 # :1360
            it += 1                                        # :1361
            changed_coefs = r.coef_t()                     # :1362
            changed = changed_coefs + r.dict_t()           # :1369
            outer_changed += changed                       # :1375
            if r.capped():
                stop = True
                break
        r.back()                                           # :1377-1379
        if stop:
            break
    return it                                              # :1384


def learn_alter3(X, E, D, A, m, p, du=0, max_iter=0, trace=None):
    """bsvd.cpp:1388-1434"""
    E[:] = R.residual(X, D, A, p)                          # :1396-1397
    r = _Run(E, D, A, m, p, du, max_iter, trace)
    changed, it = p + 1, 0                                 # :1402-1403
    while changed > 0:                                     # :1408
        it += 1                                            # :1409
        r.there()                                          # :1410-1412
        changed = r.dict_t()                               # :1413
        r.back()                                           # :1420-1422
        changed = r.dict()                                 # :1423 only the direct step decides
        if r.capped():
            break
    return it                                              # :1433


def learn_traditional(X, E, D, A, m, p, du=0, max_iter=0):
    """bsvd.cpp:1215-1244 with either rule (bsvd_ref.learn / bsvd_prox_ref.learn)"""
    return (P.learn if du else R.learn)(X, E, D, A, m, p, max_iter)


LEARNERS = {0: learn_traditional, 1: learn_alter1, 2: learn_alter2, 3: learn_alter3}


def learn(lm, X, E, D, A, m, p, du=0, max_iter=0, trace=None):
    if lm == 0:
        return learn_traditional(X, E, D, A, m, p, du, max_iter)
    return LEARNERS[lm](X, E, D, A, m, p, du, max_iter, trace)
