"""bic_bsvd_learn_image, the driver's image mode as one call, against its five parts called one by one
(bic_patches_gather, E = X, bic_bsvd_initialize, bic_bsvd_learn_lm, bic_patches_scatter): every word of X, E, D, A
and the residual image, pitch words included, the generator's state and the iteration count. The plane is a
glyph-like page of 96 x 100 pixels in 8 x 8 patches (156 samples of 64 bits), p = 16; the restatements
(tests/bsvd_init_ref.py + tests/bsvd_ref.py over tests/patch_ref.py) say that a run on it learns something."""
import functools

import numpy as np
import pytest

import bsvd_init_ref as I
import bsvd_ref as R
import patch_ref as P
import pybic
from oracle_lib import text_plane
from pybic import as_u64

pytestmark = pytest.mark.gpu

ROWS, COLS, W, ATOMS = 96, 100, 8, 16
M = W * W
POISON = np.uint64(0x5A5AA5A5C3C33C3C)


@functools.lru_cache(maxsize=None)
def page():
    plane = text_plane(20, ROWS, COLS)
    rng = np.random.default_rng(3)
    plane[:, -1] |= rng.integers(0, 1 << 64, ROWS, dtype=np.uint64) & np.uint64((1 << (64 - COLS % 64)) - 1)
    return plane


@functools.lru_cache(maxsize=None)
def restated(mi):
    """(|X|, |E| after learning, iterations) by the restatements, traditional learner, steepest rule"""
    X = R.unpack(P.gather(page(), COLS, W))
    D, A = I.initialize(mi, X, M, ATOMS, I.Rand48())
    E = X.copy()
    it = R.learn(X, E, D, A, M, ATOMS)
    return int(X.sum()), int(E.sum()), it


def buffers(ctx, n):
    def poisoned(rows, words):
        return ctx.to_dev(np.full((rows, words + 1), POISON, np.uint64))
    return {"X": poisoned(n, 1), "E": poisoned(n, 1), "D": poisoned(ATOMS, 1), "A": poisoned(n, 1),
            "R": poisoned(ROWS, P.words(COLS))}


@pytest.mark.parametrize("mi", [pybic.BSVD_MI_NEIGHBOR, pybic.BSVD_MI_PARTITION])
def test_the_page_can_be_learned(mi):
    wx, we, it = restated(mi)
    assert it >= 1 and we < wx, (wx, we, it)


@pytest.mark.parametrize("du", [pybic.BSVD_DU_STEEPEST, pybic.BSVD_DU_PROXIMUS])
@pytest.mark.parametrize("lm", [pybic.BSVD_LM_TRADITIONAL, pybic.BSVD_LM_ALTER1])
@pytest.mark.parametrize("mi", [pybic.BSVD_MI_NEIGHBOR, pybic.BSVD_MI_PARTITION])
def test_one_call_is_the_five_calls(ctx, mi, lm, du):
    ny, nx = P.tiles(ROWS, COLS, W)
    n = ny * nx
    assert (n, M) == (156, 64)
    plane = ctx.to_dev(page())
    seed = pybic.bsvd_rng_seed(I.RANDOM_SEED)
    # the five calls
    a = buffers(ctx, n)
    ctx.patches_gather(plane, COLS, W, out=a["X"])
    a["E"][:, :1] = a["X"][:, :1]
    st_a = ctx.bsvd_initialize(mi, a["E"], M, a["D"], a["A"], ATOMS, state=seed)
    it_a = ctx.bsvd_learn(a["X"], a["E"], M, a["D"], a["A"], ATOMS, du=du, lm=lm)
    ctx.patches_scatter(a["E"], W, ROWS, COLS, out=a["R"])
    # the one call, with and without the residual image
    b, c = buffers(ctx, n), buffers(ctx, n)
    it_b, st_b = ctx.bsvd_learn_image(plane, COLS, W, b["X"], b["E"], b["D"], b["A"], ATOMS, mi=mi, lm=lm, du=du,
                                      state=seed, residual=b["R"])
    it_c, st_c = ctx.bsvd_learn_image(plane, COLS, W, c["X"], c["E"], c["D"], c["A"], ATOMS, mi=mi, lm=lm, du=du,
                                      state=seed)
    ctx.sync()
    X = as_u64(a["X"])
    assert np.array_equal(X[:, :1], P.gather(page(), COLS, W))
    wx, we = int(R.unpack(X, 1).sum()), int(R.unpack(as_u64(a["E"]), 1).sum())
    assert it_a >= 1 and we < wx, (wx, we, it_a)   # the run learns something
    assert (st_a == seed) == (mi == pybic.BSVD_MI_PARTITION)   # only the neighbour rule draws
    assert (it_b, st_b) == (it_a, st_a) and (it_c, st_c) == (it_a, st_a)
    for key in ("X", "E", "D", "A", "R"):
        want = as_u64(a[key])
        assert (want[:, -1] == POISON).all(), key
        assert np.array_equal(as_u64(b[key]), want), key
        if key != "R":
            assert np.array_equal(as_u64(c[key]), want), key
    assert (as_u64(c["R"]) == POISON).all()  # residual = NULL: nothing is written
    assert np.array_equal(as_u64(a["R"])[:, :-1], P.scatter(as_u64(a["E"]), W, ROWS, COLS))


def test_w_above_64_is_refused(ctx):
    rows, cols, w = 70, 200, 65
    n, xw = 2 * 4, P.words(w * w)
    plane = ctx.to_dev(np.zeros((rows, 4), np.uint64))
    X, E = (ctx.to_dev(np.full((n, xw), POISON, np.uint64)) for _ in range(2))
    D = ctx.to_dev(np.full((ATOMS, xw), POISON, np.uint64))
    A = ctx.to_dev(np.full((n, 1), POISON, np.uint64))
    with pytest.raises(pybic.BicError) as e:
        ctx.bsvd_learn_image(plane, cols, w, X, E, D, A, ATOMS, state=pybic.bsvd_rng_seed(1))
    assert e.value.code == pybic.BIC_EINVAL
    ctx.sync()
    for t in (X, E, D, A):
        assert (as_u64(t) == POISON).all()
