"""The image-mode kernels (bic_patch.hip; include/bic.h bic_patches_gather, bic_patches_scatter, bic_mosaic) against
tests/patch_ref.py, which tests/test_patch_ref.py pins to get_submatrix and to the host binary_matrix loops. All own
words and all pitch words are compared: every input has dirty padding, source and destination pitches are one word
more than needed, and the pitch words hold a poison pattern that must survive. Each case first asserts on the
restatement that it meets the path it is there for."""
import functools

import numpy as np
import pytest

import patch_ref as P
import pybic
from pybic import as_u64

pytestmark = pytest.mark.gpu

POISON = np.uint64(0xDEADBEEFCAFEF00D)
# (rows, cols, W): straddling fields, the wrap into the next row and the bottom-right tile past the last row; the
# wrap out of word-exact rows; aligned; W = 63 and 64; one-bit tiles; W > 64; 65 words per row (more than one work
# item per tile row). The last two are the sizes at which a work item no longer holds a tile's W rows (gather) or a
# tile's whole row of X (scatter): words of X, and tile rows, are then split over work items.
GEOMS = [(37, 126, 5), (17, 64, 3), (64, 128, 16), (40, 130, 63), (130, 200, 64), (9, 9, 1), (70, 200, 65),
         (70, 4100, 16), (600, 130, 520), (1030, 70, 1024)]
WRAPS = [(37, 126, 5), (17, 64, 3)]
MOSAICS = [(5, 25), (7, 70), (512, 256), (3, 4500), (17, 4096), (65, 9)]


def pitched(M):
    """M with one poisoned word appended to every row"""
    return np.concatenate([M, np.full((M.shape[0], 1), POISON, np.uint64)], axis=1)


@functools.lru_cache(maxsize=None)
def case(rows, cols, W):
    """one random image with dirty padding per geometry, random samples of its shape, and both restatements"""
    rng = np.random.default_rng(rows * 100003 + cols * 101 + W)
    used, xw = P.words(cols), P.words(W * W)
    I = rng.integers(0, 1 << 64, (rows, used), dtype=np.uint64)
    st = {}
    X = P.gather(I, cols, W, st)
    ny, nx = P.tiles(rows, cols, W)
    Xs = rng.integers(0, 1 << 64, (ny * nx, xw), dtype=np.uint64)  # (its own pad bits are dirty too)
    return {"I": I, "X": X, "st": st, "Xs": Xs, "back": P.scatter(Xs, W, rows, cols), "n": ny * nx, "nx": nx}


@pytest.mark.parametrize("rows,cols,W", GEOMS)
def test_gather(ctx, rows, cols, W):
    c = case(rows, cols, W)
    if cols % 64 and c["nx"] * W > cols:
        assert c["st"]["pad_ones"] > 0   # a 1 read from a pad bit
    if (rows, cols, W) in WRAPS:
        assert c["st"]["wrap_ones"] > 0  # a 1 read from the next row
    xw = P.words(W * W)
    out0 = np.full((c["n"], xw + 1), POISON, np.uint64)
    out = ctx.to_dev(out0)
    got = ctx.patches_gather(ctx.to_dev(pitched(c["I"])), cols, W, out=out)
    ctx.sync()
    got = as_u64(got)
    assert np.array_equal(got[:, :xw], c["X"])
    assert (got[:, xw] == POISON).all()


@pytest.mark.parametrize("fill", [0, 0xFFFFFFFFFFFFFFFF])
@pytest.mark.parametrize("rows,cols,W", GEOMS)
def test_scatter(ctx, rows, cols, W, fill):
    """over a plane of zeros and over a plane of ones: no stale bit, pad bits 0, pitch words kept"""
    c = case(rows, cols, W)
    used = P.words(cols)
    plane0 = np.full((rows, used + 1), np.uint64(fill), np.uint64)
    plane0[:, used] = POISON
    plane = ctx.to_dev(plane0)
    ctx.patches_scatter(ctx.to_dev(pitched(c["Xs"])), W, rows, cols, out=plane)
    ctx.sync()
    got = as_u64(plane)
    assert np.array_equal(got[:, :used], c["back"])
    assert (got[:, used] == POISON).all()


@pytest.mark.parametrize("rows,cols,W", GEOMS)
def test_round_trip(ctx, rows, cols, W):
    c = case(rows, cols, W)
    X = ctx.patches_gather(ctx.to_dev(c["I"]), cols, W)
    back = ctx.patches_scatter(X, W, rows, cols)
    ctx.sync()
    want = P.pack(P.unpack(c["I"], P.words(cols))[:, :cols])  # the valid pixels, pads 0
    assert np.array_equal(as_u64(back), want)


@pytest.mark.parametrize("n,m", MOSAICS)
def test_mosaic(ctx, n, m):
    rng = np.random.default_rng(n * 7919 + m)
    mw = P.words(m)
    D = rng.integers(0, 1 << 64, (n, mw), dtype=np.uint64)  # bits w^2 .. m - 1 and the padding are dirty
    want = P.mosaic(D, m)
    w, _, irows, icols = P.mosaic_dims(n, m)
    assert ctx.mosaic_dims(n, m) == (irows, icols)
    if w * w < m or m % 64:
        assert P.unpack(D, mw)[:, w * w:].any()
    img0 = np.full((irows, P.words(icols) + 1), POISON, np.uint64)
    img = ctx.to_dev(img0)
    ctx.mosaic(ctx.to_dev(pitched(D)), m, out=img)
    ctx.sync()
    got = as_u64(img)
    assert np.array_equal(got[:, :-1], want)
    assert (got[:, -1] == POISON).all()


def test_einval_launches_nothing(ctx):
    rows, cols, W = 37, 126, 5
    c = case(rows, cols, W)
    lib, h, p = ctx.lib, ctx.h, pybic._p
    I = ctx.to_dev(c["I"])
    xw = P.words(W * W)
    X0 = np.full((c["n"], xw), POISON, np.uint64)
    X = ctx.to_dev(X0)
    plane0 = np.full((rows, 2), POISON, np.uint64)
    plane = ctx.to_dev(plane0)
    D = ctx.to_dev(np.full((5, 1), POISON, np.uint64))
    img = ctx.to_dev(np.full((12, 1), POISON, np.uint64))
    ctx._bind_stream()
    bad = [
        lib.bic_patches_gather(h, p(I), rows, cols, 2, 0, p(X), xw),
        lib.bic_patches_gather(h, p(I), rows, cols, 2, 1025, p(X), 16420),
        lib.bic_patches_gather(h, p(I), rows, cols, 1, W, p(X), xw),       # a short plane pitch
        lib.bic_patches_gather(h, p(I), rows, cols, 2, 6, p(X), 0),         # a short pitch of X
        lib.bic_patches_gather(h, None, rows, cols, 2, W, p(X), xw),
        lib.bic_patches_gather(h, p(I), rows, cols, 2, W, None, xw),
        lib.bic_patches_gather(h, p(I), 0, cols, 2, W, p(X), xw),
        lib.bic_patches_scatter(h, p(X), xw, 0, p(plane), rows, cols, 2),
        lib.bic_patches_scatter(h, p(X), xw, 1025, p(plane), rows, cols, 2),
        lib.bic_patches_scatter(h, p(X), xw, W, p(plane), rows, cols, 1),
        lib.bic_patches_scatter(h, p(X), 0, W, p(plane), rows, cols, 2),
        lib.bic_patches_scatter(h, None, xw, W, p(plane), rows, cols, 2),
        lib.bic_patches_scatter(h, p(X), xw, W, None, rows, cols, 2),
        lib.bic_mosaic(h, p(D), 5, 0, 1, p(img), 1),
        lib.bic_mosaic(h, p(D), 5, 1048577, 16385, p(img), 1),
        lib.bic_mosaic(h, p(D), 0, 25, 1, p(img), 1),
        lib.bic_mosaic(h, p(D), 5, 25, 0, p(img), 1),                      # a short pitch of D
        lib.bic_mosaic(h, p(D), 5, 70, 2, p(img), 0),                      # a short image pitch
        lib.bic_mosaic(h, None, 5, 25, 1, p(img), 1),
        lib.bic_mosaic(h, p(D), 5, 25, 1, None, 1),
    ]
    ctx.sync()
    assert bad == [pybic.BIC_EINVAL] * len(bad)
    assert (as_u64(X) == POISON).all() and (as_u64(plane) == POISON).all() and (as_u64(img) == POISON).all()
