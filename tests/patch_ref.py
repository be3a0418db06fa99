"""Numpy restatement of the dictionary-learning driver's image mode (test infrastructure: the yardstick of
tests/test_gpu_patch.py and tools/time_bsvd_image.py, pinned by tests/test_patch_ref.py against the oracle's
get_submatrix and against the host binary_matrix loops).

Planes are packed uint64 arrays [rows, pitch], column j at MSB >> (j % 64), as everywhere in the tests.

  gather       bsvd_test.cpp:89-97   copy_submatrix_to (binmat.cpp:267-298, the flat word indexing) +
                                     copy_vectorized_to (binmat.cpp:306-320, its tile read through get_block,
                                     binmat.h:188-190) + set_row
  scatter      bsvd_test.cpp:130-139 copy_row_to + set_vectorized (binmat.cpp:322-341) + set_submatrix
                                     (binmat.cpp:373-414); the valid pixels, with ZERO padding (include/bic.h
                                     states the difference from set_submatrix)
  mosaic_dims  util.cpp:57-61        w = (idx_t)sqrt(m), gn = ceil(sqrt(n)), gm = ceil(n / gn), in integers
  mosaic       util.cpp:53-82        render_mosaic's image
"""
import math

import numpy as np


def words(bits):
    return (bits + 63) // 64


def unpack(P, nwords):
    """the first nwords words of every row -> 0/1 uint8 [rows, 64 nwords]"""
    P = np.ascontiguousarray(np.asarray(P, np.uint64)[:, :nwords])
    return np.unpackbits(P.astype(">u8").view(np.uint8).reshape(P.shape[0], -1), axis=1)


def pack(bits):
    """0/1 [rows, cols] -> packed words [rows, ceil(cols/64)], zero padding"""
    rows, cols = bits.shape
    pad = np.zeros((rows, 64 * words(cols)), np.uint8)
    pad[:, :cols] = bits
    return np.packbits(pad, axis=1).view(">u8").astype(np.uint64).reshape(rows, words(cols))


def tiles(rows, cols, W):
    return (rows + W - 1) // W, (cols + W - 1) // W


def gather_index(rows, cols, W):
    """flat[N, W*W]: for bit r W + c of patch ti Nx + tj, the FLAT bit index of the plane it is read from: a row is
    its first ceil(cols/64) words and the next row follows it at once (binmat.cpp:267-298)"""
    ny, nx = tiles(rows, cols, W)
    used = words(cols)
    ti, tj, r, c = np.meshgrid(np.arange(ny), np.arange(nx), np.arange(W), np.arange(W), indexing="ij")
    return ((ti * W + r) * (64 * used) + tj * W + c).reshape(ny * nx, W * W)


def gather(I, cols, W, stats=None):
    """bsvd_test.cpp:89-97 -> X packed [Ny Nx, ceil(W^2/64)], pad bits 0. The pad bits of a row's last word are read
    as stored, anything past the last row reads 0. stats (dict, optional): how many 1 bits were read from a pad
    column ("pad_ones"), and from the row after the tile row's own ("wrap_ones")."""
    I = np.asarray(I, np.uint64)
    rows, used = I.shape[0], words(cols)
    flat = unpack(I, used).reshape(-1)
    idx = gather_index(rows, cols, W)
    inside = idx < flat.size
    bits = np.where(inside, flat[np.minimum(idx, flat.size - 1)], 0).astype(np.uint8)
    if stats is not None:
        col = idx % (64 * used)
        ny, nx = tiles(rows, cols, W)
        r = np.tile(np.repeat(np.arange(W), W), (ny * nx, 1))
        ti = np.repeat(np.arange(ny), nx)[:, None]
        stats["pad_ones"] = int(bits[inside & (col >= cols)].sum())
        stats["wrap_ones"] = int(bits[inside & (idx // (64 * used) != ti * W + r)].sum())
    return pack(bits)


def scatter(X, W, rows, cols):
    """bsvd_test.cpp:130-139 -> the plane packed [rows, ceil(cols/64)], pad bits 0: pixel (i, j) is bit
    (i mod W) W + (j mod W) of row (i / W) Nx + j / W of X"""
    ny, nx = tiles(rows, cols, W)
    xb = unpack(X, words(W * W))
    i, j = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    return pack(xb[(i // W) * nx + j // W, (i % W) * W + j % W])


def mosaic_dims(n, m):
    """util.cpp:57-61 -> (w, gn, image rows, image cols)"""
    w = math.isqrt(m)
    gn = math.isqrt(n - 1) + 1 if n > 1 else 1
    gm = (n + gn - 1) // gn
    return w, gn, gm * (w + 1), gn * (w + 1)


def mosaic(D, m):
    """util.cpp:53-82 -> the image packed [gm gw, ceil(gn gw / 64)]: pixel (gw i + r, gw j + c) = D(i gn + j, r w + c)"""
    D = np.asarray(D, np.uint64)
    n = D.shape[0]
    w, gn, irows, icols = mosaic_dims(n, m)
    db = unpack(D, words(m))
    img = np.zeros((irows, icols), np.uint8)
    for li in range(n):
        i, j = divmod(li, gn)
        img[(w + 1) * i:(w + 1) * i + w, (w + 1) * j:(w + 1) * j + w] = db[li, :w * w].reshape(w, w)
    return pack(img)
