"""Bit-serial numpy restatement of the growing-dictionary tile loop of the reference's
compress2_test.cpp:79-129 (variant 2) and compress3_test.cpp:87-149 (variant 3): TEST INFRASTRUCTURE, the
expected side of tests/test_gpu_dict.py, itself pinned to the drivers' own output by tests/test_dict_ref.py
(tests/golden/dict.npz, made by tests/golden/make_golden_dict.py from the drivers compiled as they are).

Pixels are handled one bool each; nothing here is word-parallel and nothing is shared with the device code.

* get_submatrix (binmat.cpp:259-298) reads word k = i0 * blocks_per_row + j0 / 64 (+ the next one) of the
  flat buffer, words past it as 0: row r of the window is the W bits from flat bit (i0 + r) * 64 *
  blocks_per_row + j0 on, so a window past the right edge continues in the next row and past the last row
  it is 0.
* The dictionary holds tile INDEX pairs (i, j) (compress2_test.cpp:105,124; compress3_test.cpp:118,145) and
  atom windows are read at PIXEL (c.i, c.j) (:87-88 / :95-96). atom_step scales the pair: 1 is the drivers'
  behaviour, W reads the tile itself.
"""
import math

import numpy as np


def flat_bits(plane, cols):
    """the plane's first ceil(cols/64) words per row as one flat bool vector, followed by zeros"""
    plane = np.ascontiguousarray(plane, np.uint64)
    rows = plane.shape[0]
    used = (cols + 63) // 64
    words = np.ascontiguousarray(plane[:, :used]).astype(">u8")
    bits = np.unpackbits(words.view(np.uint8).reshape(-1)).astype(bool)
    return np.concatenate([bits, np.zeros(64 * (used + 2) + 64 * used * 64, bool)]), used, rows


def window(flat, used, i, j, W):
    """get_submatrix(i, i + W, j, j + W) as W*W bools (rows past the buffer read the zeros after it)"""
    out = np.zeros((W, W), bool)
    for r in range(W):
        s = (i + r) * used * 64 + j
        if s + W <= flat.size:
            out[r] = flat[s:s + W]
        elif s < flat.size:
            out[r, :flat.size - s] = flat[s:]
    return out.reshape(-1)


def dict_encode(plane, cols, variant, W, T, atom_step, enuml):
    """-> dict of per-tile arrays, the dictionary, the two sample sequences and the totals"""
    assert variant in (2, 3) and atom_step in (1, W)
    flat, used, rows = flat_bits(plane, cols)
    M = W * W
    ny, nx = (W - 1 + rows) // W, (W - 1 + cols) // W
    nt = ny * nx
    h = 0.5 * math.log2(float(M)) if variant == 2 else 0.0        # :103 / compress3_test.cpp:111-115
    atoms = np.zeros((nt, M), bool)                                 # atom windows, dictionary order
    nD = 0
    out = {k: np.zeros(nt, np.uint32) for k in ("bestk", "bestd", "dsize", "weights", "ties")}
    out["nomatch_len"] = np.zeros(nt, np.uint64)
    out["match_len"] = np.zeros(nt, np.uint64)
    modes, joined, dict_tiles = bytearray(nt), np.zeros(nt, np.uint8), []
    s_match, s_nomatch = [], []
    L = matches = 0
    for t in range(nt):
        i, j = divmod(t, nx)
        P = window(flat, used, i * W, j * W, W)                     # :83 / :91
        bestk, bestd, ties = 0, M, 0
        if nD:                                                      # :86-98 / :94-106: strict <, first zero ends it
            d = (atoms[:nD] ^ P).sum(axis=1)
            k = int(np.argmin(d))                                   # (the first of the least)
            if d[k] < M:
                bestk, bestd = k, int(d[k])
                ties = int((d == d[k]).sum())
        wP = int(P.sum())
        nomatch_len = int((1 + enuml[wP]) + h)                      # :103 / :116
        out["bestk"][t], out["bestd"][t], out["dsize"][t], out["ties"][t] = bestk, bestd, nD, ties
        out["nomatch_len"][t] = nomatch_len
        push = False
        if nD == 0:                                                 # :104-109 / :117-122: no sample coded
            push, match = True, False
            L += nomatch_len
        else:
            match_len = int(((1 + math.ceil(math.log2(nD))) + enuml[bestd]) + h)   # :115 / :128
            out["match_len"][t] = match_len
            match = nomatch_len > match_len                         # :118 / :131
            L += match_len if match else nomatch_len
            if variant == 2:
                push = not match                                    # :122-126
            else:
                (s_match if match else s_nomatch).append(bestd if match else wP)   # :136 / :140
                push = bestd > T                                    # :143
        matches += match
        modes[t] = ord("x" if match else "o")
        out["weights"][t] = bestd if match else wP
        if push:
            atoms[nD] = window(flat, used, i * atom_step, j * atom_step, W)
            dict_tiles.append(t)
            joined[t] = 1
            nD += 1
    out.update(modes=bytes(modes).decode(), joined=joined, dict_tiles=np.array(dict_tiles, np.uint32),
               samples_match=np.array(s_match, np.uint32), samples_nomatch=np.array(s_nomatch, np.uint32),
               matches=int(matches), L=int(L), nD=nD, nx=nx, ny=ny)
    return out


def glyph_plane(seed, rows, cols, W, noise_share=0.7, flips=(0, 1, 2, 0, 40, 3, 0, 45), period=4):
    """A glyph-like page on the W-tile grid: one glyph g0 (a random period x period cell repeated over the
    tile, so a window at any pixel of a run of g0 tiles is g0 shifted), tiles of g0 with a few or many
    pixels flipped (`flips`, in turn), and noise tiles (a share of `noise_share`, placed at random). The
    first two tile rows and columns are g0 itself: with atom_step = 1 every atom window lies inside them
    as long as the tile grid is at most W x W, and atom 0 is g0 in both modes."""
    from oracle_lib import pack_rows
    rng = np.random.default_rng(seed)
    cell = rng.random((period, period)) < 0.5
    g0 = np.tile(cell, (W // period + 1, W // period + 1))[:W, :W]
    ny, nx = rows // W, cols // W
    bits = np.zeros((rows, cols), bool)
    n = 0
    for i in range(ny):
        for j in range(nx):
            if i < 2 and j < 2:
                tile = g0
            elif rng.random() < noise_share:
                tile = rng.random((W, W)) < 0.5
            else:
                tile = g0.copy().reshape(-1)
                tile[rng.choice(W * W, flips[n % len(flips)], replace=False)] ^= True
                tile = tile.reshape(W, W)
                n += 1
            bits[i * W:(i + 1) * W, j * W:(j + 1) * W] = tile
    return pack_rows(bits)
