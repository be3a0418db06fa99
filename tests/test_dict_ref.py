"""tests/dict_ref.py (the numpy restatement of compress2_test.cpp:79-129 / compress3_test.cpp:87-149 that the GPU
tests compare against) equals what the drivers themselves printed (tests/golden/dict.npz, made by
tests/golden/make_golden_dict.py from the drivers compiled as they are) at atom_step = 1; hand-worked cases; and
the conditions the inputs must meet for the GPU comparison to mean something. CPU only."""
import json
import os

import numpy as np
import pytest

import dict_cases
import dict_ref
from oracle_lib import pack_rows

GOLD = dict_cases.GOLDEN
RUNS = [(n, v) for n, c in enumerate(dict_cases.CASES) for v in c["variants"]]


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(GOLD, "dict.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLD, "dict.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def restated(gold):
    """every (case, variant) at atom_step = 1 with the recorded enumL table, computed once"""
    _, arrays = gold
    out = {}
    for n, v in RUNS:
        case = dict_cases.CASES[n]
        plane, rows, cols = dict_cases.make_input(case)
        out[n, v] = dict_ref.dict_encode(plane, cols, v, case["W"], case["T"], 1, arrays[f"enuml_W{case['W']}"])
    return out


def fmt6(x):
    """what `std::cout << double` prints (6 significant digits)"""
    return float("%.6g" % x)


@pytest.mark.parametrize("n,v", RUNS)
def test_restatement_equals_the_drivers(gold, restated, oracle, n, v):
    meta, arrays = gold
    case, r = dict_cases.CASES[n], restated[n, v]
    plane, rows, cols = dict_cases.make_input(case)
    assert np.array_equal(plane, arrays[f"c{n}_plane"]) and (meta[n]["rows"], meta[n]["cols"]) == (rows, cols)
    g = {k: arrays[f"c{n}_v{v}_{k}"] for k in ("i", "j", "bestk", "bestd", "dsize", "nomatch_len", "match_len",
                                              "has_lens", "use_match", "add")}
    W, nt = case["W"], len(g["i"])
    assert nt == r["nx"] * r["ny"]
    assert np.array_equal(g["i"], (np.arange(nt) // r["nx"]) * W) and np.array_equal(g["j"], (np.arange(nt) % r["nx"]) * W)
    for k in ("bestk", "bestd", "dsize"):
        assert np.array_equal(g[k], r[k]), k
    # the lengths are printed for every tile but the one that meets an empty dictionary
    assert g["has_lens"].tolist() == [0] + [1] * (nt - 1)
    assert np.array_equal(g["nomatch_len"][1:], r["nomatch_len"][1:])
    assert np.array_equal(g["match_len"][1:], r["match_len"][1:])
    modes = np.frombuffer(r["modes"].encode(), np.uint8)
    assert np.array_equal(g["use_match"] != 0, modes == ord("x"))
    # "ADD TO DICT!" is every push but the first tile's (pushed without a line)
    assert g["add"][0] == 0 and r["joined"][0] == 1
    assert np.array_equal(g["add"][1:], r["joined"][1:])
    s = meta[n]["variants"][str(v)]
    if v == 2:
        assert float(s["comp"]) == fmt6(r["L"])
    else:
        o = oracle
        bm, bn = o.golomb_samples(r["samples_match"], False)[0], o.golomb_samples(r["samples_nomatch"], False)[0]
        assert int(s["matches"]) == r["matches"] and r["matches"] not in (0, nt)
        assert int(s["golomb_per_match"]) == bm // r["matches"]
        assert int(s["golomb_per_nomatch"]) == bn // (nt - r["matches"])
        assert float(s["comp"]) == fmt6((r["L"] + bm + bn) / 8)


def table(W):
    import dropin_expect
    return np.array([dropin_expect.enumL(W * W, w) for w in range(W * W + 1)])


def test_hand_first_tile_and_no_atom_beats_M():
    """2 x 4, W = 2, atom_step = W: tile 0 = 00/00 meets an empty dictionary (pushed, 'o', no sample even in
    variant 3); tile 1 = 11/11 is at distance 4 = M from it: strict < keeps (bestk, bestd) = (0, M)."""
    plane = pack_rows(np.array([[0, 0, 1, 1], [0, 0, 1, 1]], bool))
    e = table(2)  # log2 C(4, w): 0, 2, 2.58.., 2, 0
    r = dict_ref.dict_encode(plane, 4, 3, 2, 0, 2, e)
    assert r["bestk"].tolist() == [0, 0] and r["bestd"].tolist() == [4, 4] and r["dsize"].tolist() == [0, 1]
    # tile 1: nomatch_len = (idx_t)(1 + 0) = 1, match_len = (idx_t)(1 + ceil(log2 1) + 0) = 1: not a match
    assert r["modes"] == "oo" and r["nomatch_len"].tolist() == [1, 1] and r["match_len"].tolist() == [0, 1]
    assert r["samples_match"].tolist() == [] and r["samples_nomatch"].tolist() == [4]  # tile 0 codes nothing
    assert r["joined"].tolist() == [1, 1] and r["dict_tiles"].tolist() == [0, 1] and r["L"] == 2  # bestd 4 > T 0
    r2 = dict_ref.dict_encode(plane, 4, 2, 2, 0, 2, e)  # variant 2: h = 0.5 log2 4 = 1 on both lengths
    assert r2["nomatch_len"].tolist() == [2, 2] and r2["match_len"].tolist() == [0, 2] and r2["modes"] == "oo"
    assert r2["joined"].tolist() == [1, 1] and r2["L"] == 4


def test_hand_first_argmin_and_independent_join():
    """2 x 8, W = 2, atom_step = W, variant 3, T = 0. Tiles: A = 10/00, B = 01/00, C = 11/00 (distance 1 from
    both A and B: the tie goes to atom 0), A again (perfect match at atom 0, which is not the last)."""
    bits = np.array([[1, 0, 0, 1, 1, 1, 1, 0], [0, 0, 0, 0, 0, 0, 0, 0]], bool)
    r = dict_ref.dict_encode(pack_rows(bits), 8, 3, 2, 0, 2, table(2))
    assert r["dsize"].tolist() == [0, 1, 2, 3]
    assert r["bestk"].tolist() == [0, 0, 0, 0] and r["bestd"].tolist() == [4, 2, 1, 0] and r["ties"][2] == 2
    # lengths: nomatch 1 + log2 C(4, w) -> 3, 3, 3, 3; match 1 + ceil(log2 |D|) + log2 C(4, d) -> -, 3, 4, 3
    assert r["nomatch_len"].tolist() == [3, 3, 3, 3] and r["match_len"].tolist() == [0, 3, 4, 3]
    assert r["modes"] == "oooo" and r["samples_nomatch"].tolist() == [1, 2, 1]
    assert r["joined"].tolist() == [1, 1, 1, 0]  # C joins (bestd 1 > T), the repeat of A does not (bestd 0)


def test_hand_atom_step_1_reads_the_pixel_of_the_index():
    """4 x 4, W = 2: tile 3 (index pair (1, 1)) is 11/11. With atom_step = 1 its atom is the window at PIXEL
    (1, 1), i.e. rows 1-2 x cols 1-2 = 0 1 / 1 1 here, not the tile."""
    bits = np.array([[0, 0, 0, 0], [0, 0, 1, 0], [0, 1, 1, 1], [0, 0, 1, 1]], bool)
    plane = pack_rows(bits)
    flat, used, _ = dict_ref.flat_bits(plane, 4)
    assert dict_ref.window(flat, used, 1, 1, 2).astype(int).tolist() == [0, 1, 1, 1]
    assert dict_ref.window(flat, used, 2, 2, 2).astype(int).tolist() == [1, 1, 1, 1]
    # past the right edge a window continues in the same word's pad bits (0), past the last row it reads 0
    assert dict_ref.window(flat, used, 3, 3, 2).astype(int).tolist() == [1, 0, 0, 0]


MAIN = [(n, v, step) for n, c in enumerate(dict_cases.CASES) if c.get("main") for v in c["variants"]
        for step in (1, c["W"])]


@pytest.mark.parametrize("n,v,step", MAIN)
def test_input_conditions(gold, n, v, step):
    """a vacuous input fails here, not silently on the GPU"""
    _, arrays = gold
    case = dict_cases.CASES[n]
    plane, rows, cols = dict_cases.make_input(case)
    r = dict_ref.dict_encode(plane, cols, v, case["W"], case["T"], step, arrays[f"enuml_W{case['W']}"])
    match = np.frombuffer(r["modes"].encode(), np.uint8) == ord("x")
    assert 0.2 <= match.mean() <= 0.8
    assert ((r["ties"] >= 2) & (r["dsize"] > 0)).any()                                    # a tied minimum
    assert ((r["bestd"] == 0) & (r["dsize"] > 0) & (r["bestk"] + 1 < r["dsize"])).any()   # perfect, not the last atom
    if v == 3:
        assert (match & (r["bestd"] > case["T"])).any() and (match & (r["joined"] == 1)).any()
    assert r["nD"] >= 64
