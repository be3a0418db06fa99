"""Pins tests/bsvd_init_ref.py, the restatement of the reference's model initialisers (bsvd.cpp:99-267) that the
device is compared with: its generator against libc's rand48 family and against libbic.so's two host-only entries,
the four rules on literals small enough to verify on paper, and the padding convention. CPU only."""
import ctypes
import functools

import numpy as np
import pytest

import bsvd_init_ref as I
import pybic
from bsvd_ref import words
from test_bsvd_prox_ref import bits

SEED = 20  # of the clustered input (I.clustered)
# (n, m, p): one word, ragged p; whole words; three words with the last masked, p past one word; past the 31-row
# flush and several workgroups per atom; the widest m; the most atoms of these; one atom; one bit
SHAPES = [(300, 64, 33), (257, 256, 64), (130, 320, 100), (2500, 130, 40), (64, 4096, 65), (1025, 100, 512),
          (65, 65, 1), (1, 1, 1)]


# ---- the generator ----
def libc_outputs(seed, count):
    libc = ctypes.CDLL(None)
    libc.mrand48.restype = ctypes.c_long
    if seed:
        libc.srand48.argtypes = [ctypes.c_long]
        libc.srand48(seed)
    else:  # gsl_rng_set(0): x0 = 0x330E, x1 = 0xABCD, x2 = 0x1234
        libc.seed48.restype = ctypes.c_void_p
        libc.seed48((ctypes.c_ushort * 3)(0x330E, 0xABCD, 0x1234))
    return [libc.mrand48() & 0xFFFFFFFF for _ in range(count)]


@pytest.mark.parametrize("seed", [I.RANDOM_SEED, 1, 0])
def test_generator_is_libc_rand48(seed):
    r = I.Rand48(seed)
    assert [r.get() for _ in range(2000)] == libc_outputs(seed, 2000)


def test_seed_uses_the_low_32_bits():
    assert I.Rand48(34503498).state == (34503498 << 16) | 0x330E
    assert I.Rand48(0).state == 0x1234ABCD330E == I.Rand48(1 << 32).state
    assert I.Rand48((7 << 32) | 5).state == I.Rand48(5).state


@pytest.mark.parametrize("seed", [I.RANDOM_SEED, 0])
@pytest.mark.parametrize("bound", [512, 65536, 1610612736])
def test_library_generator_is_the_restatement(seed, bound):
    """bic_bsvd_rng_seed / bic_bsvd_rng_uniform: the values and, since rejected outputs are used up, the state
    after each call. The last bound has scale 2 and rejects a quarter of the outputs."""
    r = I.Rand48(seed)
    state = pybic.bsvd_rng_seed(seed)
    assert state == r.state
    for count in (1, 0, 3999):
        got, state = pybic.bsvd_rng_uniform(state, bound, count)
        assert np.array_equal(got, r.uniform(bound, count)) and state == r.state, count
    if bound == 1610612736:
        assert 1.2 * 4000 < r.outputs < 1.5 * 4000  # 4 / 3 outputs per value
    else:
        assert r.outputs < 1.01 * 4000 + 4


# ---- the rules on literals (m = 4 unless said; bits left to right) ----
def atoms(D, m=4):
    return ["".join(str(b) for b in row[:m]) for row in D]


def test_neighbor_pick_that_meets_no_other_row_gives_all_ones():
    st = {}
    D, A = I.initialize_neighbor(bits(["1000", "0110", "0011"]), 4, 1, picks=[0], stats=st)
    assert atoms(D) == ["1111"] and st["u1"] == 1 and not D[:, 4:].any() and not A.any()  # u = 1: 0 >= 0 everywhere


def test_neighbor_u3_returns_the_pick():
    st = {}
    D, _ = I.initialize_neighbor(bits(["1100", "1000", "0100", "0011"]), 4, 1, picks=[0], stats=st)
    assert atoms(D) == ["1100"] and st["max_u"] == 3  # u / 2 = 1: every bit of the pick has its own count


def test_neighbor_u4_drops_a_bit_only_the_pick_has():
    st = {}
    D, _ = I.initialize_neighbor(bits(["1110", "1000", "1000", "1000"]), 4, 1, picks=[0], stats=st)
    assert atoms(D) == ["1000"] and st["max_u"] == 4 and st["ties"] == 0  # counts 4 1 1 0, u / 2 = 2


def test_neighbor_u4_keeps_a_bit_two_of_four_have():
    st = {}
    D, _ = I.initialize_neighbor(bits(["1100", "1100", "1000", "1000"]), 4, 1, picks=[0], stats=st)
    assert atoms(D) == ["1100"] and st["max_u"] == 4 and st["ties"] == 1  # counts 4 2 0 0: 2 >= 2


def test_neighbor_same_row_twice_and_explicit_zero_or_absent_pick():
    D, _ = I.initialize_neighbor(bits(["1100", "0000", "0110"]), 4, 4, picks=[2, 1, 2, 3])
    assert atoms(D) == ["0110", "0000", "0110", "0000"]  # u = 2; a zero pick and a pick past n leave zero atoms


def test_neighbor_zero_row_is_drawn_again_and_uses_up_a_draw():
    E = bits(["0000", "1010"])
    seed = next(s for s in range(1, 64) if I.Rand48(s).uniform_int(2) == 0)  # starts on the zero row
    draws = I.Rand48(seed).uniform(2, 64)
    first = int(np.flatnonzero(draws == 1)[0])
    assert first >= 1
    r, st = I.Rand48(seed), {}
    D, _ = I.initialize_neighbor(E, 4, 1, rng=r, stats=st)
    after = I.Rand48(seed)
    after.uniform(2, first + 1)
    assert atoms(D) == ["1111"] and st["redraws"] == first and r.outputs == first + 1 and r.state == after.state
    assert st["picks"] == [1]


def test_partition_samples_the_ranking_but_not_the_centroid():
    """m = 65 (two words per row), n = 6: col_weight sees rows 0 .. 2. Column 5 has sampled weight 1 (full 2),
    column 9 sampled 0 (full 3): the pivot is column 5, its members rows 0 and 3 -- of ALL rows -- so u = 2 and
    the atom is their union {5, 9}. (Full weights would rank column 9 first: {5, 9, 64}; a sampled centroid
    would be {5}.) The second pivot is the lowest column of sampled weight 0, column 0, which no row has: u = 0."""
    E = np.zeros((6, 128), np.uint8)
    for i, cols in enumerate([[5], [], [], [5, 9], [9, 64], [9]]):
        E[i, cols] = 1
    assert [I.col_weight(E, 65, c) for c in (5, 9, 64)] == [1, 0, 0]
    st = {}
    D, A = I.initialize_partition(E, 65, 2, stats=st)
    assert st["pivots"] == [5, 0] and st["sampled_differs"] == 3 and st["zero_pivots"] == 1
    assert list(np.flatnonzero(D[0])) == [5, 9]
    assert D[1, :65].all() and not D[1, 65:].any() and not A.any()


def test_partition_ties_zero_pivot_and_atoms_past_m():
    st = {}
    D, _ = I.initialize_partition(bits(["0110", "0110"]), 4, 6, stats=st)
    assert st["pivots"] == [1, 2, 0, 3] and st["rank_ties"] == 2  # equal weights: the lower column first
    # an all-zero pivot column (0, then 3): all ones; atoms k >= m: zero
    assert atoms(D) == ["0110", "0110", "1111", "1111", "0000", "0000"]


def test_counting_sort_reverses_ties():
    s = [(2, 0), (0, 1), (2, 2), (1, 3), (0, 4)]
    I.counting_sort(s)
    assert s == [(0, 4), (0, 1), (1, 3), (2, 2), (2, 0)]


def test_centroids_tie_sets_the_bit_and_an_empty_atom_is_all_ones():
    st = {}
    D, A = I.initialize_centroids(bits(["1100", "0100"]), 4, 2, assign=[0, 0], stats=st)
    assert atoms(D) == ["1100", "1111"] and st["ties"] == 1 and st["empty"] == 1  # counts 1 2 0 0 of u = 2
    assert A[:, :2].tolist() == [[1, 0], [1, 0]] and not A[:, 2:].any() and not D[:, 4:].any()


def test_centroids_xor_is_the_parity_and_an_empty_atom_is_zero():
    D, A = I.initialize_centroids(bits(["1100", "0100", "0110", "0001"]), 4, 3, assign=[0, 0, 0, 2], xor=True)
    assert atoms(D) == ["1110", "0000", "0001"]
    assert A[:, :3].tolist() == [[1, 0, 0], [1, 0, 0], [1, 0, 0], [0, 0, 1]]


def test_centroids_assignment_past_p_is_skipped():
    D, A = I.initialize_centroids(bits(["1100", "0011"]), 4, 1, assign=[1, 0])
    assert atoms(D) == ["0011"] and A[:, 0].tolist() == [0, 1]


# ---- the cases the device is compared on ----
@functools.lru_cache(maxsize=None)
def case(n, m, p, seed=SEED):
    """the clustered input and, per rule, the restatement's D, A, stats and generator state from random_seed;
    computed once, never modified"""
    E, lonely = I.clustered(seed, n, m)
    out = {"E": E, "lonely": lonely}
    for mi in (I.NEIGHBOR, I.PARTITION, I.CENTROIDS, I.CENTROIDS_XOR):
        r, st = I.Rand48(), {}
        D, A = I.initialize(mi, E, m, p, r, st)
        for a in (D, A):
            a.setflags(write=False)
        out[mi] = dict(D=D, A=A, st=st, state=r.state)
    E.setflags(write=False)
    return out


def nonvacuous():
    """what the clustered cases exercise (asserted here and again by the GPU tests before they compare)"""
    c = {s: case(*s) for s in SHAPES}
    assert sum(c[s][I.NEIGHBOR]["st"]["redraws"] >= 1 for s in SHAPES) >= 5  # a zero row was drawn
    for s in SHAPES[:6]:
        assert c[s][I.NEIGHBOR]["D"].sum() >= 300, s           # the atoms are not trivial
    assert sum(c[s][I.NEIGHBOR]["st"]["u1"] for s in SHAPES) >= 4
    assert sum(c[s][I.NEIGHBOR]["st"]["ties"] for s in SHAPES) >= 1
    assert max(c[s][I.NEIGHBOR]["st"]["max_u"] for s in SHAPES) > 31  # past one carry-save flush
    for s in SHAPES:
        pt = c[s][I.PARTITION]["st"]
        assert (pt["sampled_differs"] > 0) == (s[1] > 64 and s[0] > 1), s
    assert sum(c[s][I.PARTITION]["st"]["rank_ties"] for s in SHAPES) >= 1
    assert sum(c[s][I.PARTITION]["st"]["small_pivots"] for s in SHAPES) >= 1
    assert sum(c[s][I.CENTROIDS]["st"]["empty"] > 0 for s in SHAPES) >= 3
    assert sum(c[s][I.CENTROIDS]["st"]["ties"] > 0 for s in SHAPES) >= 4
    assert c[(2500, 130, 40)][I.CENTROIDS]["st"]["max_u"] > 31
    return c


def test_cases_exercise_the_rules():
    nonvacuous()


@pytest.mark.parametrize("n,m,p", [(1025, 100, 512), (65, 65, 1)])
def test_dirty_padding_changes_nothing_and_outputs_are_clean(n, m, p):
    c = case(n, m, p)
    E = c["E"].copy()
    assert E[:, m:].all() and E.shape[1] > m
    E[:, m:] = 0
    for mi in (I.NEIGHBOR, I.PARTITION, I.CENTROIDS, I.CENTROIDS_XOR):
        D, A = I.initialize(mi, E, m, p, I.Rand48())
        assert np.array_equal(D, c[mi]["D"]) and np.array_equal(A, c[mi]["A"]), mi
        assert not D[:, m:].any() and not A[:, p:].any(), mi
        assert D.shape == (p, 64 * words(m)) and A.shape == (n, 64 * words(p))
