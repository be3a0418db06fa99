"""The staged encoder's listed rows (bic_fused.hip: k_row_walk, k_emit_rest, the two k_scan_rows launches) at
list lengths no small test reaches: lists longer than a kernel's grid (a workgroup takes a second row), lists
of one entry and of exactly the grid's size (every other workgroup, or none, finds the list ended), the
plane's first 1 in the last row of the last plane (no next row to take the 1-count from), and several
scan chunks of one-strip rows. Row 0 of every plane is always walked, so a batch of many one-row planes makes
a long list from little data. Every case goes, with the staged encoder forced, through encode_planes with the
Golomb coder and with the EG coder (k_emit_rest's Golomb-only and EG-only instances) and through encode_planes2
(both streams in one pass), without and with prediction, and is compared with the oracle's streams; the
premises a case relies on are computed on the CPU and asserted."""
import numpy as np
import pytest

from pybic import CODER_EG, CODER_GOLOMB, as_u64

pytestmark = pytest.mark.gpu

WALK_WAVES = 8192  # k_row_walk's grid in waves, half a residual word per lane


@pytest.fixture
def staged(ctx):
    ctx.set_encoder("staged")
    yield ctx
    ctx.set_encoder("auto")


def walk_grid(cols):
    used = (cols + 63) // 64
    return WALK_WAVES // ((2 * used + 63) // 64)


def rest_grid(ctx, cols):
    cus = ctx.torch.cuda.get_device_properties(ctx.device).multi_processor_count
    used = (cols + 63) // 64
    return cus * 32 // ((used + 63) // 64)


def row_ks(words, cols):
    """The k of every Golomb codeword of a one-row plane without prediction, by the oracle's rule: k = 1 for the
    fresh state, else the smallest k with n << k >= A (n samples coded so far, A their sum). The samples are
    the zeros before each 1 and, at the end of the row, cols - 1 - (the last 1's column)."""
    bits = np.unpackbits(words.astype(">u8").view(np.uint8))[:cols]
    pos = np.flatnonzero(bits).astype(np.int64)
    prev = np.concatenate(([-1], pos))
    s = np.concatenate((pos - prev[:-1] - 1, [cols - 1 - prev[-1]]))
    n = np.arange(len(s), dtype=np.int64)
    A = np.concatenate(([0], np.cumsum(s)[:-1]))
    k = np.ones(len(s), np.int64)
    q = (A[1:] + n[1:] - 1) // n[1:]  # ceil(A / n): the smallest k has 2^k >= q
    k[1:] = np.where(q > 1, np.floor(np.log2(np.maximum(q - 1, 1))).astype(np.int64) + 1, 0)
    return k


def mixed_rows(oracle, P, cols, pred):
    """one-row planes whose codewords (of the med residual with pred) are neither all k = 0 nor all k = 1"""
    m = 0
    for plane in P:
        k = row_ks(oracle.med(plane, cols)[0] if pred else plane[0], cols)
        m += int(not (k == 0).all() and not (k == 1).all())
    return m


def test_row_ks_is_the_oracles_rule(oracle):
    """row_ks against the oracle's coder: the row's Golomb length is the sum of k + (s >> k) + 1"""
    cols = 1000
    for seed, p in ((1, 0.5), (2, 0.1), (3, 0.9)):
        P = oracle.gen_plane(seed, p, 1, cols)
        k = row_ks(P[0], cols)
        bits = np.unpackbits(P[0].astype(">u8").view(np.uint8))[:cols]
        pos = np.flatnonzero(bits).astype(np.int64)
        prev = np.concatenate(([-1], pos))
        s = np.concatenate((pos - prev[:-1] - 1, [cols - 1 - prev[-1]]))
        assert int((k + (s >> k) + 1).sum()) == oracle.encode_plane(P, cols, 0, 0)[0]


PREDS = (0, 1)


def check(ctx, oracle, P, cols, preds=PREDS):
    """encode_planes with each coder and encode_planes2, each against the oracle's streams (computed once)"""
    P = np.ascontiguousarray(P)
    d = ctx.to_dev(P)
    for pred in preds:
        ref = {coder: [oracle.encode_plane(P[k], cols, pred, coder)[:2] for k in range(P.shape[0])] for coder in (0, 1)}
        og, bg = ctx.encode_planes(d, cols, pred, CODER_GOLOMB)
        oe, be = ctx.encode_planes(d, cols, pred, CODER_EG)
        (og2, bg2), (oe2, be2) = ctx.encode_planes2(d, cols, pred)
        ctx.sync()
        for what, coder, out, bits in (("planes", 0, og, bg), ("planes", 1, oe, be), ("planes2", 0, og2, bg2),
                                       ("planes2", 1, oe2, be2)):
            words, nbits = as_u64(out), as_u64(bits)
            for k, (eb, est) in enumerate(ref[coder]):
                assert int(nbits[k]) == eb, (what, pred, coder, k)
                assert words[k, :(eb + 63) // 64].tobytes() == est.tobytes(), (what, pred, coder, k)


def one_row_planes(oracle, seed, n, cols):
    return oracle.gen_plane(seed, 0.5, n, cols)[:, None, :]  # n planes of one Bernoulli(0.5) row


@pytest.mark.parametrize("cols", [16384, 4096])
def test_emit_rest_takes_a_second_row(staged, oracle, cols):
    """more mixed-k rows than k_emit_rest has workgroups"""
    grid = rest_grid(staged, cols)
    P = one_row_planes(oracle, 11 + cols, grid + 50, cols)
    for pred in PREDS:
        assert mixed_rows(oracle, P, cols, pred) > grid
    check(staged, oracle, P, cols)


@pytest.mark.parametrize("cols,n", [(16384, 1100), (4096, 4096 + 40)])
def test_row_walk_takes_a_second_row(staged, oracle, cols, n):
    """more walked rows (row 0 of every plane) than k_row_walk has workgroups"""
    assert n > walk_grid(cols)
    P = one_row_planes(oracle, 23 + cols, n, cols)
    check(staged, oracle, P, cols)


def test_list_of_one_entry(staged, oracle):
    """one plane of one row: a list of one entry, for every workgroup but the first the list has ended"""
    for cols in (16384, 4096, 100):
        P = one_row_planes(oracle, 5 + cols, 1, cols)
        for pred in PREDS:
            assert mixed_rows(oracle, P, cols, pred) == 1
        check(staged, oracle, P, cols)


def test_list_of_exactly_the_grid(staged, oracle):
    cols = 16384
    grid = rest_grid(staged, cols)
    """as many walked rows (row 0 of every plane) as k_emit_rest has workgroups: the list's last entry is the last
    workgroup's. About one Bernoulli(0.5) row in a thousand codes with k = 1 throughout and is skipped; the rest
    are emitted"""
    P = one_row_planes(oracle, 34, grid, cols)
    assert P.shape[0] == grid
    for pred in PREDS:
        assert mixed_rows(oracle, P, cols, pred) >= grid - grid // 100
    check(staged, oracle, P, cols)


@pytest.mark.parametrize("nplanes", [1, 3])
@pytest.mark.parametrize("rows,cols", [(40, 1000), (9, 16384)])
def test_first_one_in_the_last_row_of_the_last_plane(staged, oracle, nplanes, rows, cols):
    """the first-1 test of the last row reads the plane's total, not the 1-count of a row past the plane"""
    P = np.stack([oracle.gen_plane(41 + k, 0.3, rows, cols) for k in range(nplanes)])
    P[-1, :-1] = 0
    assert P[-1, -1].any() and not P[-1, :-1].any()
    check(staged, oracle, P, cols)


def test_scans_over_several_chunks_of_one_strip_rows(staged, oracle):
    """three planes of 3000 rows of 64 columns: both scans cross chunk boundaries with one strip per row"""
    rows, cols = 3000, 64
    P = np.stack([oracle.gen_plane(51 + k, p, rows, cols) for k, p in enumerate((0.5, 0.05, 0.3))])
    assert rows > 2 * 1024  # more than two chunks at either chunk size the scan has used
    check(staged, oracle, P, cols)
