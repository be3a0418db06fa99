"""Seeded, structured bit planes for the device decoders' lane paths ("Decoder path coverage").

Every generator returns (P[n, rows, wpr] uint64, cols) with zero pad bits, built with numpy from the
oracle's own generators (gen_plane / gen_bytes), so that any machine regenerates the same planes. Which
path of k_dec_golomb_nib / k_dec_egad / k_dec_eg_rows a row takes is decided by the coder's running state;
tests/decoder_census.py counts which of them these inputs reach, tests/test_gpu_decode_paths.py decodes
them on the device.

PATH_INPUTS: name -> (family, maker); rows <= 192, cols <= 4096 and n <= 4, but for one 16384-column input
(the EG row kernel's four words per lane). TALL_INPUTS: more than 16384 rows, for the column scan's second
and third rounds of 256 chunks."""
import numpy as np

from oracle_lib import pack_rows


def _uniform(oracle, seed, n):
    """n seeded uniforms in [0, 1) out of gen_bytes"""
    return oracle.gen_bytes(seed, 4 * n).view("<u4").astype(np.float64) / 4294967296.0


def _bern(oracle, seed, rows, cols, p):
    """bool [rows, cols], pixel (i, j) set with probability p (a scalar or an array that broadcasts)"""
    return _uniform(oracle, seed, rows * cols).reshape(rows, cols) < p


def _ints(oracle, seed, n, lo, hi):
    """n seeded integers in [lo, hi)"""
    return lo + (_uniform(oracle, seed, n) * (hi - lo)).astype(np.int64)


def _stack(bits_list, cols):
    return np.stack([pack_rows(b) for b in bits_list]), cols


# ---- the families ------------------------------------------------------------------------------------
def dense_then_sparse(oracle, seed, n, rows, cols, split, p_hi=0.5, p_lo=0.004):
    """rows [0, split) at p_hi, the rest at p_lo: k rises from <= 1 to >= 2 inside one plane"""
    p = np.where(np.arange(rows)[:, None] < split, p_hi, p_lo)
    return _stack([_bern(oracle, seed + 101 * k, rows, cols, p) for k in range(n)], cols)


def sparse_then_dense(oracle, seed, n, rows, cols, split, p_lo=0.004, p_hi=0.5):
    """rows [0, split) at p_lo, the rest at p_hi: k from >= 2 down to <= 1 (slow lanes beside table lanes)"""
    p = np.where(np.arange(rows)[:, None] < split, p_lo, p_hi)
    return _stack([_bern(oracle, seed + 101 * k, rows, cols, p) for k in range(n)], cols)


def density_step_col(oracle, seed, n, rows, cols, split, p_left=0.5, p_right=0.004):
    """the density step inside every row, at column `split`"""
    p = np.where(np.arange(cols)[None, :] < split, p_left, p_right)
    return _stack([_bern(oracle, seed + 101 * k, rows, cols, p) for k in range(n)], cols)


def density_ramp(oracle, seed, n, rows, cols, p0=0.6, p1=0.0005):
    """the density falls geometrically from p0 in row 0 to p1 in the last row (every k on the way)"""
    t = np.arange(rows) / max(1, rows - 1)
    p = (p0 * (p1 / p0) ** t)[:, None]
    out = []
    for k in range(n):
        b = _bern(oracle, seed + 101 * k, rows, cols, p)
        out.append(b if k % 2 == 0 else b[::-1].copy())  # odd planes ramp upwards
    return _stack(out, cols)


def gaps(oracle, seed, n, rows, cols, p=0.6):
    """p = 0.6 with zero gaps of 60-200 columns at random places, and in every fourth row gaps that
    start or end on columns 63, 64 and 65 of a word"""
    out = []
    for k in range(n):
        s = seed + 101 * k
        b = _bern(oracle, s, rows, cols, p)
        per = 3
        start = _ints(oracle, s + 1, rows * per, 0, max(1, cols - 60))
        length = _ints(oracle, s + 2, rows * per, 60, 201)
        edge = _ints(oracle, s + 3, rows, 0, 6)
        word = _ints(oracle, s + 4, rows, 1, max(2, cols // 64))
        for i in range(rows):
            for q in range(per):
                a = int(start[i * per + q])
                b[i, a:a + int(length[i * per + q])] = False
            if i % 4 == 0 and cols >= 320:
                e = 64 * int(word[i]) + (63, 64, 65)[int(edge[i]) % 3] - 64  # column 63, 64 or 65 of a word
                if edge[i] < 3:
                    b[i, e:e + 100] = False  # a gap that starts there
                    if e > 0:
                        b[i, e - 1] = True
                else:
                    b[i, max(0, e - 100):e] = False  # a gap that ends there
                    if e < cols:
                        b[i, e] = True
        out.append(b)
    return _stack(out, cols)


def alternating(oracle, seed, n, rows, cols, flip=0.02):
    """every other column, 2 % of the pixels flipped: the Golomb state sits at |x| <= 5, where k flips
    between codewords inside one table byte"""
    base = (np.arange(cols)[None, :] & 1).astype(bool)
    return _stack([base ^ _bern(oracle, seed + 101 * k, rows, cols, flip) for k in range(n)], cols)


def first_row_run(oracle, seeds, cols=256):
    """one-row planes gen_plane(seed, 0.5, 1, cols): the first row starts from a fresh coder and reads
    its first bytes bit by bit; in these the last such byte ends inside a zero run that has crossed a
    64-column word (the seeds found with tests/decoder_census.py)"""
    return np.stack([oracle.gen_plane(s, 0.5, 1, cols) for s in seeds]), cols


def all_zero(n, rows, cols):
    return np.zeros((n, rows, (cols + 63) // 64), np.uint64), cols


def all_one(n, rows, cols):
    return _stack([np.ones((rows, cols), bool) for _ in range(n)], cols)


def single_one(rows, cols, places):
    """one plane per (r, c): a single 1 there (negative r, c count from the end)"""
    out = []
    for r, c in places:
        b = np.zeros((rows, cols), bool)
        b[r % rows, c % cols] = True
        out.append(b)
    return _stack(out, cols)


def mixed_wave(oracle, seed, rows, cols, ps=(0.5, 0.003, 0.9)):
    """n = 3 planes of 40 or 48 rows: a wave of 64 consecutive plane * rows + row ids holds a dense
    plane's rows beside a sparse plane's"""
    return _stack([_bern(oracle, seed + 101 * k, rows, cols, ps[k]) for k in range(len(ps))], cols)


def widths(oracle, seed, rows, cols, ps=(0.5, 0.05, 0.93)):
    """i.i.d. planes at a width that the j + 16 <= cols / col + 40 <= cols guards and the trail word see"""
    return _stack([_bern(oracle, seed + 101 * k + cols, rows, cols, ps[k]) for k in range(len(ps))], cols)


def tail_across_block(oracle, seed, rows, cols, p=0.9):
    """a dense plane (k = 0: one stream bit per column) followed by an all-zero one, 96 rows each and
    cols in [256, 263]: the middle wave holds the dense plane's last rows beside the sparse plane's first,
    so its first block of 32 bytes is stepped; the dense rows' last step there is past the j + 16 <= cols
    guard and goes bit by bit across column 256, and the sparse rows end inside the block -- the next block
    is the all-lanes one, entered with open words behind j (bic_decode.hip:592), and the dense rows'
    last byte is its first (stop == 0)"""
    return _stack([_bern(oracle, seed, rows, cols, p), np.zeros((rows, cols), bool)], cols)


def ones_tail_k1(oracle, seed, rows=96, zeros=256, cols=456, p=0.1):
    """Rows of `zeros` 0s and then 1s to the end, coded at k = 1 (A / n = 256 / 201): 2 + zeros / 2 stream
    bits for the run and "01" per 1, so the row's byte 63 -- the last step of its second block of 32 -- holds
    the 1s on columns 444 .. 447. That step is past the j + 16 <= cols guard, goes bit by bit and leaves j on
    column 448, a word ahead of ow, with 18 stream bits to go: the next block's stop is 2. A sparse plane
    follows (rows of 257 .. 512 stream bits: lanes that are never block-able and end in the second block), so
    the wave of the first plane's last rows and the second's first steps through its second block and takes
    the all-lanes path for the third, entered stale by lanes that place columns in it (bic_decode.hip:592).
    Planes 2 and 3 have planes 0 and 1 as their residuals (predict = 1)."""
    a = np.zeros((rows, cols), bool)
    a[:, zeros:] = True
    s = _bern(oracle, seed, rows, cols, p)
    return _stack([a, s, as_residual(a), as_residual(s)], cols)


def as_residual(bits):
    """the plane whose med residual is `bits` (but for R(0, 0), which med never writes): the prefix XOR
    along the rows and down the columns"""
    return np.logical_xor.accumulate(np.logical_xor.accumulate(bits, axis=1), axis=0)


def burst_to_word_end(rows, cols, target=20):
    """Rows built against the Golomb coder's state v = 2 n - A (n samples, A zeros so far; the table steps
    need v >= 16, k >= 2 is v < 0): zeros until v is well below 0, then a burst of 1s that ends on column
    62 or 63 of a word with v = target +- 1, then 001 001 ... (v level). The burst's last byte is read bit by
    bit (it started below 16) and leaves j in the next word -- by the 1 on column 63, or by the two zeros
    after column 62 -- and the next byte is a table step: a stale entry (bic_decode.hip:530) in a later row,
    after k >= 2 codewords. Plane 0 has these rows as its pixels (predict = 0), plane 1 as its residual."""
    b = np.zeros((rows, cols), bool)
    ones = 0
    for r in range(rows):
        v0 = 3 * ones + 2 * r - r * cols
        e = 62 + (r & 1) + 64 * (1 + r % ((cols - 40) // 64 - 1))
        s = next(q // 3 for q in (v0 + 2 * (e + 1) - t for t in (target, target + 1, target - 1)) if q % 3 == 0)
        assert 0 < s < e - 8, (r, v0, e, s)
        b[r, s:e + 1] = True
        b[r, e + 3::3] = True
        ones += int(b[r].sum())
    return _stack([b, as_residual(b)], cols)


def eg_first(oracle, seed, rows, cols, places, p=0.5):
    """i.i.d. planes cleared before (r, c), which is set: the plane's first 1 (without prediction) sits
    there, and the rows after it are ordinary"""
    out = []
    for k, (r, c) in enumerate(places):
        r, c = r % rows, c % cols
        b = _bern(oracle, seed + 101 * k, rows, cols, p)
        b[:r] = False
        b[r, :c] = False
        b[r, c] = True
        out.append(b)
    return _stack(out, cols)


def tall(oracle, seed, rows, cols):
    """n = 2, p = 0.5: more than 16384 rows (k_col_scan_par's carry across rounds of 256 chunks)"""
    return np.stack([oracle.gen_plane(seed + 7 * k + rows + cols, 0.5, rows, cols) for k in range(2)]), cols


# ---- the committed input set ---------------------------------------------------------------------------
FIRST_ROW_SEEDS = (105, 111, 590)  # tests/test_gpu_pbm.py::test_round_trip_first_row_run_across_word's
FIRST_ROW_SEEDS_MORE = (210, 342, 551, 657)  # found with the census, as were (789, 792, 832)
WIDTHS = (1, 15, 16, 17, 31, 33, 63, 64, 65, 127, 128, 129, 1000, 1024, 4096)
_EDGE_COLS = (0, 1, 62, 63, 64, 65, -2, -1)


def _path_inputs():
    I = {}

    def add(name, family, fn):
        assert name not in I
        I[name] = (family, fn)

    add("dense_then_sparse-128x2048", "dense_then_sparse", lambda o: dense_then_sparse(o, 0xD5, 1, 128, 2048, 64))
    add("dense_then_sparse-70x1000", "dense_then_sparse", lambda o: dense_then_sparse(o, 0xD6, 2, 70, 1000, 23, 0.5, 0.02))
    add("sparse_then_dense-64x1024", "sparse_then_dense", lambda o: sparse_then_dense(o, 0x5D, 1, 64, 1024, 16))
    add("sparse_then_dense-100x520", "sparse_then_dense", lambda o: sparse_then_dense(o, 0x5E, 2, 100, 520, 37, 0.01, 0.35))
    add("density_step_col-64x1024", "density_step_col", lambda o: density_step_col(o, 0xDC, 2, 64, 1024, 500))
    add("density_step_col-33x700", "density_step_col", lambda o: density_step_col(o, 0xDD, 2, 33, 700, 193, 0.003, 0.5))
    add("density_ramp-192x512", "density_ramp", lambda o: density_ramp(o, 0xDA, 2, 192, 512))
    add("density_ramp-96x4096", "density_ramp", lambda o: density_ramp(o, 0xDB, 1, 96, 4096, 0.5, 0.0002))
    add("gaps-64x2048", "gaps", lambda o: gaps(o, 0x6A, 2, 64, 2048))
    add("gaps-45x333", "gaps", lambda o: gaps(o, 0x6B, 2, 45, 333))
    add("alternating-128x2048", "alternating", lambda o: alternating(o, 0xA1, 1, 128, 2048))
    add("alternating-70x255", "alternating", lambda o: alternating(o, 0xA2, 3, 70, 255))
    add("first_row_run-known", "first_row_run", lambda o: first_row_run(o, FIRST_ROW_SEEDS))
    add("first_row_run-more", "first_row_run", lambda o: first_row_run(o, FIRST_ROW_SEEDS_MORE))
    add("first_row_run-1000", "first_row_run", lambda o: first_row_run(o, (789, 792, 832), 1000))
    add("all_zero-64x1000", "all_zero", lambda o: all_zero(2, 64, 1000))
    add("all_zero-5x70", "all_zero", lambda o: all_zero(1, 5, 70))
    add("all_one-64x260", "all_one", lambda o: all_one(2, 64, 260))
    add("all_one-7x1000", "all_one", lambda o: all_one(1, 7, 1000))
    for c in _EDGE_COLS:  # one call: the 1 in row 0, row 1 and the last row (the EG decoder's first rows differ)
        add(f"single_one-c{c}", "single_one", lambda o, c=c: single_one(5, 130, [(0, c), (1, c), (-1, c)]))
    add("mixed_wave-40x1024", "mixed_wave", lambda o: mixed_wave(o, 0x3A, 40, 1024))
    add("mixed_wave-48x300", "mixed_wave", lambda o: mixed_wave(o, 0x3B, 48, 300, (0.002, 0.5, 0.03)))
    for c in WIDTHS:
        rows = 12 if c > 129 else 20
        add(f"widths-{c}", "widths", lambda o, c=c, rows=rows: widths(o, 0x1D, rows, c))
    add("tail_across_block-96x260", "tail_across_block", lambda o: tail_across_block(o, 0x7A, 96, 260))
    add("tail_across_block-96x519", "tail_across_block", lambda o: tail_across_block(o, 0x7B, 96, 519, 0.95))
    add("ones_tail_k1-96x456", "ones_tail_k1", lambda o: ones_tail_k1(o, 0x0E))
    add("burst_to_word_end-40x520", "burst_to_word_end", lambda o: burst_to_word_end(40, 520))
    add("burst_to_word_end-70x300", "burst_to_word_end", lambda o: burst_to_word_end(70, 300))
    add("eg_first-9x200", "eg_first", lambda o: eg_first(o, 0xE6, 9, 200, [(4, 62), (4, 63), (8, 64), (0, -1)]))
    add("eg_first-6x16384", "eg_first", lambda o: eg_first(o, 0xE7, 6, 16384, [(3, 4095), (5, 8192), (0, -1), (5, -1)]))
    return I


PATH_INPUTS = _path_inputs()
TALL_INPUTS = {f"tall-{r}x{c}": (lambda o, r=r, c=c: tall(o, 0x7A11, r, c))
               for r in (16385, 16448, 33000) for c in (1, 64, 65)}

_CACHE = {}


def get(oracle, name):
    """(P, cols) of a named input, made once and read-only"""
    if name not in _CACHE:
        fn = PATH_INPUTS[name][1] if name in PATH_INPUTS else TALL_INPUTS[name]
        P, cols = fn(oracle)
        P = np.ascontiguousarray(P, np.uint64)
        assert P.shape[2] == (cols + 63) // 64
        if cols % 64:  # zero pad bits
            assert not (P[:, :, -1] & np.uint64((1 << (64 - cols % 64)) - 1)).any()
        P.setflags(write=False)
        _CACHE[name] = (P, cols)
    return _CACHE[name]


def family(name):
    return PATH_INPUTS[name][0] if name in PATH_INPUTS else "tall"
