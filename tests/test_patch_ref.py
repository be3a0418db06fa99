"""tests/patch_ref.py, the restatement of the driver's image mode, is pinned on the CPU: (a) every tile of the
gather is get_submatrix's rows as the oracle (and, where built, the reference) gives them; (b) the host
binary_matrix of this build, running the driver's two loops and render_mosaic (tests/cpp/patch_host_check.cpp,
compiled without device code), gives the same samples word for word, the same valid pixels and the same mosaic
file; (c) hand-worked literals."""
import os
import subprocess

import numpy as np
import pytest

import patch_ref as P
from conftest import PKG, ROOT
from oracle_lib import Ref, have_ref
from pnm_io import plane_to_p4_rows, read_pbm_bytes

GEOMS = [(37, 70, 5), (37, 126, 5), (64, 128, 16), (40, 130, 63), (130, 200, 64), (9, 9, 1), (33, 65, 8), (50, 190, 24),
         (17, 64, 3), (20, 100, 7), (64, 64, 64), (70, 4100, 16), (70, 200, 65), (130, 300, 100), (128, 256, 128),
         (200, 330, 130)]
MOSAICS = [(1, 1), (5, 25), (7, 70), (512, 256), (10, 64), (3, 4500), (17, 4096), (2, 3), (100, 49), (65, 9)]
WHITE = (9, 10, 11, 12, 13, 32)


def random_plane(seed, rows, cols, pitch=0, dirty=True):
    """random words, a first raster byte that read_pbm_header's pattern does not swallow (pbm.cpp:19), pad bits
    and `pitch` extra words per row random (dirty) or zero"""
    rng = np.random.default_rng(seed)
    used = P.words(cols)
    I = rng.integers(0, 1 << 64, (rows, used + pitch), dtype=np.uint64)
    I[0, 0] = (I[0, 0] & np.uint64((1 << 56) - 1)) | np.uint64(0xA5 << 56)
    if not dirty and cols % 64:
        I[:, used - 1] &= np.uint64(~((1 << (64 - cols % 64)) - 1) & ((1 << 64) - 1))
    return I


def pbm_file(path, words, cols):
    """a P4 file of the plane, its first raster byte not white space"""
    raster = plane_to_p4_rows(words, cols)
    assert int(raster[0, 0]) not in WHITE
    with open(path, "wb") as f:
        f.write(f"P4\n{cols} {words.shape[0]}\n".encode())
        f.write(raster.tobytes())
    return str(path)


def valid(words, cols):
    return P.unpack(words, P.words(cols))[:, :cols]


# ---- (a) the oracle's and the reference's get_submatrix ---------------------------------------------------------

@pytest.mark.parametrize("rows,cols,W", [(37, 126, 5), (17, 64, 3), (40, 130, 63), (70, 200, 65)])
def test_gather_is_get_submatrix_per_tile(oracle, rows, cols, W):
    I = random_plane(rows * 1000 + cols, rows, cols)
    st = {}
    X = P.unpack(P.gather(I, cols, W, st), P.words(W * W))
    if cols % 64:
        assert st["pad_ones"] > 0  # the tiles that cover pad columns read what is stored there
    if (rows, cols, W) in ((37, 126, 5), (17, 64, 3)):
        assert st["wrap_ones"] > 0  # SURVEY.md section 4 hazard 3: the right-edge tile reads the next row
    assert not X[:, W * W:].any()
    # the reference's objects take the plane pixel by pixel (oracle/ref_capi.cpp from_words), so they see clean
    # padding: they pin the same image with its pad bits cleared, the wrap included
    clean = P.pack(P.unpack(I, P.words(cols))[:, :cols])
    Xc = P.unpack(P.gather(clean, cols, W, st), P.words(W * W))
    if (rows, cols, W) in ((37, 126, 5), (17, 64, 3)):
        assert st["wrap_ones"] > 0 and st["pad_ones"] == 0
    sources = [(oracle, I, X), (oracle, clean, Xc)] + ([(Ref(), clean, Xc)] if have_ref() else [])
    ny, nx = P.tiles(rows, cols, W)
    for src, image, samples in sources:
        for ti in range(ny):
            for tj in range(nx):
                B = src.get_submatrix(image, cols, ti * W, (ti + 1) * W, tj * W, (tj + 1) * W)
                want = P.unpack(B, P.words(W))[:, :W].reshape(-1)
                assert np.array_equal(samples[ti * nx + tj, :W * W], want), (ti, tj)


# ---- (b) the host binary_matrix ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("patch_host") / "patch_host_check")
    src = [os.path.join(ROOT, "tests", "cpp", "patch_host_check.cpp")]
    src += [os.path.join(PKG, "host", f) for f in ("binmat.cpp", "util.cpp", "pbm.cpp")]
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", exe] + src, check=True)
    return exe


@pytest.mark.parametrize("dirty", [0, 1])
@pytest.mark.parametrize("rows,cols,W", GEOMS)
def test_host_gather_loop(host_exe, tmp_path, rows, cols, W, dirty):
    I = random_plane(7 * rows + cols + W, rows, cols, dirty=False)
    src = pbm_file(tmp_path / "I.pbm", I, cols)
    if dirty and cols % 64:  # (the program sets every pad bit after reading the file)
        I[:, -1] |= np.uint64((1 << (64 - cols % 64)) - 1)
    out = str(tmp_path / "X.bin")
    subprocess.run([host_exe, "gather", src, str(W), str(dirty), out], check=True, timeout=60)
    ny, nx = P.tiles(rows, cols, W)
    got = np.fromfile(out, np.uint64).reshape(ny * nx, P.words(W * W))
    st = {}
    want = P.gather(I, cols, W, st)
    assert np.array_equal(got, want)  # all own words of X, pad bits included
    if dirty and cols % 64 and nx * W > cols:
        assert st["pad_ones"] > 0


@pytest.mark.parametrize("rows,cols,W", GEOMS)
def test_host_scatter_loop(host_exe, tmp_path, rows, cols, W):
    ny, nx = P.tiles(rows, cols, W)
    X = random_plane(rows + 3 * cols + W, ny * nx, W * W, dirty=False)
    src = pbm_file(tmp_path / "X.pbm", X, W * W)
    out = str(tmp_path / "I.pbm")
    subprocess.run([host_exe, "scatter", src, str(W), str(rows), str(cols), out], check=True, timeout=60)
    with open(out, "rb") as f:
        rr, cc, got = read_pbm_bytes(f.read())
    assert (rr, cc) == (rows, cols)
    want = P.scatter(X, W, rows, cols)
    assert np.array_equal(valid(got, cols), valid(want, cols))
    assert not (P.unpack(want, P.words(cols))[:, cols:]).any()  # the restatement's padding is zero


@pytest.mark.parametrize("n,m", MOSAICS)
def test_host_render_mosaic(host_exe, tmp_path, n, m):
    D = random_plane(31 * n + m, n, m, dirty=False)
    src = pbm_file(tmp_path / "D.pbm", D, m)
    out = str(tmp_path / "mosaic.pbm")
    subprocess.run([host_exe, "mosaic", src, out], check=True, timeout=60)
    want = P.mosaic(D, m)
    _, _, irows, icols = P.mosaic_dims(n, m)
    with open(out, "rb") as f:
        data = f.read()
    assert data == f"P4\n{icols} {irows}\n".encode() + plane_to_p4_rows(want, icols).tobytes()  # the whole file


# ---- (c) literals ------------------------------------------------------------------------------------------------------

def test_gather_3x3_w2_by_hand():
    """a b c / d e f / g h i with W = 2: four tiles; columns 3 .. read the pad, rows 3 .. read 0"""
    bits = np.array([[1, 0, 1], [0, 1, 1], [1, 1, 0]], np.uint8)
    I = P.pack(bits)
    X = P.unpack(P.gather(I, 3, 2), 1)[:, :4]
    assert X.tolist() == [[1, 0, 0, 1], [1, 0, 1, 0], [1, 1, 0, 0], [0, 0, 0, 0]]
    I[:, 0] |= np.uint64(1 << 60)  # the pad column 3 of every row set: tile 1 and tile 3 read it
    X = P.unpack(P.gather(I, 3, 2), 1)[:, :4]
    assert X.tolist() == [[1, 0, 0, 1], [1, 1, 1, 1], [1, 1, 0, 0], [0, 1, 0, 0]]
    back = P.unpack(P.scatter(P.gather(I, 3, 2), 2, 3, 3), 1)
    assert back[:, :3].tolist() == bits.tolist() and not back[:, 3:].any()


def test_gather_2x64_w3_wraps_into_row_1():
    """cols = 64: one word per row, no pad. The last tile of row band 0 starts at column 63: its columns 64 and
    65 are the FLAT bits after the row's word: columns 0 and 1 of the next row"""
    bits = np.zeros((2, 64), np.uint8)
    bits[0, 63] = 1
    bits[1, 0] = 1   # read by tile 21 as (row 0, column 64)
    bits[1, 63] = 1
    I = P.pack(bits)
    st = {}
    X = P.unpack(P.gather(I, 64, 3, st), 1)[:, :9]
    assert X.shape[0] == 22 and st["wrap_ones"] == 1 and st["pad_ones"] == 0
    # tile 21: row 0 reads columns 63, 64, 65 -> 1, then row 1's columns 0, 1 -> 1 0; row 1 reads its column 63 and
    # then past the last row -> 1 0 0; row 2 is past the image
    assert X[21].tolist() == [1, 1, 0, 1, 0, 0, 0, 0, 0]
    assert X[0].tolist() == [0, 0, 0, 1, 0, 0, 0, 0, 0]
    assert not X[1:21].any()


@pytest.mark.parametrize("n,m,dims", [(1, 1, (2, 2)), (5, 25, (12, 18)), (7, 70, (27, 27)), (512, 256, (391, 391)),
                                      (3, 4500, (136, 136))])
def test_mosaic_dims_literals(n, m, dims):
    assert P.mosaic_dims(n, m)[2:] == dims
    D = np.zeros((n, P.words(m)), np.uint64)
    assert P.mosaic(D, m).shape == (dims[0], P.words(dims[1]))


def test_mosaic_by_hand():
    """two atoms of 5 bits: w = 2, gn = 2, one tile row of 3 x 6 pixels; bit 4 of an atom is ignored"""
    D = P.pack(np.array([[1, 0, 1, 1, 1], [0, 1, 0, 0, 1]], np.uint8))
    img = P.unpack(P.mosaic(D, 5), 1)[:, :6]
    assert img.tolist() == [[1, 0, 0, 0, 1, 0], [1, 1, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0]]
