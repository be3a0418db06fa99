"""The inputs of the growing-dictionary tests (tests/test_dict_ref.py, tests/test_gpu_dict.py) and of their
golden records (tests/golden/make_golden_dict.py): seeded planes, the same on every side. T is variant 3's
threshold. `main` cases carry the input conditions test_dict_ref.py asserts."""
import os

import numpy as np

from dict_ref import glyph_plane
from oracle_lib import pack_rows, periodic_plane
from pnm_io import read_pbm_bytes

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

CASES = [
    # cols not a multiple of W, tiles past the last row (37 = 7 * 5 + 2)
    dict(name="camera", kind="pbm", file="camera_70x37.pbm", W=5, T=3, variants=[2, 3]),
    dict(name="glyph", kind="glyph", seed=1, rows=128, cols=192, W=16, T=32, variants=[2, 3], main=True),
    # the tile crosses a word boundary, cols not a multiple of 64, a tile row past the last row
    dict(name="w33", kind="periodic", seed=3, rows=96, cols=130, W=33, T=30, ph=33, pw=33, flip=0.02, variants=[2, 3]),
    dict(name="w64", kind="periodic", seed=4, rows=128, cols=128, W=64, T=50, ph=64, pw=64, flip=0.01, variants=[2, 3]),
    dict(name="w8", kind="periodic", seed=5, rows=64, cols=64, W=8, T=2, ph=8, pw=16, flip=0.03, variants=[2, 3]),
    # 2048 tiles, nearly every one joins: the dictionary spans many blocks and LDS chunks
    dict(name="noise", kind="noise", seed=6, rows=256, cols=512, W=8, T=4, variants=[2, 3]),
]


def make_input(case):
    """-> (plane uint64 [rows, ceil(cols/64)], rows, cols)"""
    if case["kind"] == "pbm":
        with open(os.path.join(GOLDEN, case["file"]), "rb") as f:
            rows, cols, plane = read_pbm_bytes(f.read())
        return plane, rows, cols
    rows, cols = case["rows"], case["cols"]
    if case["kind"] == "glyph":
        return glyph_plane(case["seed"], rows, cols, case["W"]), rows, cols
    if case["kind"] == "periodic":
        return periodic_plane(case["seed"], rows, cols, case["ph"], case["pw"], 0.5, case["flip"]), rows, cols
    rng = np.random.default_rng(case["seed"])
    return pack_rows(rng.random((rows, cols)) < 0.5), rows, cols
