"""bic_encode_gray16 / bic_encode_gray16_packed / bic_bitplanes_u16 (samples of two bytes, pnm.cpp:71-74)
against the oracle: the planes are bitplane_tool.cpp:24-30's of the 16-bit samples (bo_bitplanes with
2-byte samples), the streams each plane's Golomb and EG streams (bo_encode_plane). Nothing is compared
only with the code under test, except where a test says it compares two paths of the library."""
import numpy as np
import pytest

import pybic
from pnm_io import write_pgm
from pybic import as_u64, stream_bytes

pytestmark = pytest.mark.gpu


@pytest.fixture
def staged(ctx):
    """the staged encoder (and the fused count pass) at test sizes, which the automatic choice would
    give to the single kernel"""
    ctx.set_encoder("staged")
    yield
    ctx.set_encoder("auto")


_IMG, _PLANES, _STREAM = {}, {}, {}


def _img(oracle, kind, rows, cols):
    """seeded inputs: uniform16 (every plane p = 0.5), smooth12 (planes 12-15 zero, long runs in the
    middle planes), blank_top (smooth12 with a constant top half: the first residual 1 deep in the plane)"""
    key = (kind, rows, cols)
    if key not in _IMG:
        seed = 0x16B17 + 131 * rows + cols
        if kind == "uniform16":
            a = oracle.gen_bytes(seed, 2 * rows * cols).view(np.uint16).reshape(rows, cols).copy()
        else:
            i, j = np.mgrid[0:rows, 0:cols]
            noise = oracle.gen_bytes(seed, rows * cols).reshape(rows, cols) % 7
            a = ((37 * i + 3 * j + noise) % 4096).astype(np.uint16)
            if kind == "blank_top":
                a[:rows // 2] = 0x0A37
        _IMG[key] = a
        _PLANES[key] = oracle.bitplanes(a, 16)
    return key, _IMG[key], _PLANES[key]


def _stream(oracle, key, k, pred, coder):
    """plane k's expected (bits, stream bytes), computed once per (image, plane, pred, coder)"""
    q = (key, k, pred, coder)
    if q not in _STREAM:
        eb, est, _ = oracle.encode_plane(_PLANES[key][k], key[2], pred, coder)
        _STREAM[q] = (eb, est.tobytes())
    return _STREAM[q]


def _raster(ctx, img, big_endian, pitch=None, off=0):
    """the samples as raster bytes in the chosen order, rows of `pitch` bytes, `off` bytes into a larger
    uint8 device buffer -> (the view at the first sample, pitch)"""
    rows, cols = img.shape
    pitch = pitch or 2 * cols
    buf = np.full(off + rows * pitch + 64, 0x5A, np.uint8)
    r = np.full((rows, pitch), 0xC3, np.uint8)  # bytes past 2 * cols never reach a plane
    r[:, :2 * cols] = img.astype(">u2" if big_endian else "<u2").view(np.uint8).reshape(rows, 2 * cols)
    buf[off:off + rows * pitch] = r.reshape(-1)
    d = ctx.torch.from_numpy(buf).to(ctx.dev)
    return d[off:], pitch


def _check_streams(oracle, key, plane0, nplanes, pred, g, e, tag=None):
    for k in range(nplanes):
        for coder, res in ((0, g), (1, e)):
            if res is None:
                continue
            out, bits = res
            eb, est = _stream(oracle, key, plane0 + k, pred, coder)
            nb = int(as_u64(bits)[k])
            print(tag, "plane", plane0 + k, "coder", coder, "bits", nb, "expected", eb)
            assert nb == eb, (tag, plane0 + k, coder)
            assert stream_bytes(out[k], nb) == est, (tag, plane0 + k, coder)


def _encode(ctx, oracle, kind, rows, cols, be, pred, store, plane0=0, nplanes=16, pitch=None, off=0):
    key, img, planes16 = _img(oracle, kind, rows, cols)
    d, pitch = _raster(ctx, img, be, pitch, off)
    planes, g, e = ctx.encode_gray16(d, rows=rows, cols=cols, pitch=pitch, nplanes=nplanes, plane0=plane0,
                                     big_endian=bool(be), predict=bool(pred), store_planes=store)
    ctx.sync()
    tag = (kind, rows, cols, be, pred, store, plane0, nplanes, pitch, off)
    if store:
        assert np.array_equal(as_u64(planes), planes16[plane0:plane0 + nplanes]), tag
    else:
        assert planes is None
    _check_streams(oracle, key, plane0, nplanes, pred, g, e, tag)


# 1. the fused path with the EG stream as the residual source (planes NULL, predict, both streams);
#    predict = 0 takes the route through the context's residual buffer
@pytest.mark.parametrize("be", [1, 0])
@pytest.mark.parametrize("rows,cols,kind", [
    (33, 4096, "uniform16"),   # one whole strip
    (24, 8192, "uniform16"),   # two strips: the next-segment word across a strip boundary
    (70, 16384, "smooth12"),   # four strips
    (1, 4096, "uniform16"),
    (60, 4096, "blank_top"),
])
def test_gray16_eg_source(ctx, oracle, staged, rows, cols, kind, be):
    for pred in (1, 0):
        _encode(ctx, oracle, kind, rows, cols, be, pred, False)


def test_gray16_launches(ctx, oracle, staged):
    """which kernels a call launches (bic_prof_collect's names): the fused count pass where it applies
    (with the EG-source emission when the planes are not wanted), plane extraction otherwise -- so
    that the cases above test the path they are meant to, not the fallback"""
    key, img, _ = _img(oracle, "uniform16", 33, 4096)
    d, pitch = _raster(ctx, img, 1)
    ctx.sync()
    ctx.prof_collect()
    ctx.prof_enable(True)
    try:
        ctx.prof_only(None)
        ctx.encode_gray16(d, rows=33, cols=4096, big_endian=True, store_planes=False)
        got = ctx.prof_collect()
        assert got["bitplanes_count"][0] == 1 and "encode_rows_golomb_egsrc" in got and "bitplanes_u16" not in got, got
        ctx.encode_gray16(d, rows=33, cols=4096, big_endian=True, store_planes=True)
        got = ctx.prof_collect()
        assert got["bitplanes_count"][0] == 1 and "encode_rows_golomb_eg" in got and "bitplanes_u16" not in got, got
        ctx.encode_gray16(d, rows=33, cols=2000, pitch=8192, big_endian=True)  # 32 words: 4096 readable bytes
        got = ctx.prof_collect()
        assert got["bitplanes_count"][0] == 1, got
        ctx.encode_gray16(d, rows=33, cols=2000, pitch=4000, big_endian=True)  # rows too short for the fused read
        got = ctx.prof_collect()
        assert got["bitplanes_u16"][0] == 1 and "bitplanes_count" not in got, got
    finally:
        ctx.prof_only(None)
        ctx.prof_enable(False)


# 2. the fused path with the planes returned, partial strips
@pytest.mark.parametrize("be", [1, 0])
@pytest.mark.parametrize("rows,cols,pitch,kind", [
    (40, 5000, 10240, "smooth12"),
    (17, 100, 256, "uniform16"),  # one partial word, the pitch just enough for the fused read
])
def test_gray16_planes_returned(ctx, oracle, staged, rows, cols, pitch, kind, be):
    for pred in (1, 0):
        _encode(ctx, oracle, kind, rows, cols, be, pred, True, pitch=pitch)
    _encode(ctx, oracle, kind, rows, cols, be, 1, False, pitch=pitch)


# 3. plane ranges: the same planes as the full call's (both are the oracle's)
@pytest.mark.parametrize("plane0,nplanes", [(0, 16), (0, 12), (5, 6), (8, 8), (3, 4), (15, 1)])
@pytest.mark.parametrize("kind,be", [("uniform16", 1), ("smooth12", 0)])
def test_gray16_plane_range(ctx, oracle, staged, plane0, nplanes, kind, be):
    for store in (False, True):
        _encode(ctx, oracle, kind, 20, 4096, be, 1, store, plane0=plane0, nplanes=nplanes)
    _encode(ctx, oracle, kind, 20, 4096, be, 0, False, plane0=plane0, nplanes=nplanes)


# 4. a raster at any byte offset and pitch
@pytest.mark.parametrize("off", [1, 7, 19])
@pytest.mark.parametrize("slack", [0, 6])
def test_gray16_misaligned(ctx, oracle, staged, off, slack):
    rows, cols = 21, 4096
    for be, store in ((1, False), (0, True)):
        _encode(ctx, oracle, "uniform16", rows, cols, be, 1, store, pitch=2 * cols + slack, off=off)


def test_gray16_p5_file(ctx, oracle, staged, tmp_path):
    """a P5 file with maxval 4095 and a comment line, encoded where its raster lies in the file's bytes"""
    rows, cols = 21, 4096
    key, img, planes16 = _img(oracle, "smooth12", rows, cols)
    data = open(write_pgm(str(tmp_path / "g.pgm"), img, 4095, comment="sixteen bits"), "rb").read()
    h = pybic.pnm_header(data[:256])
    assert (h.type, h.rows, h.cols, h.maxval) == (5, rows, cols, 4095)
    dev = ctx.torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(ctx.dev)
    for store in (False, True):
        planes, g, e = ctx.encode_gray16(dev[h.data_offset:], rows=rows, cols=cols, nplanes=12, big_endian=True,
                                         store_planes=store)
        ctx.sync()
        if store:
            assert np.array_equal(as_u64(planes), planes16[:12])
        _check_streams(oracle, key, 0, 12, 1, g, e, ("p5", store))


# 5. where the fused path does not apply: plane extraction + the plane encoder
def test_gray16_fallback_short_rows(ctx, oracle, staged):
    for be in (1, 0):
        for store in (True, False):
            for pred in (1, 0):
                _encode(ctx, oracle, "uniform16", 9, 300, be, pred, store, pitch=600)


@pytest.mark.parametrize("name", ["single-kernel", "two-pass"])
def test_gray16_fallback_encoders(ctx, oracle, name):
    ctx.set_encoder(name)
    try:
        for store in (True, False):
            _encode(ctx, oracle, "smooth12", 20, 4096, 1, 1, store)
        _encode(ctx, oracle, "uniform16", 9, 300, 0, 1, False, plane0=5, nplanes=6, pitch=600)
    finally:
        ctx.set_encoder("auto")


# 6. packed output, the row index, and the device round trip back to the raster
def _packed_expect(oracle, key, nplanes, pred, coder):
    """the packed buffer bic_pack_streams makes of the oracle's streams, and the word offsets"""
    words, offs = [], [0]
    for k in range(nplanes):
        eb, est = _stream(oracle, key, k, pred, coder)
        words.append(est)
        offs.append(offs[-1] + (eb + 63) // 64)
    return b"".join(words), offs


@pytest.mark.parametrize("store", [False, True])
def test_gray16_packed_round_trip(ctx, oracle, staged, store):
    rows, cols = 40, 4096
    key, img, planes16 = _img(oracle, "smooth12", rows, cols)
    d, pitch = _raster(ctx, img, 1)
    idx = ctx.empty_i64(16 * rows * 2)
    planes, (og, bg, fg), (oe, be, fe) = ctx.encode_gray16_packed(d, rows=rows, cols=cols, big_endian=True,
                                                                  store_planes=store, row_index=idx)
    ctx.sync()
    for coder, out, off in ((0, og, fg), (1, oe, fe)):
        exp, eoff = _packed_expect(oracle, key, 16, 1, coder)
        assert list(as_u64(off)) == eoff
        assert as_u64(out)[:eoff[-1]].tobytes() == exp
    ri = as_u64(idx).reshape(16, 2 * rows)
    for k in range(16):
        assert np.array_equal(ri[k], oracle.row_index(planes16[k], cols, 1)), k
    p00 = ctx.torch.from_numpy(((int(img[0, 0]) >> np.arange(16)) & 1).astype(np.uint8)).to(ctx.dev)
    want = img.astype(">u2").view(np.uint8).reshape(rows, 2 * cols)
    for back in (ctx.decode_planes(0, og, bg, 16, rows, cols, True, word_off=fg, row_index=idx, p00=p00),
                 ctx.decode_planes(1, oe, be, 16, rows, cols, True, word_off=fe, p00=p00)):
        ctx.sync()
        assert np.array_equal(as_u64(back), planes16)
        gray = ctx.planes_to_gray(back, cols, sample_bytes=2)
        ctx.sync()
        assert np.array_equal(gray.cpu().numpy(), want)


# 7. the one call == the two calls (bic_pgm_bitplanes + bic_encode_planes2), 16 x 300 = 4800 plane rows
def test_gray16_matches_two_calls(ctx, oracle, staged):
    rows, cols = 300, 16384
    img = oracle.gen_bytes(0x2CA11, 2 * rows * cols).view(np.uint16).reshape(rows, cols)
    d, _ = _raster(ctx, img, 1)
    planes, (og, bg), (oe, be) = ctx.encode_gray16(d, rows=rows, cols=cols, big_endian=True)
    _, (og1, bg1), (oe1, be1) = ctx.encode_gray16(d, rows=rows, cols=cols, big_endian=True, store_planes=False)
    p2 = ctx.pgm_bitplanes(d, rows, cols, 65535, 16)
    (og2, bg2), (oe2, be2) = ctx.encode_planes2(p2, cols, True)
    # the host's order from a 16-bit tensor (int16 carries the same bits)
    t16 = ctx.torch.from_numpy(img.astype("<u2").view(np.int16)).to(ctx.dev)
    planes3, (og3, bg3), (oe3, be3) = ctx.encode_gray16(t16)
    ctx.sync()
    assert ctx.torch.equal(planes, p2) and ctx.torch.equal(planes3, p2)
    for b in (bg, bg1, bg3):
        assert np.array_equal(as_u64(b), as_u64(bg2))
    for b in (be, be1, be3):
        assert np.array_equal(as_u64(b), as_u64(be2))
    nbg, nbe = as_u64(bg2), as_u64(be2)
    for k in range(16):
        wg, we = (int(nbg[k]) + 63) // 64, (int(nbe[k]) + 63) // 64
        for o in (og, og1, og3):
            assert ctx.torch.equal(o[k, :wg], og2[k, :wg]), k
        for o in (oe, oe1, oe3):
            assert ctx.torch.equal(o[k, :we], oe2[k, :we]), k


# 8. refusals, and an 8-bit call on the same context afterwards (shared scratch, the residual buffer)
def test_gray16_rejects(ctx, oracle, staged):
    t = ctx.torch
    g = t.zeros((4, 128), dtype=t.uint8, device=ctx.dev)
    for kw in (dict(cols=64, plane0=1, nplanes=16), dict(cols=64, nplanes=0, planes=ctx.empty_i64(1, 4, 1)),
               dict(cols=64, pitch=127), dict(cols=64, golomb=False, eg=False)):
        kw.setdefault("pitch", 128)
        with pytest.raises(pybic.BicError) as e:
            ctx.encode_gray16(g, rows=4, **kw)
        assert e.value.code == pybic.BIC_EINVAL, kw
    with pytest.raises(pybic.BicError) as e:
        ctx.bitplanes_u16(g, rows=4, cols=64, pitch=128, plane0=9, nplanes=8)
    assert e.value.code == pybic.BIC_EINVAL
    _encode(ctx, oracle, "uniform16", 33, 4096, 1, 1, False)
    _encode(ctx, oracle, "uniform16", 33, 4096, 1, 0, False)
    rows, cols = 33, 4096
    img8 = oracle.gen_bytes(0x8B17, rows * cols).reshape(rows, cols)
    exp = oracle.bitplanes(img8, 8)
    for store in (False, True):
        planes, (og, bg), (oe, be) = ctx.encode_gray(t.from_numpy(img8).to(ctx.dev), store_planes=store)
        ctx.sync()
        if store:
            assert np.array_equal(as_u64(planes), exp)
        for k in range(8):
            for coder, out, bits in ((0, og, bg), (1, oe, be)):
                eb, est, _ = oracle.encode_plane(exp[k], cols, 1, coder)
                nb = int(as_u64(bits)[k])
                assert nb == eb and stream_bytes(out[k], nb) == est.tobytes(), (store, k, coder)


# 9. bic_bitplanes_u16
@pytest.mark.parametrize("be", [1, 0])
@pytest.mark.parametrize("off,slack", [(0, 0), (3, 10), (1, 0)])
def test_bitplanes_u16(ctx, oracle, be, off, slack):
    rows, cols = 21, 1000
    key, img, planes16 = _img(oracle, "uniform16", rows, cols)
    d, pitch = _raster(ctx, img, be, 2 * cols + slack, off)
    for plane0, n in ((0, 16), (5, 6), (8, 8), (15, 1)):
        got = ctx.bitplanes_u16(d, rows=rows, cols=cols, pitch=pitch, big_endian=bool(be), plane0=plane0, nplanes=n)
        ctx.sync()
        assert np.array_equal(as_u64(got), planes16[plane0:plane0 + n]), (plane0, n)
