"""BIC_OPT_GRAY_CODE: every call that maps samples to planes codes G(v) = v ^ (v >> 1) on the whole sample, every
call that maps planes to samples applies the inverse. Expected planes and streams are the oracle's
(bo_bitplanes, bo_encode_plane) of the numpy-transformed image (graycode_ref.gray), expected samples the
input image (or numpy arithmetic on it): never anything the library produced. All comparisons are exact."""
import numpy as np
import pytest

import pybic
from graycode_ref import gray, ungray
from pybic import CODER_EG, CODER_GOLOMB, as_u64, stream_bytes

pytestmark = pytest.mark.gpu

G, E = CODER_GOLOMB, CODER_EG


@pytest.fixture
def staged(ctx):
    """the staged encoder (and the fused count pass) at test sizes"""
    ctx.set_encoder("staged")
    yield
    ctx.set_encoder("auto")


@pytest.fixture
def gc(ctx):
    """the option on for one test, back to its default afterwards (the context is the session's)"""
    ctx.set_gray_code(True)
    yield
    ctx.set_gray_code(False)


_IMG, _PLANES, _STREAM = {}, {}, {}


def _img(oracle, kind, rows, cols):
    """seeded inputs, made once and read-only: uniform8 / uniform16 (every bit p = 0.5, so bit 8 of a 16-bit
    sample is random and a missing byte coupling shows) -> (key, image, the oracle's planes of gray(image))"""
    key = (kind, rows, cols)
    if key not in _IMG:
        seed = 0x6C0DE + 131 * rows + cols
        if kind == "uniform8":
            a = oracle.gen_bytes(seed, rows * cols).reshape(rows, cols).copy()
        else:
            a = oracle.gen_bytes(seed, 2 * rows * cols).view(np.uint16).reshape(rows, cols).copy()
        a.setflags(write=False)
        _IMG[key] = a
        p = oracle.bitplanes(gray(a), 8 * a.dtype.itemsize)
        p.setflags(write=False)
        _PLANES[key] = p
    return key, _IMG[key], _PLANES[key]


def _stream(oracle, key, k, pred, coder, planes=None):
    q = (key, k, pred, coder)
    if q not in _STREAM:
        eb, est, _ = oracle.encode_plane((_PLANES[key] if planes is None else planes)[k], key[2], pred, coder)
        _STREAM[q] = (eb, est.tobytes())
    return _STREAM[q]


def _raster(ctx, img, big_endian=0, pitch=None, off=0):
    """the samples' bytes (two-byte samples in the chosen order), rows of `pitch` bytes, `off` bytes into a
    larger uint8 device buffer -> (the view at the first sample, pitch)"""
    rows, cols = img.shape
    bps = img.dtype.itemsize
    pitch = pitch or bps * cols
    buf = np.full(off + rows * pitch + 64, 0x5A, np.uint8)
    r = np.full((rows, pitch), 0xC3, np.uint8)  # bytes past the row's samples never reach a plane
    src = img if bps == 1 else img.astype(">u2" if big_endian else "<u2").view(np.uint8).reshape(rows, 2 * cols)
    r[:, :bps * cols] = src
    buf[off:off + rows * pitch] = r.reshape(-1)
    return ctx.torch.from_numpy(buf).to(ctx.dev)[off:], pitch


def _view(t, rows, pitch):
    """[rows, pitch] over a flat device view (the bytes behind the last row's samples belong to the buffer)"""
    return t.as_strided((rows, pitch), (pitch, 1))


def _profiled(ctx, fn):
    """fn() with bic_prof_collect's launch names -> (fn's result, {name: (launches, ms)})"""
    ctx.sync()
    ctx.prof_collect()
    ctx.prof_enable(True)
    try:
        ctx.prof_only(None)
        res = fn()
        got = ctx.prof_collect()
    finally:
        ctx.prof_only(None)
        ctx.prof_enable(False)
    return res, got


def _check_streams(oracle, key, plane0, nplanes, pred, g, e, tag, planes=None):
    for k in range(nplanes):
        for coder, res in ((G, g), (E, e)):
            out, bits = res
            eb, est = _stream(oracle, key, plane0 + k, pred, coder, planes)
            nb = int(as_u64(bits)[k])
            print(tag, "plane", plane0 + k, "coder", coder, "bits", nb, "expected", eb)
            assert nb == eb, (tag, plane0 + k, coder)
            assert stream_bytes(out[k], nb) == est, (tag, plane0 + k, coder)


def _encode(ctx, oracle, kind, rows, cols, pred, store, plane0=0, nplanes=None, pitch=None, off=0, be=0, path="fused"):
    key, img, planes = _img(oracle, kind, rows, cols)
    bps = img.dtype.itemsize
    nplanes = nplanes or 8 * bps
    d, pitch = _raster(ctx, img, be, pitch, off)
    # the fused count pass takes an even plane pitch: returned planes get one (the pad word is not compared);
    # without planes an odd ceil(cols / 64) goes through the two calls, which must give the same streams
    used = (cols + 63) // 64
    out_planes = ctx.empty_i64(nplanes, rows, used + used % 2) if store else None
    if path != "fallback" and not store and used % 2:
        path = "fallback"

    def call():
        if bps == 2:
            return ctx.encode_gray16(d, rows=rows, cols=cols, pitch=pitch, nplanes=nplanes, plane0=plane0,
                                     big_endian=bool(be), predict=bool(pred), planes=out_planes, store_planes=store)
        return ctx.encode_gray(_view(d, rows, pitch), cols=cols, nplanes=nplanes, plane0=plane0, predict=bool(pred),
                               planes=out_planes, store_planes=store)

    (got_planes, g, e), prof = _profiled(ctx, call)
    ctx.sync()
    tag = (kind, rows, cols, pred, store, plane0, nplanes, pitch, off, be)
    # the path the case is meant to reach: the fused count pass (with the EG-source emission when it writes
    # the EG stream itself), or plane extraction and the plane encoder
    if path == "fallback":
        assert "bitplanes_count" not in prof and ("bitplanes_u8" in prof or "bitplanes_u16" in prof), (tag, prof)
    else:
        assert prof["bitplanes_count"][0] == 1 and "bitplanes_u8" not in prof and "bitplanes_u16" not in prof, (tag, prof)
        if path == "egs" and pred and not store:
            assert "encode_rows_golomb_egsrc" in prof, (tag, prof)
    if store:
        assert np.array_equal(as_u64(got_planes)[:, :, :used], planes[plane0:plane0 + nplanes]), tag
    else:
        assert got_planes is None
    _check_streams(oracle, key, plane0, nplanes, pred, g, e, tag)


# ---- 8-bit encode: predict 0/1, planes NULL / returned ----------------------------------------------------
@pytest.mark.parametrize("rows,cols,pitch,off,plane0,nplanes,path", [
    (33, 4096, None, 0, 0, 8, "egs"),     # one whole strip, the count pass writes the EG stream
    (24, 8192, None, 0, 0, 8, "egs"),     # lb and the next-segment word across a strip boundary
    (9, 4100, 4160, 0, 0, 8, "fused"),    # a partial second strip, pad bits
    (5, 70, 128, 0, 0, 8, "fused"),       # one partial strip
    (33, 4096, 4101, 3, 0, 8, "egs"),     # byte offset 3, odd pitch: the misaligned loader
    (24, 8192, None, 0, 3, 4, "egs"),     # a plane range (the shift follows the code)
    (2, 16448, None, 0, 0, 8, "fallback"),  # past 16384 columns: the two calls
])
def test_encode_gray8(ctx, oracle, staged, gc, rows, cols, pitch, off, plane0, nplanes, path):
    for pred in (1, 0):
        for store in (False, True):
            _encode(ctx, oracle, "uniform8", rows, cols, pred, store, plane0, nplanes, pitch, off, path=path)


def test_encode_gray8_packed(ctx, oracle, staged, gc):
    """bic_encode_gray_packed: packed offsets and the row index of the coded image"""
    rows, cols = 33, 4096
    key, img, planes = _img(oracle, "uniform8", rows, cols)
    d, _ = _raster(ctx, img)
    idx = ctx.empty_i64(8 * rows * 2)
    _, (og, bg, fg), (oe, be, fe) = ctx.encode_gray_packed(_view(d, rows, cols), row_index=idx, store_planes=False)
    ctx.sync()
    for coder, out, bits, off in ((G, og, bg, fg), (E, oe, be, fe)):
        words, offs = [], [0]
        for k in range(8):
            eb, est = _stream(oracle, key, k, 1, coder)
            assert int(as_u64(bits)[k]) == eb
            words.append(est)
            offs.append(offs[-1] + (eb + 63) // 64)
        assert list(as_u64(off)) == offs
        assert as_u64(out)[:offs[-1]].tobytes() == b"".join(words)
    ri = as_u64(idx).reshape(8, 2 * rows)
    for k in range(8):
        assert np.array_equal(ri[k], oracle.row_index(planes[k], cols, 1)), k


# ---- 16-bit encode, both byte orders ----------------------------------------------------------------------
@pytest.mark.parametrize("be", [1, 0])
@pytest.mark.parametrize("rows,cols,pitch,off,plane0,nplanes,path", [
    (33, 4096, None, 0, 0, 16, "egs"),
    (24, 8192, None, 0, 0, 16, "egs"),
    (9, 4100, 8320, 0, 0, 16, "fused"),
    (21, 4096, 8197, 3, 0, 16, "egs"),    # misaligned: one wave per byte group
    (20, 4096, None, 0, 5, 6, "egs"),     # crosses the byte boundary
    (20, 4096, None, 0, 7, 1, "egs"),     # the low group alone: still needs the high byte
    (20, 4096, None, 0, 8, 8, "egs"),     # the high group alone
])
def test_encode_gray16(ctx, oracle, staged, gc, rows, cols, pitch, off, plane0, nplanes, path, be):
    for pred in (1, 0):
        for store in (False, True):
            _encode(ctx, oracle, "uniform16", rows, cols, pred, store, plane0, nplanes, pitch, off, be, path)


def test_encode_gray16_packed(ctx, oracle, staged, gc):
    rows, cols = 20, 4096
    key, img, planes = _img(oracle, "uniform16", rows, cols)
    d, pitch = _raster(ctx, img, 1)
    idx = ctx.empty_i64(16 * rows * 2)
    _, (og, bg, fg), (oe, be, fe) = ctx.encode_gray16_packed(d, rows=rows, cols=cols, big_endian=True, row_index=idx,
                                                             store_planes=False)
    ctx.sync()
    for coder, out, bits, off in ((G, og, bg, fg), (E, oe, be, fe)):
        words, offs = [], [0]
        for k in range(16):
            eb, est = _stream(oracle, key, k, 1, coder)
            assert int(as_u64(bits)[k]) == eb
            words.append(est)
            offs.append(offs[-1] + (eb + 63) // 64)
        assert list(as_u64(off)) == offs
        assert as_u64(out)[:offs[-1]].tobytes() == b"".join(words)
    ri = as_u64(idx).reshape(16, 2 * rows)
    for k in range(16):
        assert np.array_equal(ri[k], oracle.row_index(planes[k], cols, 1)), k


# ---- stand-alone extraction -------------------------------------------------------------------------------
@pytest.mark.parametrize("pitch,off", [(1008, 0), (1003, 3)])
def test_bitplanes_u8(ctx, oracle, gc, pitch, off):
    rows, cols = 21, 1000
    key, img, planes = _img(oracle, "uniform8", rows, cols)
    d, pitch = _raster(ctx, img, 0, pitch, off)
    for plane0, n in ((0, 8), (2, 5), (7, 1)):
        got = ctx.bitplanes_u8(_view(d, rows, pitch), cols=cols, nplanes=n, plane0=plane0)
        ctx.sync()
        assert np.array_equal(as_u64(got), planes[plane0:plane0 + n]), (plane0, n)


@pytest.mark.parametrize("be", [1, 0])
@pytest.mark.parametrize("off,slack", [(0, 0), (3, 5)])
def test_bitplanes_u16(ctx, oracle, gc, be, off, slack):
    rows, cols = 21, 1000
    key, img, planes = _img(oracle, "uniform16", rows, cols)
    d, pitch = _raster(ctx, img, be, 2 * cols + slack, off)
    for plane0, n in ((0, 16), (5, 6), (7, 1), (8, 8)):
        got = ctx.bitplanes_u16(d, rows=rows, cols=cols, pitch=pitch, big_endian=bool(be), plane0=plane0, nplanes=n)
        ctx.sync()
        assert np.array_equal(as_u64(got), planes[plane0:plane0 + n]), (plane0, n)


def test_pgm_bitplanes(ctx, oracle, gc):
    rows, cols = 5, 70
    for kind, maxval, off in (("uniform8", 255, 0), ("uniform16", 65535, 0), ("uniform16", 65535, 5)):
        key, img, planes = _img(oracle, kind, rows, cols)
        nb = 8 * img.dtype.itemsize
        d, _ = _raster(ctx, img, 1, None, off)
        got = ctx.pgm_bitplanes(d, rows, cols, maxval, nb)
        ctx.sync()
        assert np.array_equal(as_u64(got), planes), (kind, off)
        p0 = 7 if nb == 16 else 4  # (16-bit: bits 7, 8, 9 -- across the byte boundary)
        got = ctx.pgm_bitplanes(d, rows, cols, maxval, 3, plane0=p0)
        ctx.sync()
        assert np.array_equal(as_u64(got), planes[p0:p0 + 3]), (kind, off, p0)


@pytest.mark.parametrize("rows,cols", [(21, 1000), (8, 1024)])  # byte stores; 16-byte stores
def test_planes_to_gray_inverts_bitplanes(ctx, oracle, gc, rows, cols):
    """planes_to_gray(bitplanes(v)) == v for both sample widths, and from the oracle's planes of G(v)"""
    key, img, planes = _img(oracle, "uniform8", rows, cols)
    d, _ = _raster(ctx, img)
    p = ctx.bitplanes_u8(_view(d, rows, cols), cols=cols)
    for src in (p, ctx.torch.from_numpy(np.array(planes).view(np.int64)).to(ctx.dev)):
        back = ctx.planes_to_gray(src, cols)
        ctx.sync()
        assert np.array_equal(back.cpu().numpy()[:, :cols], img)
    key, img, planes = _img(oracle, "uniform16", rows, cols)
    d, pitch = _raster(ctx, img, 1)
    p = ctx.bitplanes_u16(d, rows=rows, cols=cols, big_endian=True)
    want = img.astype(">u2").view(np.uint8).reshape(rows, 2 * cols)
    for src in (p, ctx.torch.from_numpy(np.array(planes).view(np.int64)).to(ctx.dev)):
        back = ctx.planes_to_gray(src, cols, sample_bytes=2, pitch=2 * cols + (6 if cols % 64 else 0))  # byte stores too
        ctx.sync()
        assert np.array_equal(back.cpu().numpy()[:, :2 * cols], want)
    # a range that reaches the top plane returns the image's own bits; bits below it are 0
    back = ctx.planes_to_gray(p[5:], cols, plane0=5, sample_bytes=2)
    ctx.sync()
    want = (img & np.uint16(0xFFE0)).astype(">u2").view(np.uint8).reshape(rows, 2 * cols)
    assert np.array_equal(back.cpu().numpy()[:, :2 * cols], want)


# ---- decode -----------------------------------------------------------------------------------------------
def _p00(ctx, img, plane0, nplanes):
    """the corner pixel's bits of the planes coded: those of G(v)"""
    v = int(gray(img[0, 0]))
    return ctx.torch.tensor([(v >> (plane0 + b)) & 1 for b in range(nplanes)], dtype=ctx.torch.uint8, device=ctx.dev)


def _round_trip(ctx, img, coder, pred, plane0, nplanes, be, off, slack):
    """encode_gray*_packed -> decode_gray into a buffer `off` bytes past an aligned address, rows
    cols * bps + slack bytes apart -> the decoded samples as the image's dtype"""
    rows, cols = img.shape
    bps = img.dtype.itemsize
    idx = ctx.empty_i64(nplanes * rows * 2) if coder == G else None
    want = dict(golomb=coder == G, eg=coder == E)
    if bps == 2:
        raster = np.ascontiguousarray(img.astype(">u2" if be else "<u2")).view(np.uint8).reshape(rows, 2 * cols)
        _, g, e = ctx.encode_gray16_packed(ctx.torch.from_numpy(raster).to(ctx.dev), rows=rows, cols=cols, nplanes=nplanes,
                                           plane0=plane0, big_endian=bool(be), predict=bool(pred), row_index=idx,
                                           store_planes=False, **want)
    else:
        _, g, e = ctx.encode_gray_packed(ctx.torch.from_numpy(np.array(img)).to(ctx.dev), nplanes=nplanes, plane0=plane0,
                                         predict=bool(pred), row_index=idx, store_planes=False, **want)
    out, bits, woff = g if coder == G else e
    pitch = cols * bps + slack
    buf = ctx.torch.zeros(off + rows * pitch + 64, dtype=ctx.torch.uint8, device=ctx.dev)
    ctx.decode_gray(coder, out, bits, nplanes, rows, cols, bool(pred), word_off=woff, row_index=idx,
                    p00=_p00(ctx, img, plane0, nplanes) if pred else None, plane0=plane0, sample_bytes=bps,
                    big_endian=bool(be), out=buf[off:], pitch=pitch)
    ctx.sync()
    h = buf.cpu().numpy()
    assert (h[:off] == 0).all() and (h[off + rows * pitch:] == 0).all()
    got = h[off:off + rows * pitch].reshape(rows, pitch)
    assert (got[:, cols * bps:] == 0).all()  # nothing stored between the rows
    got = np.ascontiguousarray(got[:, :cols * bps])
    return got if bps == 1 else got.view(">u2" if be else "<u2").astype(np.uint16)


@pytest.mark.parametrize("off,slack", [(0, 0), (3, 5)])  # 16-byte stores; byte stores
@pytest.mark.parametrize("coder", [G, E])
@pytest.mark.parametrize("pred", [1, 0])
def test_round_trip_8bit(ctx, oracle, staged, gc, coder, pred, off, slack):
    _, img, _ = _img(oracle, "uniform8", 40, 4096)
    assert np.array_equal(_round_trip(ctx, img, coder, pred, 0, 8, 0, off, slack), img)


@pytest.mark.parametrize("off,slack", [(0, 8), (3, 5)])  # 16-byte stores in the full words; byte stores
@pytest.mark.parametrize("be", [1, 0])
@pytest.mark.parametrize("coder", [G, E])
@pytest.mark.parametrize("pred", [1, 0])
def test_round_trip_16bit(ctx, oracle, staged, gc, coder, pred, be, off, slack):
    _, img, _ = _img(oracle, "uniform16", 24, 4100)
    assert np.array_equal(_round_trip(ctx, img, coder, pred, 0, 16, be, off, slack), img)


@pytest.mark.parametrize("coder", [G, E])
def test_decode_ranges(ctx, oracle, staged, gc, coder):
    """ranges that reach the top plane return v & mask; one that drops high planes returns the documented
    ungray(G(v) & mask) & mask"""
    _, img8, _ = _img(oracle, "uniform8", 40, 4096)
    assert np.array_equal(_round_trip(ctx, img8, coder, 1, 2, 6, 0, 0, 0), img8 & np.uint8(0xFC))
    _, img16, _ = _img(oracle, "uniform16", 24, 4100)
    for be in (1, 0):
        assert np.array_equal(_round_trip(ctx, img16, coder, 1, 5, 11, be, 0, 8), img16 & np.uint16(0xFFE0))
    want = ungray(gray(img8) & np.uint8(0x1F), 8) & np.uint8(0x1F)
    assert not np.array_equal(want, img8 & np.uint8(0x1F))  # (the case is the non-invertible one)
    assert np.array_equal(_round_trip(ctx, img8, coder, 1, 0, 5, 0, 0, 0), want)


# ---- option hygiene ---------------------------------------------------------------------------------------
def test_option_off_after_on(ctx, oracle, staged):
    rows, cols = 33, 4096
    key, img, _ = _img(oracle, "uniform8", rows, cols)
    plain = oracle.bitplanes(img, 8)
    d, _ = _raster(ctx, img)
    ctx.set_gray_code(True)
    ctx.encode_gray(_view(d, rows, cols), store_planes=False)
    ctx.set_gray_code(False)
    for store in (False, True):
        got, g, e = ctx.encode_gray(_view(d, rows, cols), store_planes=store)
        ctx.sync()
        if store:
            assert np.array_equal(as_u64(got), plain)
        _check_streams(oracle, ("plain8", rows, cols), 0, 8, 1, g, e, ("off", store), plain)


def test_option_rejects_other_values(ctx, oracle):
    rows, cols = 5, 70
    key, img, coded = _img(oracle, "uniform8", rows, cols)
    plain = oracle.bitplanes(img, 8)
    d, _ = _raster(ctx, img)
    try:
        for on, want in ((False, plain), (True, coded)):
            ctx.set_gray_code(on)
            for bad in (2, -1):
                with pytest.raises(pybic.BicError) as err:
                    ctx.set_gray_code(bad)
                assert err.value.code == pybic.BIC_EINVAL
            got = ctx.bitplanes_u8(_view(d, rows, cols), cols=cols)
            ctx.sync()
            assert np.array_equal(as_u64(got), want), on  # the setting stayed as it was
    finally:
        ctx.set_gray_code(False)
