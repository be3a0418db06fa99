"""bic_encode_rgb / bic_encode_rgb_packed / bic_bitplanes_rgb (interleaved R G B samples of one byte,
pnm.cpp:194-239) against the oracle: output c * nplanes + k is plane plane0 + k of channel c, its planes
bo_bitplanes' of img[:, :, c] taken as a gray image and its streams bo_encode_plane's of them. Nothing is
compared only with the code under test, except where a test says it compares two paths of the library."""
import ctypes as C

import numpy as np
import pytest

import pybic
from pybic import as_u64, stream_bytes

pytestmark = pytest.mark.gpu


@pytest.fixture
def staged(ctx):
    """the staged encoder (and the fused count pass) at test sizes, which the automatic choice would
    give to the single kernel"""
    ctx.set_encoder("staged")
    yield
    ctx.set_encoder("auto")


@pytest.fixture
def gray_code(ctx):
    ctx.set_gray_code(True)
    yield
    ctx.set_gray_code(False)


_IMG, _PLANES, _STREAM = {}, {}, {}


def _img(oracle, kind, rows, cols, gc=False):
    """seeded inputs, every channel different from the others: uniform24 (independent uniform bytes), smooth
    (a different ramp and noise per channel, long runs in the upper planes), blank_top (smooth with a constant
    top half: the first residual 1 deep in the plane). -> (key, img [rows, cols, 3], the 24 expected planes:
    plane 8 c + b = bit b of channel c; gc: of v ^ (v >> 1) per channel)"""
    key = (kind, rows, cols, gc)
    if key not in _IMG:
        seed = 0x52474200 + 131 * rows + cols
        if kind == "uniform24":
            a = oracle.gen_bytes(seed, 3 * rows * cols).reshape(rows, cols, 3).copy()
        else:
            i, j = np.mgrid[0:rows, 0:cols]
            n = oracle.gen_bytes(seed, 3 * rows * cols).reshape(3, rows, cols)
            a = np.stack([(3 * i + j // 7 + n[0] % 5) % 200, (5 * i + j // 3 + n[1] % 3) % 120,
                          (i // 2 + 2 * j // 11 + n[2] % 7) % 61], axis=2).astype(np.uint8)
            if kind == "blank_top":
                a[:rows // 2] = (0x37, 0xA4, 0x1B)
        for c in range(3):
            assert not np.array_equal(a[:, :, c], a[:, :, (c + 1) % 3])
        _IMG[key] = a
        v = a ^ (a >> 1) if gc else a
        _PLANES[key] = np.concatenate([oracle.bitplanes(np.ascontiguousarray(v[:, :, c]), 8) for c in range(3)])
    return key, _IMG[key], _PLANES[key]


def _stream(oracle, key, p, pred, coder):
    """plane p's (8 c + b) expected (bits, stream bytes), computed once per (image, plane, pred, coder)"""
    q = (key, p, pred, coder)
    if q not in _STREAM:
        eb, est, _ = oracle.encode_plane(_PLANES[key][p], key[2], pred, coder)
        _STREAM[q] = (eb, est.tobytes())
    return _STREAM[q]


def _raster(ctx, img, pitch=None, off=0):
    """the pixels as raster bytes, rows of `pitch` bytes, `off` bytes into a larger uint8 device buffer whose
    other bytes hold a pattern that must never reach a plane -> (the view at the first sample, pitch)"""
    rows, cols, _ = img.shape
    pitch = pitch or 3 * cols
    buf = np.full(off + rows * pitch + 256, 0x5A, np.uint8)
    r = np.full((rows, pitch), 0xC3, np.uint8)
    r[:, :3 * cols] = img.reshape(rows, 3 * cols)
    buf[off:off + rows * pitch] = r.reshape(-1)
    d = ctx.torch.from_numpy(buf).to(ctx.dev)
    return d[off:], pitch


def _want_planes(planes24, plane0, nplanes, wpr=None):
    """the call's 3 * nplanes planes, rows of wpr words (pad words 0)"""
    p = np.concatenate([planes24[8 * c + plane0:8 * c + plane0 + nplanes] for c in range(3)])
    return p if wpr is None else np.pad(p, ((0, 0), (0, 0), (0, wpr - p.shape[2])))


def _even(cols):
    """an even number of words per row: what the one-read count pass takes"""
    return ((cols + 63) // 64 + 1) // 2 * 2


def _check_streams(oracle, key, plane0, nplanes, pred, g, e, tag=None):
    for c in range(3):
        for k in range(nplanes):
            for coder, res in ((0, g), (1, e)):
                if res is None:
                    continue
                out, bits = res[0], res[1]
                eb, est = _stream(oracle, key, 8 * c + plane0 + k, pred, coder)
                nb = int(as_u64(bits)[c * nplanes + k])
                print(tag, "channel", c, "plane", plane0 + k, "coder", coder, "bits", nb, "expected", eb)
                assert nb == eb, (tag, c, plane0 + k, coder)
                assert stream_bytes(out[c * nplanes + k], nb) == est, (tag, c, plane0 + k, coder)


def _encode(ctx, oracle, kind, rows, cols, pred, store, plane0=0, nplanes=8, pitch=None, off=0, gc=False, wpr=None):
    key, img, planes24 = _img(oracle, kind, rows, cols, gc)
    d, pitch = _raster(ctx, img, pitch, off)
    if store and wpr:  # (pad words are the caller's: the count pass writes the words that hold pixels)
        pl = ctx.torch.zeros((3 * nplanes, rows, wpr), dtype=ctx.torch.int64, device=ctx.dev)
    else:
        pl = None
    planes, g, e = ctx.encode_rgb(d, rows=rows, cols=cols, pitch=pitch, nplanes=nplanes, plane0=plane0,
                                  predict=bool(pred), store_planes=store, planes=pl, wpr=wpr)
    ctx.sync()
    tag = (kind, rows, cols, pred, store, plane0, nplanes, pitch, off, gc, wpr)
    if store:
        assert np.array_equal(as_u64(planes), _want_planes(planes24, plane0, nplanes, wpr)), tag
    else:
        assert planes is None
    _check_streams(oracle, key, plane0, nplanes, pred, g, e, tag)


def _fused_pitch(cols, extra=0):
    """the shortest pitch the fused read takes: ceil(cols / 64) * 192"""
    return (cols + 63) // 64 * 192 + extra


# 1. the fused path with the EG stream as the residual source (planes NULL, predict, both streams);
#    predict = 0 takes the route through the context's residual buffer
@pytest.mark.parametrize("rows,cols,kind", [
    (33, 4096, "uniform24"),   # one whole strip
    (24, 8192, "uniform24"),   # two strips: the next-segment word across a strip boundary
    (70, 16384, "smooth"),     # four strips
    (1, 4096, "uniform24"),
    (60, 4096, "blank_top"),
])
def test_rgb_eg_source(ctx, oracle, staged, rows, cols, kind):
    for pred in (1, 0):
        _encode(ctx, oracle, kind, rows, cols, pred, False)


def test_rgb_launches(ctx, oracle, staged):
    """which kernels a call launches (bic_prof_collect's names): the fused count pass where it applies (with
    the EG-source emission when the planes are not wanted), bic_bitplanes_rgb's extraction otherwise -- so
    that the cases of this file test the path they are meant to -- and every one gives the oracle's streams"""
    ctx.sync()
    ctx.prof_collect()
    ctx.prof_enable(True)

    def run(kind, rows, cols, store, pitch=None, off=0, wpr=None):
        ctx.prof_collect()
        _encode(ctx, oracle, kind, rows, cols, 1, store, pitch=pitch, off=off, wpr=wpr)
        return ctx.prof_collect()

    try:
        ctx.prof_only(None)
        for shape in ((33, 4096, "uniform24"), (24, 8192, "uniform24"), (70, 16384, "smooth"), (1, 4096, "uniform24"),
                      (60, 4096, "blank_top")):
            got = run(shape[2], shape[0], shape[1], False)
            assert got["bitplanes_count"][0] == 1 and "encode_rows_golomb_egsrc" in got and "bitplanes_rgb" not in got, got
        got = run("uniform24", 33, 4096, True)
        assert got["bitplanes_count"][0] == 1 and "encode_rows_golomb_eg" in got and "bitplanes_rgb" not in got, got
        got = run("uniform24", 33, 4096, False, pitch=3 * 4096 + 5, off=13)  # misaligned rows: still one read
        assert got["bitplanes_count"][0] == 1 and "encode_rows_golomb_egsrc" in got and "bitplanes_rgb" not in got, got
        for store in (True, False):  # partial last strip: the planes or the residual buffer
            for rows, cols in ((37, 4100), (9, 130)):
                got = run("smooth", rows, cols, store, pitch=_fused_pitch(cols), wpr=_even(cols))
                assert got["bitplanes_count"][0] == 1 and "bitplanes_rgb" not in got, got
                assert "encode_rows_golomb_egsrc" not in got, got
            got = run("smooth", 37, 4100, store, pitch=_fused_pitch(4100))  # an odd wpr: the extraction
            assert got["bitplanes_rgb"][0] == 1 and "bitplanes_count" not in got, got
            # rows wider than 16384 columns: the extraction, then the multi-pass encoder
            got = run("uniform24", 3, 16448, store)
            assert got["bitplanes_rgb"][0] == 1 and "bitplanes_count" not in got, got
            # a pitch shorter than the fused read needs (3 * 4100 < 65 * 192)
            got = run("smooth", 37, 4100, store, wpr=66)
            assert got["bitplanes_rgb"][0] == 1 and "bitplanes_count" not in got, got
        ctx.set_encoder("auto")  # a small batch without the staged encoder forced
        try:
            for store in (True, False):
                got = run("uniform24", 33, 4096, store)
                assert got["bitplanes_rgb"][0] == 1 and "bitplanes_count" not in got, got
        finally:
            ctx.set_encoder("staged")
    finally:
        ctx.prof_only(None)
        ctx.prof_enable(False)


# 2. the planes returned and the residual buffer: partial last strip, pad bits, 3 * cols no multiple of 16;
#    padded pitches (a multiple of 16, and an odd one that still holds the fused read), and the tight pitch,
#    which goes through the extraction
@pytest.mark.parametrize("rows,cols,kind", [(37, 4100, "smooth"), (9, 130, "uniform24")])
@pytest.mark.parametrize("pad", ["fused16", "fused_odd", "tight"])
def test_rgb_planes_returned(ctx, oracle, staged, rows, cols, kind, pad):
    pitch = {"fused16": _fused_pitch(cols), "fused_odd": _fused_pitch(cols, 5), "tight": 3 * cols}[pad]
    assert pad == "tight" or (pitch % 16 == 0) == (pad == "fused16")
    for pred in (1, 0):
        for wpr in (_even(cols), None):  # (65 and 3 words per row are odd: those go through the extraction)
            _encode(ctx, oracle, kind, rows, cols, pred, True, pitch=pitch, wpr=wpr)
            _encode(ctx, oracle, kind, rows, cols, pred, False, pitch=pitch, wpr=wpr)


# 3. a raster at any byte offset into a larger buffer
@pytest.mark.parametrize("off", [0, 1, 5, 13])
def test_rgb_misaligned(ctx, oracle, staged, off):
    for store in (False, True):
        _encode(ctx, oracle, "uniform24", 21, 4096, 1, store, off=off)  # (EG source / planes returned)
        _encode(ctx, oracle, "smooth", 37, 4100, 1, store, pitch=_fused_pitch(4100, 5), off=off, wpr=66)
    _encode(ctx, oracle, "uniform24", 9, 130, 0, True, pitch=_fused_pitch(130), off=off, wpr=4)


# 4. plane ranges: the same planes as the full call's (both are the oracle's)
@pytest.mark.parametrize("plane0,nplanes", [(0, 8), (3, 2), (7, 1), (0, 1)])
@pytest.mark.parametrize("kind", ["uniform24", "smooth"])
def test_rgb_plane_range(ctx, oracle, staged, plane0, nplanes, kind):
    for store in (False, True):
        _encode(ctx, oracle, kind, 20, 4096, 1, store, plane0=plane0, nplanes=nplanes)
    _encode(ctx, oracle, kind, 20, 4096, 0, False, plane0=plane0, nplanes=nplanes)
    _encode(ctx, oracle, kind, 37, 4100, 1, True, plane0=plane0, nplanes=nplanes, pitch=_fused_pitch(4100), wpr=66)


# 5. Gray code on: the expectation is the oracle's on v ^ (v >> 1) per channel
@pytest.mark.parametrize("rows,cols,pitch,off", [(33, 4096, None, 0), (24, 8192, None, 0), (21, 4096, 3 * 4096 + 7, 5),
                                                 (37, 4100, 65 * 192, 0), (37, 4100, 65 * 192 + 5, 1),
                                                 (9, 130, None, 0)])
def test_rgb_gray_code(ctx, oracle, staged, gray_code, rows, cols, pitch, off):
    for store in (False, True):
        _encode(ctx, oracle, "smooth", rows, cols, 1, store, pitch=pitch, off=off, gc=True, wpr=_even(cols))
    _encode(ctx, oracle, "smooth", rows, cols, 0, True, pitch=pitch, off=off, gc=True, wpr=_even(cols))
    _encode(ctx, oracle, "smooth", rows, cols, 1, False, plane0=3, nplanes=2, pitch=pitch, off=off, gc=True,
            wpr=_even(cols))


# 6. where the fused path does not apply for the encoder's sake
@pytest.mark.parametrize("name", ["single-kernel", "two-pass"])
def test_rgb_fallback_encoders(ctx, oracle, name):
    ctx.set_encoder(name)
    try:
        for store in (True, False):
            _encode(ctx, oracle, "smooth", 20, 4096, 1, store)
        _encode(ctx, oracle, "uniform24", 9, 130, 1, False, plane0=3, nplanes=2)
    finally:
        ctx.set_encoder("auto")


# 7. packed output and the row index
def _packed_expect(oracle, key, plane0, nplanes, pred, coder):
    """the packed buffer bic_pack_streams makes of the oracle's streams, and the word offsets"""
    words, offs = [], [0]
    for c in range(3):
        for k in range(nplanes):
            eb, est = _stream(oracle, key, 8 * c + plane0 + k, pred, coder)
            words.append(est)
            offs.append(offs[-1] + (eb + 63) // 64)
    return b"".join(words), offs


def _check_packed(ctx, oracle, key, planes24, rows, cols, plane0, nplanes, g, e, idx, tag):
    for coder, res in ((0, g), (1, e)):
        out, bits, off = res
        exp, eoff = _packed_expect(oracle, key, plane0, nplanes, 1, coder)
        assert list(as_u64(off)) == eoff, (tag, coder)
        assert as_u64(out)[:eoff[-1]].tobytes() == exp, (tag, coder)
    want = _want_planes(planes24, plane0, nplanes)
    ri = as_u64(idx).reshape(3 * nplanes, 2 * rows)
    for p in range(3 * nplanes):
        assert np.array_equal(ri[p], oracle.row_index(want[p], cols, 1)), (tag, p)


@pytest.mark.parametrize("store", [False, True])
@pytest.mark.parametrize("rows,cols,pitch,plane0,nplanes", [(40, 4096, None, 0, 8), (37, 4100, 65 * 192, 3, 2),
                                                            (9, 130, 576, 0, 8), (9, 130, None, 0, 8)])
def test_rgb_packed_and_index(ctx, oracle, staged, store, rows, cols, pitch, plane0, nplanes):
    """the packed streams, their offsets and the row index are the oracle's, hence the slot forms' and
    bic_row_index's of the same planes (compared too)"""
    key, img, planes24 = _img(oracle, "smooth", rows, cols)
    d, pitch = _raster(ctx, img, pitch)
    n3, wpr = 3 * nplanes, _even(cols)  # (an even wpr: the packed streams and the index from the one-read path)
    idx = ctx.empty_i64(n3 * rows * 2)
    pl = ctx.torch.zeros((n3, rows, wpr), dtype=ctx.torch.int64, device=ctx.dev) if store else None
    planes, g, e = ctx.encode_rgb_packed(d, rows=rows, cols=cols, pitch=pitch, plane0=plane0, nplanes=nplanes,
                                         store_planes=store, planes=pl, wpr=wpr, row_index=idx)
    ctx.sync()
    _check_packed(ctx, oracle, key, planes24, rows, cols, plane0, nplanes, g, e, idx, (rows, cols, store))
    want = _want_planes(planes24, plane0, nplanes)
    if store:
        assert np.array_equal(as_u64(planes), _want_planes(planes24, plane0, nplanes, wpr))
    # the library's other path to the same numbers: the slot forms and bic_row_index
    _, (og, bg), (oe, be) = ctx.encode_rgb(d, rows=rows, cols=cols, pitch=pitch, plane0=plane0, nplanes=nplanes)
    idx2 = ctx.row_index(ctx.torch.from_numpy(want.view(np.int64)).to(ctx.dev), cols, True)
    ctx.sync()
    assert np.array_equal(as_u64(idx2), as_u64(idx))
    for (out, bits, off), (so, sb) in ((g, (og, bg)), (e, (oe, be))):
        assert np.array_equal(as_u64(bits), as_u64(sb))
        o, fl = as_u64(off), as_u64(out)
        for p in range(n3):
            nw = (int(as_u64(sb)[p]) + 63) // 64
            assert np.array_equal(fl[int(o[p]):int(o[p]) + nw], as_u64(so[p])[:nw]), p


def test_rgb_p6_file(ctx, oracle, staged):
    """a P6 file's bytes with a comment line in the header, encoded where its raster lies in them"""
    rows, cols = 21, 4096
    key, img, planes24 = _img(oracle, "smooth", rows, cols)
    data = b"P6\n# twenty-four bits\n%d %d\n255\n" % (cols, rows) + img.tobytes()
    h = pybic.pnm_header(data[:256])
    assert (h.type, h.rows, h.cols, h.maxval) == (6, rows, cols, 255)
    assert data[h.data_offset:] == img.tobytes() and h.data_offset % 16 != 0
    dev = ctx.torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(ctx.dev)
    for store in (False, True):
        idx = ctx.empty_i64(24 * rows * 2)
        planes, g, e = ctx.encode_rgb_packed(dev[h.data_offset:], rows=rows, cols=cols, store_planes=store,
                                             row_index=idx)
        ctx.sync()
        if store:
            assert np.array_equal(as_u64(planes), planes24)
        _check_packed(ctx, oracle, key, planes24, rows, cols, 0, 8, g, e, idx, ("p6", store))


# 8. argument errors are BIC_EINVAL with no device work; rows = 0 is BIC_OK
def test_rgb_rejects(ctx, oracle, staged):
    t = ctx.torch
    d = t.zeros(4 * 192, dtype=t.uint8, device=ctx.dev)
    ctx.sync()
    ctx.prof_collect()
    ctx.prof_enable(True)
    try:
        ctx.prof_only(None)
        for kw in (dict(pitch=191), dict(plane0=1, nplanes=8), dict(plane0=8, nplanes=1), dict(nplanes=0),
                   dict(nplanes=9), dict(plane0=-1, nplanes=2), dict(golomb=False, eg=False)):
            kw.setdefault("pitch", 192)
            kw.setdefault("planes", ctx.empty_i64(24, 4, 1))
            for fn in (ctx.encode_rgb, ctx.encode_rgb_packed):
                with pytest.raises(pybic.BicError) as e:
                    fn(d, rows=4, cols=64, **kw)
                assert e.value.code == pybic.BIC_EINVAL, kw
        for kw in (dict(pitch=191), dict(plane0=1, nplanes=8), dict(nplanes=0)):
            kw.setdefault("pitch", 192)
            with pytest.raises(pybic.BicError) as e:
                ctx.bitplanes_rgb(d, rows=4, cols=64, out=ctx.empty_i64(24, 4, 1), **kw)
            assert e.value.code == pybic.BIC_EINVAL, kw
        ctx._bind_stream()
        out, bits = ctx.empty_i64(24, 64), ctx.empty_i64(24)
        vp = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
        rc = ctx.lib.bic_encode_rgb(ctx.h, None, 192, 4, 64, 0, 8, None, 1, 1, vp(out), 64, vp(bits), None, 0, None)
        assert rc == pybic.BIC_EINVAL  # NULL rgb with rows > 0
        assert ctx.prof_collect() == {}
        bits.fill_(-1)
        rc = ctx.lib.bic_encode_rgb(ctx.h, None, 192, 0, 64, 0, 8, None, 1, 1, vp(out), 64, vp(bits), None, 0, None)
        assert rc == pybic.BIC_OK  # rows = 0: every stream empty
        ctx.sync()
        assert (as_u64(bits) == 0).all()
    finally:
        ctx.prof_only(None)
        ctx.prof_enable(False)
    _encode(ctx, oracle, "uniform24", 33, 4096, 1, False)  # and the context encodes afterwards


# 9. bic_bitplanes_rgb alone
@pytest.mark.parametrize("off,slack", [(0, 0), (3, 10), (1, 0), (0, 4)])
def test_bitplanes_rgb(ctx, oracle, off, slack):
    rows, cols = 21, 1000
    key, img, planes24 = _img(oracle, "uniform24", rows, cols)
    d, pitch = _raster(ctx, img, 3 * cols + slack, off)
    for plane0, n in ((0, 8), (3, 2), (7, 1), (0, 1)):
        got = ctx.bitplanes_rgb(d, rows=rows, cols=cols, pitch=pitch, plane0=plane0, nplanes=n)
        ctx.sync()
        assert np.array_equal(as_u64(got), _want_planes(planes24, plane0, n)), (plane0, n)
    wide = ctx.bitplanes_rgb(d, rows=rows, cols=cols, pitch=pitch, wpr=18)  # pad words are written 0
    ctx.sync()
    w = as_u64(wide)
    assert np.array_equal(w[:, :, :16], planes24) and (w[:, :, 16:] == 0).all()
