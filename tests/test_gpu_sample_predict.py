"""BIC_OPT_SAMPLE_PREDICT: every call that maps one-byte gray samples to planes codes T(img) -- each sample minus its
left neighbour, folded in mode 2 -- and every call that maps planes to one-byte samples applies the inverse. Expected
planes and streams are the oracle's (bo_bitplanes, bo_encode_plane) of the numpy-transformed image
(sample_predict_ref.predict, then graycode_ref.gray where that option is on too), expected samples the input image
(or numpy arithmetic on it): never anything the library produced. All comparisons are exact. The inputs are uniform
bytes: every plane of T(img) is then Bernoulli(0.5), so a wrong left neighbour at any one column changes the stream."""
import numpy as np
import pytest

import pybic
from graycode_ref import gray, ungray
from pybic import CODER_EG, CODER_GOLOMB, as_u64, stream_bytes
from sample_predict_ref import predict, unpredict

pytestmark = pytest.mark.gpu

G, E = CODER_GOLOMB, CODER_EG
FILL = 0x5A


@pytest.fixture
def staged(ctx):
    """the staged encoder (and the fused count pass) at test sizes"""
    ctx.set_encoder("staged")
    yield
    ctx.set_encoder("auto")


@pytest.fixture
def opts(ctx):
    """set(mode, gray_code) for one test; both options back to their defaults afterwards (the context is the
    session's)"""
    def set_(mode, gc=False):
        ctx.set_sample_predict(mode)
        ctx.set_gray_code(bool(gc))
    yield set_
    ctx.set_sample_predict(0)
    ctx.set_gray_code(False)


_IMG, _PLANES, _STREAM, _INDEX = {}, {}, {}, {}


def _img(oracle, rows, cols, f=0):
    """seeded uniform bytes, made once and read-only"""
    key = (rows, cols, f)
    if key not in _IMG:
        a = oracle.gen_bytes(0x5A4D + 131 * rows + cols + 7919 * f, rows * cols).reshape(rows, cols).copy()
        a.setflags(write=False)
        _IMG[key] = a
    return _IMG[key]


def _coded(img, mode, gc):
    z = predict(img, mode)
    return gray(z) if gc else z


def _planes(oracle, rows, cols, mode, gc, f=0):
    """-> (key, the oracle's 8 planes of T(img), Gray-coded with gc)"""
    key = (rows, cols, f, mode, int(bool(gc)))
    if key not in _PLANES:
        p = oracle.bitplanes(_coded(_img(oracle, rows, cols, f), mode, gc), 8)
        p.setflags(write=False)
        _PLANES[key] = p
    return key, _PLANES[key]


def _stream(oracle, key, k, pred, coder):
    q = (key, k, pred, coder)
    if q not in _STREAM:
        eb, est, _ = oracle.encode_plane(_PLANES[key][k], key[1], pred, coder)
        _STREAM[q] = (eb, est.tobytes())
    return _STREAM[q]


def _index(oracle, key, k, pred):
    q = (key, k, pred)
    if q not in _INDEX:
        _INDEX[q] = oracle.row_index(_PLANES[key][k], key[1], pred)
    return _INDEX[q]


def _raster(ctx, img, pitch=None, off=0):
    """the samples, rows of `pitch` bytes, `off` bytes into a larger uint8 device buffer -> (the view at the first
    sample, pitch)"""
    rows, cols = img.shape
    pitch = pitch or cols
    buf = np.full(off + rows * pitch + 64, FILL, np.uint8)
    r = np.full((rows, pitch), 0xC3, np.uint8)  # bytes past the row's samples never reach a plane
    r[:, :cols] = img
    buf[off:off + rows * pitch] = r.reshape(-1)
    return ctx.torch.from_numpy(buf).to(ctx.dev)[off:], pitch


def _view(t, rows, pitch):
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


def _check_streams(oracle, key, plane0, nplanes, pred, g, e, tag, base=0):
    """entries base .. base + nplanes - 1 of g / e against planes plane0 .. of key"""
    for k in range(nplanes):
        for coder, res in ((G, g), (E, e)):
            out, bits = res[0], res[1]
            eb, est = _stream(oracle, key, plane0 + k, pred, coder)
            nb = int(as_u64(bits)[base + k])
            print(tag, "plane", plane0 + k, "coder", coder, "bits", nb, "expected", eb)
            assert nb == eb, (tag, plane0 + k, coder)
            assert stream_bytes(out[base + k], nb) == est, (tag, plane0 + k, coder)


def _encode(ctx, oracle, rows, cols, mode, gc, pred, store, plane0=0, nplanes=8, pitch=None, off=0, path="fused"):
    img = _img(oracle, rows, cols)
    key, planes = _planes(oracle, rows, cols, mode, gc)
    d, pitch = _raster(ctx, img, pitch, off)
    # the fused count pass takes an even plane pitch: returned planes get one (the pad word is not compared);
    # without planes an odd ceil(cols / 64) goes through the two calls, which must give the same streams
    used = (cols + 63) // 64
    out_planes = ctx.empty_i64(nplanes, rows, used + used % 2) if store else None
    if path != "fallback" and not store and used % 2:
        path = "fallback"
    (got_planes, g, e), prof = _profiled(ctx, lambda: ctx.encode_gray(
        _view(d, rows, pitch), cols=cols, nplanes=nplanes, plane0=plane0, predict=bool(pred), planes=out_planes,
        store_planes=store))
    ctx.sync()
    tag = (rows, cols, mode, gc, pred, store, plane0, nplanes, pitch, off)
    if path == "fallback":
        assert "bitplanes_count" not in prof and "bitplanes_u8" in prof, (tag, prof)
    else:
        assert prof["bitplanes_count"][0] == 1 and "bitplanes_u8" not in prof, (tag, prof)
        if path == "egs" and pred and not store:
            assert "encode_rows_golomb_egsrc" in prof, (tag, prof)
    if store:
        assert np.array_equal(as_u64(got_planes)[:, :, :used], planes[plane0:plane0 + nplanes]), tag
    else:
        assert got_planes is None
    _check_streams(oracle, key, plane0, nplanes, pred, g, e, tag)


# ---- encode: predict 0/1, planes NULL / returned ------------------------------------------------------------------
_SHAPES = [
    (33, 4096, None, 0, 0, 8, "egs"),       # one whole strip, the count pass writes the EG stream
    (24, 8192, None, 0, 0, 8, "egs"),       # the left byte and the next-segment word across a strip boundary
    (9, 4100, 4160, 0, 0, 8, "fused"),      # a partial second strip, pad bits
    (5, 70, 128, 0, 0, 8, "fused"),         # one partial strip
    (33, 4096, 4101, 3, 0, 8, "egs"),       # byte offset 3, odd pitch: the misaligned loader
    (24, 8192, None, 0, 3, 4, "egs"),       # a plane range (the shift follows T and the code)
    (2, 16448, None, 0, 0, 8, "fallback"),  # past 16384 columns: the two calls
]


# both modes at every shape; the Gray code on top of each at the first two
_CASES = [s + (mode, 0) for s in _SHAPES for mode in (1, 2)] + [s + (mode, 1) for s in _SHAPES[:2] for mode in (1, 2)]


@pytest.mark.parametrize("rows,cols,pitch,off,plane0,nplanes,path,mode,gc", _CASES)
def test_encode_gray(ctx, oracle, staged, opts, rows, cols, pitch, off, plane0, nplanes, path, mode, gc):
    opts(mode, gc)
    for pred in (1, 0):
        for store in (False, True):
            _encode(ctx, oracle, rows, cols, mode, gc, pred, store, plane0, nplanes, pitch, off, path=path)


@pytest.mark.parametrize("mode", [1, 2])
def test_encode_gray_packed(ctx, oracle, staged, opts, mode):
    """bic_encode_gray_packed: packed offsets and the row index of the coded image"""
    rows, cols = 33, 4096
    opts(mode)
    key, planes = _planes(oracle, rows, cols, mode, 0)
    d, _ = _raster(ctx, _img(oracle, rows, cols))
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
        assert np.array_equal(ri[k], _index(oracle, key, k, 1)), k


# ---- frames -------------------------------------------------------------------------------------------------------
def _frame_buffer(ctx, imgs, pitch, gap, off=16):
    n, rows, cols = imgs.shape
    stride = rows * pitch + gap
    buf = np.full(off + n * stride + 80, FILL, np.uint8)
    for f in range(n):
        r = np.full((rows, pitch), 0xC3, np.uint8)
        r[:, :cols] = imgs[f]
        buf[off + f * stride:off + f * stride + rows * pitch] = r.reshape(-1)
    return ctx.torch.from_numpy(buf).to(ctx.dev)[off:], stride


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("n,rows,cols,pitch,gap", [(3, 20, 4096, 4096, 32), (2, 9, 4100, 4160, 48)])
def test_encode_gray_frames_packed(ctx, oracle, staged, opts, n, rows, cols, pitch, gap, mode):
    """each frame's streams equal the single-image expectation: column 0 of every frame has no left"""
    opts(mode)
    imgs = np.stack([_img(oracle, rows, cols, f) for f in range(n)])
    d, stride = _frame_buffer(ctx, imgs, pitch, gap)
    used = (cols + 63) // 64
    wpr = (used + 1) & ~1
    for pred in (1, 0):
        for store in (False, True):
            pl = ctx.empty_i64(n * 8, rows, wpr) if store else None
            idx = ctx.empty_i64(n * 8 * rows * 2)
            (got, g, e), prof = _profiled(ctx, lambda: ctx.encode_gray_frames_packed(
                d, rows, cols, nframes=n, frame_stride=stride, pitch=pitch, predict=bool(pred), planes=pl, wpr=wpr,
                row_index=idx))
            ctx.sync()
            tag = (n, rows, cols, mode, pred, store)
            assert prof["bitplanes_count"][0] == 1 and "bitplanes_u8" not in prof, (tag, prof)
            ri = as_u64(idx).reshape(n * 8, 2 * rows)
            for coder, res in ((G, g), (E, e)):
                exp = [_stream(oracle, _planes(oracle, rows, cols, mode, 0, f)[0], k, pred, coder)
                       for f in range(n) for k in range(8)]
                assert [int(x) for x in as_u64(res[1])] == [x[0] for x in exp], (tag, coder)
                offs = [int(x) for x in as_u64(res[2])]
                assert offs == [sum((x[0] + 63) // 64 for x in exp[:i]) for i in range(n * 8 + 1)], (tag, coder)
                assert as_u64(res[0])[:offs[-1]].tobytes() == b"".join(x[1] for x in exp), (tag, coder)
            for f in range(n):
                key, planes = _planes(oracle, rows, cols, mode, 0, f)
                if store:
                    assert np.array_equal(as_u64(got)[8 * f:8 * f + 8, :, :used], planes), (tag, f)
                for k in range(8):
                    assert np.array_equal(ri[8 * f + k], _index(oracle, key, k, pred)), (tag, f, k)


# ---- stand-alone extraction ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,gc", [(1, 0), (2, 0), (2, 1)])
@pytest.mark.parametrize("pitch,off", [(1008, 0), (1003, 3)])
def test_bitplanes_u8(ctx, oracle, opts, pitch, off, mode, gc):
    rows, cols = 21, 1000
    opts(mode, gc)
    _, planes = _planes(oracle, rows, cols, mode, gc)
    d, pitch = _raster(ctx, _img(oracle, rows, cols), pitch, off)
    for plane0, n in ((0, 8), (2, 5), (7, 1)):
        got = ctx.bitplanes_u8(_view(d, rows, pitch), cols=cols, nplanes=n, plane0=plane0)
        ctx.sync()
        assert np.array_equal(as_u64(got), planes[plane0:plane0 + n]), (plane0, n)


@pytest.mark.parametrize("mode,gc", [(1, 0), (2, 0), (2, 1)])
def test_pgm_bitplanes(ctx, oracle, opts, mode, gc):
    rows, cols = 5, 70
    opts(mode, gc)
    _, planes = _planes(oracle, rows, cols, mode, gc)
    for off in (0, 5):
        d, _ = _raster(ctx, _img(oracle, rows, cols), None, off)
        got = ctx.pgm_bitplanes(d, rows, cols, 255, 8)
        ctx.sync()
        assert np.array_equal(as_u64(got), planes), off
        got = ctx.pgm_bitplanes(d, rows, cols, 255, 3, plane0=4)
        ctx.sync()
        assert np.array_equal(as_u64(got), planes[4:7]), off


# ---- the inverse --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,gc", [(1, 0), (2, 0), (2, 1)])
@pytest.mark.parametrize("rows,cols", [(21, 1000), (8, 1024), (6, 2100)])  # byte stores; 16-byte stores in one
def test_planes_to_gray_inverts_bitplanes(ctx, oracle, opts, rows, cols, mode, gc):  # piece; a carry across pieces
    """planes_to_gray(bitplanes_u8(v)) == v, and the same from the oracle's planes of T(v)"""
    opts(mode, gc)
    img = _img(oracle, rows, cols)
    _, planes = _planes(oracle, rows, cols, mode, gc)
    d, _ = _raster(ctx, img)
    p = ctx.bitplanes_u8(_view(d, rows, cols), cols=cols)
    pitch = (cols + 15) // 16 * 16 + 16  # rows 16-byte aligned, bytes behind the samples
    for src in (p, ctx.torch.from_numpy(np.array(planes).view(np.int64)).to(ctx.dev)):
        out = ctx.torch.full((rows, pitch), FILL, dtype=ctx.torch.uint8, device=ctx.dev)
        back = ctx.planes_to_gray(src, cols, out=out, pitch=pitch)
        ctx.sync()
        h = back.cpu().numpy()
        assert np.array_equal(h[:, :cols], img)
        assert (h[:, cols:] == FILL).all()  # nothing stored behind the row's samples


# ---- round trips --------------------------------------------------------------------------------------------------
def _p00(ctx, img, mode, gc, plane0, nplanes):
    return ctx.torch.from_numpy(pybic.gray_p00(mode, gc, int(img[0, 0]), plane0, nplanes)).to(ctx.dev)


def _round_trip(ctx, img, mode, gc, coder, pred, plane0, nplanes, off, slack):
    """encode_gray_packed -> decode_gray into a buffer `off` bytes past an aligned address, rows cols + slack bytes
    apart, filled beforehand -> the decoded samples; every byte outside them must keep the fill"""
    rows, cols = img.shape
    idx = ctx.empty_i64(nplanes * rows * 2) if coder == G else None
    want = dict(golomb=coder == G, eg=coder == E)
    _, g, e = ctx.encode_gray_packed(ctx.torch.from_numpy(np.array(img)).to(ctx.dev), nplanes=nplanes, plane0=plane0,
                                     predict=bool(pred), row_index=idx, store_planes=False, **want)
    out, bits, woff = g if coder == G else e
    pitch = cols + slack
    buf = ctx.torch.full((off + rows * pitch + 64,), FILL, dtype=ctx.torch.uint8, device=ctx.dev)
    ctx.decode_gray(coder, out, bits, nplanes, rows, cols, bool(pred), word_off=woff, row_index=idx,
                    p00=_p00(ctx, img, mode, gc, plane0, nplanes) if pred else None, plane0=plane0, out=buf[off:],
                    pitch=pitch)
    ctx.sync()
    h = buf.cpu().numpy()
    assert (h[:off] == FILL).all() and (h[off + rows * pitch - slack:] == FILL).all()  # before, behind the last row
    got = h[off:off + rows * pitch].reshape(rows, pitch)
    assert (got[:, cols:] == FILL).all()  # nothing stored between the rows
    return np.ascontiguousarray(got[:, :cols])


@pytest.mark.parametrize("mode,gc", [(1, 0), (2, 0), (2, 1)])
@pytest.mark.parametrize("rows,cols,off,slack", [(40, 4096, 0, 0), (40, 4096, 3, 5), (24, 4100, 0, 5)])
@pytest.mark.parametrize("coder", [G, E])
@pytest.mark.parametrize("pred", [1, 0])
def test_round_trip(ctx, oracle, staged, opts, coder, pred, rows, cols, off, slack, mode, gc):
    opts(mode, gc)
    img = _img(oracle, rows, cols)
    assert np.array_equal(_round_trip(ctx, img, mode, gc, coder, pred, 0, 8, off, slack), img)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("coder", [G, E])
@pytest.mark.parametrize("pred", [1, 0])
def test_round_trip_frames(ctx, oracle, staged, opts, coder, pred, mode):
    """encode_gray_frames_packed -> decode_gray_frames, a gap between the frames that keeps its bytes"""
    n, rows, cols, gap = 3, 20, 4096, 48
    opts(mode)
    imgs = np.stack([_img(oracle, rows, cols, f) for f in range(n)])
    d, stride = _frame_buffer(ctx, imgs, cols, gap)
    idx = ctx.empty_i64(n * 8 * rows * 2)
    _, g, e = ctx.encode_gray_frames_packed(d, rows, cols, nframes=n, frame_stride=stride, pitch=cols,
                                            predict=bool(pred), row_index=idx, golomb=coder == G, eg=coder == E)
    out, bits, woff = g if coder == G else e
    p00 = ctx.torch.from_numpy(np.concatenate([pybic.gray_p00(mode, 0, int(a[0, 0])) for a in imgs])).to(ctx.dev)
    lead, opitch = 16, cols + 16
    ostride = rows * opitch + gap
    total = lead + (n - 1) * ostride + rows * opitch + 48
    buf = ctx.torch.full((total,), FILL, dtype=ctx.torch.uint8, device=ctx.dev)
    ctx.decode_gray_frames(coder, out, bits, n, 8, rows, cols, bool(pred), word_off=woff,
                           row_index=idx if coder == G else None, p00=p00 if pred else None, out=buf[lead:],
                           pitch=opitch, frame_stride=ostride)
    ctx.sync()
    want = np.full(total, FILL, np.uint8)
    for f in range(n):
        for r in range(rows):
            o = lead + f * ostride + r * opitch
            want[o:o + cols] = imgs[f, r]
    got = buf.cpu().numpy()
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]


@pytest.mark.parametrize("mode,gc", [(1, 0), (2, 0), (2, 1)])
@pytest.mark.parametrize("coder", [G, E])
def test_decode_range(ctx, oracle, staged, opts, coder, mode, gc):
    """plane0 = 2, nplanes = 6: the header's formula -- the z sample assembled from the given planes (the others 0,
    un-Grayed and masked), unfolded, summed along the row -- and not the image's own bits"""
    opts(mode, gc)
    img = _img(oracle, 40, 4096)
    c = _coded(img, mode, gc) & np.uint8(0xFC)
    z = (ungray(c, 8) & np.uint8(0xFC)) if gc else c
    want = unpredict(z, mode)
    assert not np.array_equal(want, img & np.uint8(0xFC))  # (the case is the non-invertible one)
    assert np.array_equal(_round_trip(ctx, img, mode, gc, coder, 1, 2, 6, 0, 0), want)


# ---- option hygiene -----------------------------------------------------------------------------------------------
def test_option_off_after_on(ctx, oracle, staged, opts):
    rows, cols = 33, 4096
    img = _img(oracle, rows, cols)
    key, plain = _planes(oracle, rows, cols, 0, 0)
    assert np.array_equal(plain, oracle.bitplanes(img, 8))
    d, _ = _raster(ctx, img)
    opts(2)
    ctx.encode_gray(_view(d, rows, cols), store_planes=False)
    opts(0)
    for store in (False, True):
        got, g, e = ctx.encode_gray(_view(d, rows, cols), store_planes=store)
        ctx.sync()
        if store:
            assert np.array_equal(as_u64(got), plain)
        _check_streams(oracle, key, 0, 8, 1, g, e, ("off", store))


def test_option_rejects_other_values(ctx, oracle, opts):
    rows, cols = 5, 70
    d, _ = _raster(ctx, _img(oracle, rows, cols))
    for mode in (0, 1, 2):
        opts(mode)
        for bad in (3, -1):
            with pytest.raises(pybic.BicError) as err:
                ctx.set_sample_predict(bad)
            assert err.value.code == pybic.BIC_EINVAL
        got = ctx.bitplanes_u8(_view(d, rows, cols), cols=cols)
        ctx.sync()
        assert np.array_equal(as_u64(got), _planes(oracle, rows, cols, mode, 0)[1]), mode  # the setting stayed


def test_other_sample_kinds_ignore_the_option(ctx, oracle, staged, opts):
    """mode 2 on: two-byte samples, RGB pixels and P4 rasters still give the option-off oracle streams"""
    opts(2)

    def check(planes, cols, g, e, tag):
        for k in range(planes.shape[0]):
            for coder, (out, bits) in ((G, g), (E, e)):
                eb, est, _ = oracle.encode_plane(planes[k], cols, 1, coder)
                nb = int(as_u64(bits)[k])
                assert nb == eb and stream_bytes(out[k], nb) == est.tobytes(), (tag, k, coder)

    rows, cols = 20, 4096
    img16 = oracle.gen_bytes(0x16B17, 2 * rows * cols).view(np.uint16).reshape(rows, cols)
    d = ctx.torch.from_numpy(img16.astype("<u2").view(np.uint8).reshape(rows, 2 * cols).copy()).to(ctx.dev)
    _, g, e = ctx.encode_gray16(d, rows=rows, cols=cols, store_planes=False)
    ctx.sync()
    check(oracle.bitplanes(img16, 16), cols, g, e, "gray16")

    rows, cols = 9, 1366
    rgb = oracle.gen_bytes(0x4B6B, rows * cols * 3).reshape(rows, cols, 3)
    d = ctx.torch.from_numpy(rgb.reshape(rows, 3 * cols).copy()).to(ctx.dev)
    wpr = ((cols + 63) // 64 + 1) & ~1
    _, g, e = ctx.encode_rgb(d, rows=rows, cols=cols, wpr=wpr)
    ctx.sync()
    check(np.concatenate([oracle.bitplanes(np.ascontiguousarray(rgb[:, :, c]), 8) for c in range(3)]), cols, g, e, "rgb")

    rows, cols = 20, 4096
    bits = oracle.gen_bytes(0xB17, rows * cols // 8).reshape(rows, cols // 8)
    _, g, e = ctx.encode_pbm(ctx.torch.from_numpy(bits.reshape(-1).copy()).to(ctx.dev), rows, cols)
    ctx.sync()
    plane = bits.reshape(rows, cols // 64, 8).astype(np.uint64)
    word = np.zeros((rows, cols // 64), np.uint64)
    for b in range(8):  # big-endian: the first byte holds the leftmost pixels
        word |= plane[:, :, b] << np.uint64(56 - 8 * b)
    check(word[None], cols, g, e, "pbm")
