"""BIC_OPT_COLOR_TRANSFORM on the device. The defining property: every output of a participating call with the
option on equals, bit for bit, what the same call gives with the option off on the image T(img). So every
expected plane, stream, bit count, offset and row index here is the oracle's on colour_ref.forward(img, mode)
(Gray-coded with graycode_ref.gray where BIC_OPT_GRAY_CODE is on), never the code under test's; the decode
tests take the device encoder's streams and expect the input image, byte for byte.
The full matrix of modes {1, 2} x Gray code {off, on} runs at (33, 4096); elsewhere mode 1 with the Gray code
and mode 2 without (MODES2)."""
import contextlib

import numpy as np
import pytest

import pybic
from colour_ref import forward, inverse
from graycode_ref import gray, ungray
from pybic import CODER_EG, CODER_GOLOMB, as_u64, stream_bytes

pytestmark = pytest.mark.gpu

MATRIX = [(1, False), (1, True), (2, False), (2, True)]
MODES2 = [(1, True), (2, False)]
KINDS = ["uniform24", "edge"]
GUARD = 0x5A
_IMG, _PLANES, _STREAM = {}, {}, {}


@pytest.fixture
def staged(ctx):
    ctx.set_encoder("staged")
    yield
    ctx.set_encoder("auto")


@contextlib.contextmanager
def _opts(ctx, mode, gc):
    ctx.set_color_transform(mode)
    ctx.set_gray_code(gc)
    try:
        yield
    finally:
        ctx.set_color_transform(0)
        ctx.set_gray_code(False)


def _img(oracle, kind, rows, cols):
    """uniform24: independent uniform bytes (as tests/test_gpu_rgb.py). edge: samples drawn from {0, 1, 127, 128,
    254, 255}, the first eight pixels (0,255,255), (255,0,0), (128,0,127), (0,128,255) twice: borrows and the fold
    extreme d = -128 in neighbouring bytes of one dword."""
    key = (kind, rows, cols)
    if key not in _IMG:
        seed = 0x434C5200 + 131 * rows + cols
        a = oracle.gen_bytes(seed, 3 * rows * cols).reshape(rows, cols, 3).copy()
        if kind == "edge":
            a = np.array([0, 1, 127, 128, 254, 255], np.uint8)[a % 6]
            a[0, :8] = [(0, 255, 255), (255, 0, 0), (128, 0, 127), (0, 128, 255)] * 2
        a.setflags(write=False)
        _IMG[key] = a
    return _IMG[key]


def _planes24(oracle, kind, rows, cols, mode, gc):
    """-> (key, the 24 expected planes: plane 8 c + b = bit b of channel c of T(img), Gray-coded if gc)"""
    key = (kind, rows, cols, mode, bool(gc))
    if key not in _PLANES:
        v = forward(_img(oracle, kind, rows, cols), mode)
        if gc:
            v = gray(v)
        _PLANES[key] = np.concatenate([oracle.bitplanes(np.ascontiguousarray(v[:, :, c]), 8) for c in range(3)])
    return key, _PLANES[key]


def _stream(oracle, key, p, pred, coder):
    q = (key, p, pred, coder)
    if q not in _STREAM:
        eb, est, _ = oracle.encode_plane(_PLANES[key][p], key[2], pred, coder)
        _STREAM[q] = (eb, est.tobytes())
    return _STREAM[q]


def _raster(ctx, img, pitch=None, off=0):
    """the pixels as raster bytes, rows of `pitch` bytes, `off` bytes into a larger device buffer whose other bytes
    hold a pattern that must never reach a plane"""
    rows, cols, _ = img.shape
    pitch = pitch or 3 * cols
    buf = np.full(off + rows * pitch + 256, GUARD, np.uint8)
    r = np.full((rows, pitch), 0xC3, np.uint8)
    r[:, :3 * cols] = img.reshape(rows, 3 * cols)
    buf[off:off + rows * pitch] = r.reshape(-1)
    return ctx.torch.from_numpy(buf).to(ctx.dev)[off:], pitch


def _want_planes(planes24, plane0, nplanes, wpr=None):
    p = np.concatenate([planes24[8 * c + plane0:8 * c + plane0 + nplanes] for c in range(3)])
    return p if wpr is None else np.pad(p, ((0, 0), (0, 0), (0, wpr - p.shape[2])))


def _even(cols):
    return ((cols + 63) // 64 + 1) // 2 * 2


def _fused_pitch(cols, extra=0):
    return (cols + 63) // 64 * 192 + extra


def _check_streams(oracle, key, plane0, nplanes, pred, g, e, tag):
    for c in range(3):
        for k in range(nplanes):
            for coder, res in ((0, g), (1, e)):
                eb, est = _stream(oracle, key, 8 * c + plane0 + k, pred, coder)
                nb = int(as_u64(res[1])[c * nplanes + k])
                assert nb == eb, (tag, "channel", c, "plane", plane0 + k, "coder", coder, nb, eb)
                assert stream_bytes(res[0][c * nplanes + k], nb) == est, (tag, c, plane0 + k, coder)


def _encode(ctx, oracle, kind, rows, cols, mode, gc, pred=1, store=False, plane0=0, nplanes=8, pitch=None, off=0,
            wpr=None):
    """one bic_encode_rgb call with the options on against the oracle on T(img)"""
    key, planes24 = _planes24(oracle, kind, rows, cols, mode, gc)
    d, pitch = _raster(ctx, _img(oracle, kind, rows, cols), pitch, off)
    pl = None
    if store and wpr:
        pl = ctx.torch.zeros((3 * nplanes, rows, wpr), dtype=ctx.torch.int64, device=ctx.dev)
    with _opts(ctx, mode, gc):
        planes, g, e = ctx.encode_rgb(d, rows=rows, cols=cols, pitch=pitch, nplanes=nplanes, plane0=plane0,
                                      predict=bool(pred), store_planes=store, planes=pl, wpr=wpr)
        ctx.sync()
    tag = (kind, rows, cols, "mode", mode, "gc", gc, pred, store, plane0, nplanes, pitch, off, wpr)
    if store:
        assert np.array_equal(as_u64(planes), _want_planes(planes24, plane0, nplanes, wpr)), tag
    _check_streams(oracle, key, plane0, nplanes, pred, g, e, tag)


# ---- encode: streams and bit counts bit for bit ------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode,gc", MATRIX)
def test_one_strip(ctx, oracle, staged, mode, gc, kind):
    """(33, 4096), planes NULL, predict, both streams into slots: the EG-source path; the full matrix"""
    _encode(ctx, oracle, kind, 33, 4096, mode, gc)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode,gc", MODES2)
def test_two_strips(ctx, oracle, staged, mode, gc, kind):
    """(24, 8192): the next-segment byte across a strip boundary and the pixel before the strip, the two places
    where T's non-linearity shows; with the EG source and with the planes returned"""
    _encode(ctx, oracle, kind, 24, 8192, mode, gc)
    _encode(ctx, oracle, kind, 24, 8192, mode, gc, store=True)


@pytest.mark.parametrize("mode,gc", MODES2)
def test_partial_strip(ctx, oracle, staged, mode, gc):
    """(37, 4100): a partial last strip; planes returned and compared, and the residual buffer (planes NULL)"""
    for kind in KINDS:
        for store in (True, False):
            _encode(ctx, oracle, kind, 37, 4100, mode, gc, store=store, pitch=_fused_pitch(4100), wpr=_even(4100))


@pytest.mark.parametrize("off", [1, 13])
@pytest.mark.parametrize("mode,gc", MODES2)
def test_misaligned(ctx, oracle, staged, mode, gc, off):
    for store in (False, True):
        _encode(ctx, oracle, "edge", 21, 4096, mode, gc, store=store, pitch=3 * 4096 + 7, off=off)


@pytest.mark.parametrize("mode,gc", MODES2)
def test_no_prediction(ctx, oracle, staged, mode, gc):
    """predict = 0: the residual-buffer route (planes NULL) and the planes returned"""
    for kind in KINDS:
        _encode(ctx, oracle, kind, 33, 4096, mode, gc, pred=0)
    _encode(ctx, oracle, "edge", 33, 4096, mode, gc, pred=0, store=True)


@pytest.mark.parametrize("plane0,nplanes", [(3, 2), (7, 1)])
@pytest.mark.parametrize("mode,gc", MODES2)
def test_plane_ranges(ctx, oracle, staged, mode, gc, plane0, nplanes):
    for store in (False, True):
        _encode(ctx, oracle, "edge", 33, 4096, mode, gc, store=store, plane0=plane0, nplanes=nplanes)
    _encode(ctx, oracle, "uniform24", 24, 8192, mode, gc, plane0=plane0, nplanes=nplanes)


@pytest.mark.parametrize("mode,gc", MODES2)
def test_packed_and_index(ctx, oracle, staged, mode, gc):
    """(40, 4096): the packed streams, their offsets and the row index are the oracle's of T(img)"""
    rows, cols, kind = 40, 4096, "edge"
    key, planes24 = _planes24(oracle, kind, rows, cols, mode, gc)
    d, pitch = _raster(ctx, _img(oracle, kind, rows, cols))
    idx = ctx.empty_i64(24 * rows * 2)
    with _opts(ctx, mode, gc):
        _, g, e = ctx.encode_rgb_packed(d, rows=rows, cols=cols, pitch=pitch, store_planes=False, row_index=idx)
        ctx.sync()
    for coder, (out, bits, off) in ((0, g), (1, e)):
        words, offs = [], [0]
        for p in range(24):
            eb, est = _stream(oracle, key, p, 1, coder)
            words.append(est)
            offs.append(offs[-1] + (eb + 63) // 64)
            assert int(as_u64(bits)[p]) == eb, (coder, p)
        assert list(as_u64(off)) == offs, coder
        assert as_u64(out)[:offs[-1]].tobytes() == b"".join(words), coder
    ri = as_u64(idx).reshape(24, 2 * rows)
    for p in range(24):
        assert np.array_equal(ri[p], oracle.row_index(planes24[p], cols, 1)), p


@pytest.mark.parametrize("mode,gc", MODES2)
def test_forced_encoder(ctx, oracle, mode, gc):
    """single-kernel: the extraction (bic_bitplanes_rgb) and then the forced encoder"""
    ctx.set_encoder("single-kernel")
    try:
        for store in (True, False):
            _encode(ctx, oracle, "edge", 20, 4096, mode, gc, store=store)
    finally:
        ctx.set_encoder("auto")


@pytest.mark.parametrize("mode,gc", MODES2)
def test_odd_wpr(ctx, oracle, staged, mode, gc):
    """65 words per row: the fallback extraction under the staged encoder"""
    for store in (True, False):
        _encode(ctx, oracle, "edge", 37, 4100, mode, gc, store=store, pitch=_fused_pitch(4100))


@pytest.mark.parametrize("mode,gc", MODES2)
def test_wide_rows(ctx, oracle, staged, mode, gc):
    """(5, 16448): beyond 16384 columns, the extraction and the multi-pass encoder"""
    _encode(ctx, oracle, "edge", 5, 16448, mode, gc, store=True)
    _encode(ctx, oracle, "uniform24", 5, 16448, mode, gc)


def test_launch_names(ctx, oracle, staged):
    """bic_prof_collect names the same launches with the option on as off: still one count kernel where the
    one-read path applies, the extraction where it does not"""
    ctx.sync()
    ctx.prof_collect()
    ctx.prof_enable(True)
    cases = [dict(rows=33, cols=4096), dict(rows=33, cols=4096, store=True), dict(rows=24, cols=8192),
             dict(rows=21, cols=4096, pitch=3 * 4096 + 7, off=13),
             dict(rows=37, cols=4100, store=True, pitch=_fused_pitch(4100), wpr=_even(4100)),
             dict(rows=37, cols=4100, pitch=_fused_pitch(4100)), dict(rows=5, cols=16448)]
    try:
        ctx.prof_only(None)
        for kw in cases:
            kw = dict(kw)
            rows, cols = kw.pop("rows"), kw.pop("cols")
            names = {}
            for mode, gc in ((0, False), (1, True), (2, False)):
                ctx.prof_collect()
                _encode(ctx, oracle, "edge", rows, cols, mode, gc, **kw)
                names[mode] = {k: v[0] for k, v in ctx.prof_collect().items()}
            assert names[1] == names[0] and names[2] == names[0], (rows, cols, kw, names)
            fused = cols <= 16384 and kw.get("wpr", (cols + 63) // 64) % 2 == 0
            assert names[0].get("bitplanes_count", 0) == (1 if fused else 0), names[0]
            assert names[0].get("bitplanes_rgb", 0) == (0 if fused else 1), names[0]
    finally:
        ctx.prof_only(None)
        ctx.prof_enable(False)


# ---- the extraction alone and its inverse ------------------------------------------------------------------

@pytest.mark.parametrize("off", [0, 3])
@pytest.mark.parametrize("mode,gc", MODES2)
def test_bitplanes_and_back(ctx, oracle, mode, gc, off):
    """bic_bitplanes_rgb gives the oracle's planes of T(img); bic_planes_to_rgb gives img back (16-byte stores at
    offset 0 with an aligned pitch, byte stores at offset 3), and writes nothing beyond a row's 3 cols bytes"""
    rows, cols = 21, 1000
    for kind in KINDS:
        img = _img(oracle, kind, rows, cols)
        key, planes24 = _planes24(oracle, kind, rows, cols, mode, gc)
        pitch = 3 * cols + (8 if off == 0 else 10)
        assert (pitch % 16 == 0) == (off == 0)
        d, _ = _raster(ctx, img, pitch, off)
        buf = ctx.torch.full((off + rows * pitch + 64,), GUARD, dtype=ctx.torch.uint8, device=ctx.dev)
        with _opts(ctx, mode, gc):
            got = ctx.bitplanes_rgb(d, rows=rows, cols=cols, pitch=pitch)
            sub = ctx.bitplanes_rgb(d, rows=rows, cols=cols, pitch=pitch, plane0=3, nplanes=2)
            ctx.planes_to_rgb(got, cols, out=buf[off:], pitch=pitch)
            ctx.sync()
        assert np.array_equal(as_u64(got), planes24), (kind, mode, gc, off)
        assert np.array_equal(as_u64(sub), _want_planes(planes24, 3, 2)), (kind, mode, gc, off)
        b = buf.cpu().numpy()
        body = b[off:off + rows * pitch].reshape(rows, pitch)
        assert np.array_equal(body[:, :3 * cols], img.reshape(rows, 3 * cols)), (kind, mode, gc, off)
        assert (body[:, 3 * cols:] == GUARD).all() and (b[:off] == GUARD).all() and (b[off + rows * pitch:] == GUARD).all()


# ---- decode -------------------------------------------------------------------------------------------------

def _header_formula(img, mode, gc, plane0, nplanes):
    """include/bic.h: the channel samples assembled from the planes of the range (uncovered bits 0, after the
    un-Gray step and its mask), then R = (unfold(R') + G') & 0xFF, B likewise, G = G'"""
    m = np.uint8(((1 << nplanes) - 1) << plane0)
    t = forward(img, mode)
    t = (ungray(gray(t) & m, 8) & m) if gc else (t & m)
    return inverse(t, mode)


def _round_trip(ctx, oracle, kind, rows, cols, mode, gc, plane0=0, nplanes=8):
    img = _img(oracle, kind, rows, cols)
    src, spitch = _raster(ctx, img, _fused_pitch(cols))
    n3 = 3 * nplanes
    idx = ctx.empty_i64(n3 * rows * 2)
    want = _header_formula(img, mode, gc, plane0, nplanes)
    if (plane0, nplanes) == (0, 8):
        assert np.array_equal(want, img)
    p16 = (3 * cols + 15) // 16 * 16 + 16
    with _opts(ctx, mode, gc):
        _, g, e = ctx.encode_rgb_packed(src, rows=rows, cols=cols, pitch=spitch, plane0=plane0, nplanes=nplanes,
                                        store_planes=False, row_index=idx, wpr=_even(cols))
        p00 = ctx.torch.from_numpy(pybic.rgb_p00(mode, gc, img[0, 0], plane0, nplanes)).to(ctx.dev)
        outs = []
        for coder, (out, bits, off) in ((CODER_GOLOMB, g), (CODER_EG, e)):
            for doff, pitch in ((0, p16), (1, 3 * cols + 5)):  # the 16-byte stores / the byte stores
                buf = ctx.torch.full((doff + rows * pitch + 64,), GUARD, dtype=ctx.torch.uint8, device=ctx.dev)
                ctx.decode_rgb(coder, out, bits, nplanes, rows, cols, True, word_off=off,
                               row_index=idx if coder == CODER_GOLOMB else None, p00=p00, plane0=plane0,
                               out=buf[doff:], pitch=pitch)
                outs.append((coder, doff, pitch, buf))
        ctx.sync()
    for coder, doff, pitch, buf in outs:
        b = buf.cpu().numpy()
        body = b[doff:doff + rows * pitch].reshape(rows, pitch)
        bad = np.argwhere(body[:, :3 * cols] != want.reshape(rows, 3 * cols))
        assert bad.size == 0, ("first differing (row, byte)", bad[:4].tolist(), len(bad), kind, mode, gc, coder, doff)
        assert (body[:, 3 * cols:] == GUARD).all(), ("bytes past a row's 3 * cols", coder, doff, pitch)
        assert (b[:doff] == GUARD).all() and (b[doff + rows * pitch:] == GUARD).all()


@pytest.mark.parametrize("rows,cols", [(33, 4096), (37, 4100)])
@pytest.mark.parametrize("mode,gc", MODES2)
def test_decode_round_trip(ctx, oracle, staged, mode, gc, rows, cols):
    """bic_encode_rgb_packed -> bic_decode_rgb returns the image byte for byte, from the Golomb and from the EG
    streams, through the 16-byte stores and the byte stores; p00 from bic_rgb_p00"""
    for kind in KINDS:
        _round_trip(ctx, oracle, kind, rows, cols, mode, gc)


@pytest.mark.parametrize("mode,gc", MATRIX)
def test_decode_partial_range(ctx, oracle, staged, mode, gc):
    """planes 3 and 4 only: the header's formula, computed in numpy"""
    _round_trip(ctx, oracle, "edge", 33, 4096, mode, gc, plane0=3, nplanes=2)


# ---- state --------------------------------------------------------------------------------------------------

def test_option_state(ctx, oracle, staged):
    rows, cols, kind = 33, 4096, "edge"
    _encode(ctx, oracle, kind, rows, cols, 2, False)
    _encode(ctx, oracle, kind, rows, cols, 0, False)  # switched off: the option-off oracle result
    ctx.set_color_transform("subtract_green")
    try:
        for bad in (3, -1):
            with pytest.raises(pybic.BicError) as e:
                ctx.set_color_transform(bad)
            assert e.value.code == pybic.BIC_EINVAL
        with pytest.raises(pybic.BicError):
            ctx.set_color_transform("rct")
        # mode 1 is still in force
        key, _ = _planes24(oracle, kind, rows, cols, 1, False)
        d, pitch = _raster(ctx, _img(oracle, kind, rows, cols))
        _, g, e = ctx.encode_rgb(d, rows=rows, cols=cols, pitch=pitch, store_planes=False)
        ctx.sync()
        _check_streams(oracle, key, 0, 8, 1, g, e, "mode 1 after rejected values")
        # the gray calls ignore the option
        gimg = np.ascontiguousarray(_img(oracle, kind, rows, cols)[:, :, 0])
        P = oracle.bitplanes(gimg, 8)
        _, (og, bg), (oe, be) = ctx.encode_gray(ctx.torch.from_numpy(gimg).to(ctx.dev), store_planes=False)
        ctx.sync()
        for k in range(8):
            for coder, out, bits in ((0, og, bg), (1, oe, be)):
                eb, est, _ = oracle.encode_plane(P[k], cols, 1, coder)
                nb = int(as_u64(bits)[k])
                assert nb == eb and stream_bytes(out[k], nb) == est.tobytes(), (k, coder)
    finally:
        ctx.set_color_transform("none")
    _encode(ctx, oracle, kind, rows, cols, 0, False)
