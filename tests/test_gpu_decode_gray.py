"""bic_decode_gray: streams -> gray samples in one call (the row decoders into the context's D buffer, then
unmed's column pass forming the samples itself). Every comparison is bit-exact against the input samples
masked to the decoded planes' bits -- never against something the code under test produced, except where
a test says it compares the one call with the two calls it replaces."""
import ctypes as C

import numpy as np
import pytest

import pybic
from pybic import CODER_EG, CODER_EG_ADAPTIVE, CODER_GOLOMB

pytestmark = pytest.mark.gpu

G, E, A = CODER_GOLOMB, CODER_EG, CODER_EG_ADAPTIVE
_IMG = {}


def _img(oracle, kind, rows, cols):
    """seeded inputs, made once: uniform8 / uniform16 (every plane p = 0.5), smooth8 (a ramp with a little
    noise: all-zero high planes, long runs in the middle ones, so rows of k = 0, k = 1 and mixed k occur)"""
    key = (kind, rows, cols)
    if key not in _IMG:
        seed = 0xD6A7 + 131 * rows + cols
        if kind == "uniform8":
            a = oracle.gen_bytes(seed, rows * cols).reshape(rows, cols).copy()
        elif kind == "uniform16":
            a = oracle.gen_bytes(seed, 2 * rows * cols).view(np.uint16).reshape(rows, cols).copy()
        else:
            i, j = np.mgrid[0:rows, 0:cols]
            noise = oracle.gen_bytes(seed, rows * cols).reshape(rows, cols) % 5
            a = ((3 * i + j // 7 + noise) % 200).astype(np.uint8)
        a.setflags(write=False)
        _IMG[key] = a
    return _IMG[key]


def _dev(ctx, a):
    """a host array (the shared, read-only inputs) -> its own device tensor"""
    return ctx.torch.from_numpy(np.array(a)).to(ctx.dev)


def _mask(plane0, nplanes):
    return ((1 << nplanes) - 1) << plane0


def _p00(ctx, img, plane0, nplanes):
    v = int(img[0, 0])
    return ctx.torch.tensor([(v >> (plane0 + b)) & 1 for b in range(nplanes)], dtype=ctx.torch.uint8, device=ctx.dev)


def _encode8(ctx, img, coder, pred, packed, plane0=0, nplanes=8):
    """the device encoder's streams of an 8-bit image -> (streams, plane_bits, word_off or None, row index or
    None): packed with the index the encoder writes, or slots with the index from bic_row_index"""
    rows, cols = img.shape
    d = _dev(ctx, img)
    want = dict(golomb=coder == G, eg=coder == E)
    if packed:
        idx = ctx.empty_i64(nplanes * rows * 2) if coder == G else None
        _, g, e = ctx.encode_gray_packed(d, nplanes=nplanes, plane0=plane0, predict=bool(pred), row_index=idx, **want)
        out, bits, off = g if coder == G else e
        return out, bits, off, idx
    planes, g, e = ctx.encode_gray(d, nplanes=nplanes, plane0=plane0, predict=bool(pred), **want)
    out, bits = g if coder == G else e
    idx = ctx.row_index(planes, cols, bool(pred)) if coder == G else None
    return out, bits, None, idx


def _decode8(ctx, img, enc, coder, pred, plane0=0, nplanes=8, **kw):
    out, bits, off, idx = enc
    rows, cols = img.shape
    return ctx.decode_gray(coder, out, bits, nplanes, rows, cols, bool(pred), word_off=off, row_index=idx,
                           p00=_p00(ctx, img, plane0, nplanes) if pred else None, plane0=plane0, **kw)


# 1. round trip, 8-bit. rows straddle the column chunk of 64 (rows % 64 == 0: the Golomb row kernel forms the
#    chunk totals itself, otherwise k_col_chunks does); cols: one segment, one word, one word and a bit, trail
#    bits with rows no multiple of 16 bytes (byte stores), 64 words, more than 64 words, the widest row
@pytest.mark.parametrize("rows,cols,coder,pred,packed,kind", [
    (1, 1, G, 1, True, "uniform8"),
    (63, 64, G, 1, False, "uniform8"),
    (64, 65, G, 1, True, "uniform8"),
    (65, 1000, G, 1, True, "uniform8"),
    (130, 4096, G, 1, False, "uniform8"),
    (64, 4160, G, 1, True, "uniform8"),
    (65, 16384, G, 1, True, "uniform8"),
    (130, 1000, G, 0, True, "uniform8"),
    (64, 4096, G, 0, False, "uniform8"),
    (63, 4160, G, 0, False, "uniform8"),
    (128, 4096, G, 1, True, "smooth8"),
    (130, 1000, G, 1, False, "smooth8"),
    (1, 64, E, 1, True, "uniform8"),
    (63, 65, E, 1, False, "uniform8"),
    (64, 1000, E, 1, True, "uniform8"),
    (65, 4096, E, 0, True, "uniform8"),
    (130, 4160, E, 1, True, "uniform8"),
    (64, 16384, E, 1, False, "uniform8"),
    (130, 1, E, 0, False, "uniform8"),
    (65, 1000, E, 1, True, "smooth8"),
])
def test_round_trip_8bit(ctx, oracle, rows, cols, coder, pred, packed, kind):
    img = _img(oracle, kind, rows, cols)
    enc = _encode8(ctx, img, coder, pred, packed)
    back = _decode8(ctx, img, enc, coder, pred)
    ctx.sync()
    assert back.shape == (rows, cols)
    assert np.array_equal(back.cpu().numpy(), img)


# 2. plane ranges: stream b sets bit plane0 + b, bits no plane covers are 0
@pytest.mark.parametrize("plane0,nplanes", [(0, 8), (2, 3), (7, 1)])
@pytest.mark.parametrize("coder", [G, E])
def test_plane_ranges(ctx, oracle, plane0, nplanes, coder):
    img = _img(oracle, "uniform8", 70, 1000)
    enc = _encode8(ctx, img, coder, 1, True, plane0, nplanes)
    back = _decode8(ctx, img, enc, coder, 1, plane0, nplanes)
    ctx.sync()
    got = back.cpu().numpy()
    assert (got & ~np.uint8(_mask(plane0, nplanes)) == 0).all()
    assert np.array_equal(got, img & np.uint8(_mask(plane0, nplanes)))


# 3. two-byte samples in both byte orders; (6, 5) crosses the byte boundary
@pytest.mark.parametrize("be", [1, 0])
@pytest.mark.parametrize("plane0,nplanes", [(0, 16), (6, 5), (8, 8)])
@pytest.mark.parametrize("rows,cols", [(40, 4096), (65, 1000)])
def test_round_trip_16bit(ctx, oracle, rows, cols, plane0, nplanes, be):
    img = _img(oracle, "uniform16", rows, cols)
    order = ">u2" if be else "<u2"
    raster = np.ascontiguousarray(img.astype(order)).view(np.uint8).reshape(rows, 2 * cols)
    idx = ctx.empty_i64(nplanes * rows * 2)
    _, (og, bg, fg), (oe, be_, fe) = ctx.encode_gray16_packed(
        _dev(ctx, raster), rows=rows, cols=cols, nplanes=nplanes, plane0=plane0,
        big_endian=bool(be), row_index=idx, store_planes=False)
    p00 = _p00(ctx, img, plane0, nplanes)
    exp = (img & np.uint16(_mask(plane0, nplanes))).astype(order).view(np.uint8).reshape(rows, 2 * cols)
    for coder, out, bits, off in ((G, og, bg, fg), (E, oe, be_, fe)):
        back = ctx.decode_gray(coder, out, bits, nplanes, rows, cols, True, word_off=off, row_index=idx, p00=p00,
                               plane0=plane0, sample_bytes=2, big_endian=bool(be))
        ctx.sync()
        assert back.shape == (rows, 2 * cols)
        assert np.array_equal(back.cpu().numpy(), exp), coder


# 4. alignment and pitch: only the rows' first cols * sample_bytes bytes are written
_ENC_ALIGN = {}


@pytest.mark.parametrize("off", [0, 3, 16])
@pytest.mark.parametrize("pitch_kind", ["tight", "odd", "mult16"])
@pytest.mark.parametrize("bps,rows,cols", [(1, 66, 1000), (2, 20, 200)])
def test_alignment_and_pitch(ctx, oracle, bps, rows, cols, pitch_kind, off):
    img = _img(oracle, "uniform8" if bps == 1 else "uniform16", rows, cols)
    nplanes = 8 * bps
    if bps not in _ENC_ALIGN:
        idx = ctx.empty_i64(nplanes * rows * 2)
        if bps == 1:
            _ENC_ALIGN[bps] = _encode8(ctx, img, G, 1, True)
        else:
            _, (og, bg, fg), _e = ctx.encode_gray16_packed(_dev(ctx, img.view(np.int16)),
                                                           big_endian=False, row_index=idx, eg=False)
            _ENC_ALIGN[bps] = (og, bg, fg, idx)
    out, bits, woff, idx = _ENC_ALIGN[bps]
    line = cols * bps
    pitch = {"tight": line, "odd": line + 5, "mult16": (line + 15) // 16 * 16}[pitch_kind]
    buf = ctx.torch.full((off + rows * pitch + 64,), 0x5A, dtype=ctx.torch.uint8, device=ctx.dev)
    ctx.decode_gray(G, out, bits, nplanes, rows, cols, True, word_off=woff, row_index=idx,
                    p00=_p00(ctx, img, 0, nplanes), sample_bytes=bps, big_endian=True, out=buf[off:], pitch=pitch)
    ctx.sync()
    got = buf.cpu().numpy()
    assert (got[:off] == 0x5A).all()
    body = got[off:off + rows * pitch].reshape(rows, pitch)
    exp = img if bps == 1 else img.astype(">u2").view(np.uint8).reshape(rows, line)
    assert np.array_equal(body[:, :line], exp)
    assert (body[:, line:] == 0x5A).all()
    assert (got[off + rows * pitch:] == 0x5A).all()  # nothing past the last row


# 5. the oracle's own streams (no device encoder): slots, the indices from the oracle's coder states
@pytest.mark.parametrize("n,rows,cols", [(3, 50, 300), (2, 20, 16384)])
@pytest.mark.parametrize("coder", [G, E, A])
def test_oracle_streams(ctx, oracle, n, rows, cols, coder):
    img = _img(oracle, "uniform8", rows, cols)
    P = oracle.bitplanes(img, n)
    slot = ctx.slot_words(rows, cols, coder)
    S = np.zeros((n, slot), np.uint64)
    bits = np.zeros(n, np.uint64)
    idx = np.zeros((n, 2 * rows), np.uint64)
    for k in range(n):
        b, st, _ = oracle.encode_plane(P[k], cols, 1, coder)
        S[k, :len(st) // 8] = np.frombuffer(st.tobytes(), np.uint64)  # slot bytes = the bit stream
        bits[k] = b
        if coder == G:
            idx[k] = oracle.row_index(P[k], cols, 1)
        elif coder == A:
            idx[k] = oracle.egad_row_index(P[k], cols, 1)
    back = ctx.decode_gray(coder, ctx.to_dev(S), ctx.to_dev(bits), n, rows, cols, True,
                           row_index=None if coder == E else ctx.to_dev(idx.reshape(-1)), p00=_p00(ctx, img, 0, n))
    ctx.sync()
    assert np.array_equal(back.cpu().numpy(), img & np.uint8(_mask(0, n)))


# 6. the adaptive EG coder
@pytest.mark.parametrize("rows,cols", [(70, 65), (33, 4096)])
@pytest.mark.parametrize("pred", [1, 0])
def test_eg_adaptive(ctx, oracle, rows, cols, pred):
    img = _img(oracle, "uniform8", rows, cols)
    planes = ctx.bitplanes_u8(_dev(ctx, img), nplanes=8)
    out, bits = ctx.encode_planes(planes, cols, bool(pred), A)
    idx = ctx.egad_row_index(planes, cols, bool(pred))
    back = ctx.decode_gray(A, out, bits, 8, rows, cols, bool(pred), row_index=idx,
                           p00=_p00(ctx, img, 0, 8) if pred else None)
    ctx.sync()
    assert np.array_equal(back.cpu().numpy(), img)


# 7. the one call == the two calls it replaces, byte for byte (and both == the image)
@pytest.mark.parametrize("coder", [G, E])
def test_one_call_equals_two_calls(ctx, oracle, coder):
    rows, cols = 130, 4160
    img = _img(oracle, "uniform8", rows, cols)
    out, bits, off, idx = _encode8(ctx, img, coder, 1, True)
    p00 = _p00(ctx, img, 0, 8)
    planes = ctx.decode_planes(coder, out, bits, 8, rows, cols, True, word_off=off, row_index=idx, p00=p00)
    two = ctx.planes_to_gray(planes, cols)
    one = ctx.decode_gray(coder, out, bits, 8, rows, cols, True, word_off=off, row_index=idx, p00=p00)
    ctx.sync()
    assert ctx.torch.equal(one, two)
    assert np.array_equal(one.cpu().numpy(), img)


# 8. a malformed stream is BIC_EDATA at the sync, and the context decodes the good stream afterwards
@pytest.mark.parametrize("coder", [G, E])
def test_malformed_stream(ctx, oracle, coder):
    img = _img(oracle, "uniform8", 30, 500)
    out, bits, off, idx = _encode8(ctx, img, coder, 1, True)
    ctx.sync()
    bad = bits.clone()
    bad[0] -= 1  # the stream is one bit longer than claimed
    _decode8(ctx, img, (out, bad, off, idx), coder, 1)
    with pytest.raises(pybic.BicError) as e:
        ctx.sync()
    assert e.value.code == pybic.BIC_EDATA
    back = _decode8(ctx, img, (out, bits, off, idx), coder, 1)
    ctx.sync()
    assert np.array_equal(back.cpu().numpy(), img)


# 9. refusals
def test_rejects(ctx):
    t, b, idx = ctx.empty_i64(8, 64), ctx.empty_i64(8), ctx.empty_i64(8 * 10 * 2)

    def einval(fn):
        with pytest.raises(pybic.BicError) as e:
            fn()
        assert e.value.code == pybic.BIC_EINVAL

    einval(lambda: ctx.decode_gray(G, t, b, 8, 10, 64))  # Golomb without a row index
    einval(lambda: ctx.decode_gray(A, t, b, 8, 10, 64))  # so does the adaptive coder
    einval(lambda: ctx.decode_gray(E, t, b, 8, 10, 20000))  # rows wider than 16384 columns
    einval(lambda: ctx.decode_gray(E, t, b, 8, 10, 64, sample_bytes=3))
    einval(lambda: ctx.decode_gray(E, t, b, 8, 10, 64, plane0=1))  # plane0 + nplanes = 9, one-byte samples
    einval(lambda: ctx.decode_gray(E, t[:4], b[:4], 4, 10, 64, plane0=13, sample_bytes=2))  # 17, two-byte samples
    einval(lambda: ctx.decode_gray(E, t, b, 8, 10, 64, pitch=63))
    einval(lambda: ctx.decode_gray(E, t, b, 8, 10, 64, sample_bytes=2, pitch=127))
    ctx._bind_stream()
    rc = ctx.lib.bic_decode_gray(ctx.h, G, C.c_void_p(t.data_ptr()), 64, None, C.c_void_p(b.data_ptr()),
                                 C.c_void_p(idx.data_ptr()), 0, 8, 10, 64, 1, None, 1, 1, None, 64)  # NULL gray
    assert rc == pybic.BIC_EINVAL
    ctx.sync()


def test_no_rows(ctx):
    """rows = 0: BIC_OK, nothing written"""
    t, b = ctx.empty_i64(8, 64), ctx.empty_i64(8)
    buf = ctx.torch.full((256,), 0x5A, dtype=ctx.torch.uint8, device=ctx.dev)
    ctx.decode_gray(E, t, b, 8, 0, 64, out=buf, pitch=64)
    ctx.sync()
    assert (buf.cpu().numpy() == 0x5A).all()


# 10. the D buffer, the chunk totals and the encoder's arena share one scratch arena
def test_shared_scratch(ctx, oracle):
    big, small = _img(oracle, "uniform8", 130, 4160), _img(oracle, "uniform8", 17, 64)
    enc_big, enc_small = _encode8(ctx, big, G, 1, True), _encode8(ctx, small, E, 1, True)
    a = _decode8(ctx, big, enc_big, G, 1)
    b = _decode8(ctx, small, enc_small, E, 1)
    ctx.set_encoder("staged")
    try:  # configs[2]'s form: no planes, the count pass keeps what the emission needs in the context
        gray = _img(oracle, "uniform8", 64, 4096)
        _, (og, bg), (oe, be) = ctx.encode_gray(_dev(ctx, gray), store_planes=False)
    finally:
        ctx.set_encoder("auto")
    c = _decode8(ctx, big, enc_big, G, 1)
    d = ctx.decode_gray(E, oe, be, 8, 64, 4096, True, p00=_p00(ctx, gray, 0, 8))
    ctx.sync()
    assert np.array_equal(a.cpu().numpy(), big)
    assert np.array_equal(b.cpu().numpy(), small)
    assert np.array_equal(c.cpu().numpy(), big)
    assert np.array_equal(d.cpu().numpy(), gray)
    eb, est, _ = oracle.encode_plane(oracle.bitplanes(gray, 8)[7], 4096, 1, G)  # the encode between them
    assert int(pybic.as_u64(bg)[7]) == eb and pybic.stream_bytes(og[7], eb) == est.tobytes()


def test_profile_name(ctx, oracle):
    """the whole call is one stage of the profile, decode_gray: neither bic_decode_planes' nor
    bic_planes_to_gray's stage runs"""
    img = _img(oracle, "uniform8", 30, 500)
    enc = _encode8(ctx, img, G, 1, True)
    ctx.sync()
    ctx.prof_collect()
    ctx.prof_enable(True)
    try:
        ctx.prof_only(None)
        _decode8(ctx, img, enc, G, 1)
        got = ctx.prof_collect()
    finally:
        ctx.prof_enable(False)
    assert got["decode_gray"][0] == 1 and "decode" not in got and "planes_to_gray" not in got, got
