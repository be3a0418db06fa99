"""bic_encode_pbm / bic_encode_pbm_packed / bic_decode_pbm (P4 rasters <-> streams in one call each)
against the oracle: the planes are pbm.cpp:29-77's unpacking of the rasters (pnm_io.p4_rows_to_plane), the
streams each plane's Golomb and EG streams (bo_encode_plane), the row index bo_row_index's. Every case
also compares the one call with bic_pbm_unpack + bic_encode_planes2 on the device; nothing is compared
only with the code under test."""
import numpy as np
import pytest

import pybic
from pnm_io import p4_rows_to_plane, plane_to_p4_rows, write_pbm
from pybic import as_u64, stream_bytes

pytestmark = pytest.mark.gpu
G, E, A = pybic.CODER_GOLOMB, pybic.CODER_EG, pybic.CODER_EG_ADAPTIVE


@pytest.fixture
def staged(ctx):
    """the staged encoder (and with it the raster count kernel) at test sizes, which the automatic
    choice would give to the single kernel through the fallback"""
    ctx.set_encoder("staged")
    yield
    ctx.set_encoder("auto")


_PLANE, _STREAM, _INDEX = {}, {}, {}


def _plane(oracle, rows, cols, d, f):
    """frame f of a set: density d (a probability, "zero" or "ones"), seeded; pad bits 0"""
    key = (rows, cols, d, f)
    if key not in _PLANE:
        nb = (cols + 7) // 8
        if d == "zero":
            P = np.zeros((rows, (cols + 63) // 64), np.uint64)
        elif d == "ones":
            P = p4_rows_to_plane(np.full(rows * nb, 0xFF, np.uint8).tobytes(), rows, cols)
        else:
            P = oracle.gen_plane(0xB4 + 977 * rows + 31 * cols + 7 * f + int(d * 1000), d, rows, cols)
        assert np.array_equal(P, p4_rows_to_plane(plane_to_p4_rows(P, cols).tobytes(), rows, cols))
        _PLANE[key] = P
    return key, _PLANE[key]


def _stream(oracle, key, pred, coder):
    """a frame's expected (bits, stream bytes), computed once"""
    q = (key, pred, coder)
    if q not in _STREAM:
        eb, est, _ = oracle.encode_plane(_PLANE[key], key[1], pred, coder)
        _STREAM[q] = (eb, est.tobytes())
    return _STREAM[q]


def _index(oracle, key, pred):
    q = (key, pred)
    if q not in _INDEX:
        _INDEX[q] = oracle.row_index(_PLANE[key], key[1], pred)
    return _INDEX[q]


def _raster(ctx, planes, cols, off=0, gap=0, pad_ones=False):
    """the frames as P4 rasters `off` bytes into a 16-byte aligned device buffer, fb + gap bytes apart,
    0xA5 everywhere else -> (the view at frame 0's first byte, the stride, the host copy from there)"""
    rows, nb = planes[0].shape[0], (cols + 7) // 8
    fb = rows * nb
    stride = fb + gap
    buf = np.full(off + len(planes) * stride + 32, 0xA5, np.uint8)
    for f, P in enumerate(planes):
        r = plane_to_p4_rows(P, cols)
        if pad_ones and cols % 8:
            r[:, -1] |= np.uint8(0xFF >> (cols % 8))
        buf[off + f * stride:off + f * stride + fb] = r.reshape(-1)
    d = ctx.torch.from_numpy(buf).to(ctx.dev)
    assert d.data_ptr() % 16 == 0
    return d[off:], stride, buf[off:]


def _even(cols):
    return ((cols + 63) // 64 + 1) & ~1


def _frames(oracle, rows, cols, dens):
    keys, planes = [], []
    for f, d in enumerate(dens):
        k, P = _plane(oracle, rows, cols, d, f)
        keys.append(k)
        planes.append(P)
    return keys, planes


def _run(ctx, oracle, rows, cols, dens, off=0, gap=0, pred=1, golomb=True, eg=True, packed=False, want_planes=False,
         wpr=None, pad_ones=False, index=True):
    """one call of the encoder under test, checked against the oracle and the two calls"""
    keys, planes = _frames(oracle, rows, cols, dens)
    n, used = len(planes), (cols + 63) // 64
    wpr = wpr or _even(cols)
    d, stride, _ = _raster(ctx, planes, cols, off, gap, pad_ones)
    pl = ctx.torch.full((n, rows, wpr), -1, dtype=ctx.torch.int64, device=ctx.dev) if want_planes else None
    tag = (rows, cols, dens, off, gap, pred, golomb, eg, packed, want_planes, wpr, pad_ones)
    idx = None
    if packed:
        idx = ctx.empty_i64(n * rows * 2) if index else None
        got, g, e = ctx.encode_pbm_packed(d, rows, cols, n, stride, bool(pred), planes=pl, wpr=wpr, golomb=golomb,
                                          eg=eg, row_index=idx)
    else:
        got, g, e = ctx.encode_pbm(d, rows, cols, n, stride, bool(pred), planes=pl, wpr=wpr, golomb=golomb, eg=eg)
    ctx.sync()
    p2 = ctx.torch.stack([ctx.pbm_unpack(d[f * stride:], rows, cols, wpr) for f in range(n)])
    g2, e2 = ctx.encode_planes2(p2, cols, bool(pred), golomb, eg)
    ctx.sync()
    if want_planes:
        exp = np.zeros((n, rows, wpr), np.uint64)
        exp[:, :, :used] = np.stack(planes)
        assert np.array_equal(as_u64(got), exp), tag
        assert ctx.torch.equal(got, p2), tag
    else:
        assert got is None
    assert (g is None) == (not golomb) and (e is None) == (not eg)
    for coder, res, res2 in ((G, g, g2), (E, e, e2)):
        if res is None:
            continue
        exp = [_stream(oracle, k, pred, coder) for k in keys]
        bits, bits2 = as_u64(res[1]), as_u64(res2[1])
        print(tag, "coder", coder, "bits", list(bits), "expected", [x[0] for x in exp])
        assert list(bits) == [x[0] for x in exp], tag
        assert np.array_equal(bits, bits2), tag
        nw = [(x[0] + 63) // 64 for x in exp]
        if packed:
            offs = [int(x) for x in as_u64(res[2])]
            assert offs == [sum(nw[:f]) for f in range(n + 1)], tag
            words = as_u64(res[0])
            assert words[:offs[-1]].tobytes() == b"".join(x[1] for x in exp), tag
            for f in range(n):
                assert ctx.torch.equal(res[0][offs[f]:offs[f] + nw[f]], res2[0][f, :nw[f]]), (tag, f)
        else:
            for f in range(n):
                assert stream_bytes(res[0][f], bits[f]) == exp[f][1], (tag, f)
                assert ctx.torch.equal(res[0][f, :nw[f]], res2[0][f, :nw[f]]), (tag, f)
    if idx is not None:
        ri = as_u64(idx).reshape(n, 2 * rows)
        for f, k in enumerate(keys):
            assert np.array_equal(ri[f], _index(oracle, k, pred)), (tag, f)


SHAPES = [
    (1, 1),
    (3, 70),       # 9-byte rows: every row misaligned differently
    (17, 64),
    (33, 1000),
    (16, 4096),    # the C4 row width
    (19, 4099),    # and just over it
    (9, 8192),     # two words per lane
    (5, 16384),    # four words per lane, full last word
    (4, 16321),    # four words per lane, partial last word
    (3, 16448),    # wider than the row encoders take: the fallback
]
# (predict, golomb, eg, packed, planes returned, bytes between frames): every value of every option, twice
OPTS = [
    (1, 1, 1, 0, 0, 0),
    (0, 1, 1, 1, 1, 5),
    (1, 1, 0, 1, 0, 5),
    (0, 0, 1, 0, 1, 0),
    (1, 0, 1, 1, 1, 0),
    (0, 1, 0, 0, 0, 5),
    (1, 1, 1, 1, 1, 5),
    (0, 1, 1, 0, 0, 0),
]
PLACES = [(off, n) for off in (0, 1, 3, 13) for n in (1, 3)]


# 1. every shape at every placement (byte offset x frame count), the options rotated against the
#    placements by the shape's number so that the shapes together cross them
@pytest.mark.parametrize("si", range(len(SHAPES)), ids=[f"{r}x{c}" for r, c in SHAPES])
def test_encode_shapes(ctx, oracle, staged, si):
    rows, cols = SHAPES[si]
    for i, (off, n) in enumerate(PLACES):
        pred, golomb, eg, packed, want, gap = OPTS[(i + si) % len(OPTS)]
        if n == 1:
            dens = ((0.5, 0.02, 0.98)[(i // 2 + si) % 3],)
        else:
            dens = (0.5, 0.02, 0.98) if (i // 2 + si) % 2 else ("zero", "ones", 0.5)
        _run(ctx, oracle, rows, cols, dens, off, gap, pred, bool(golomb), bool(eg), bool(packed), bool(want),
             index=cols <= 16384)


# 2. the remaining option pairs at one misaligned shape: predict x planes x packed, both coders
@pytest.mark.parametrize("pred", [1, 0])
@pytest.mark.parametrize("want", [False, True])
@pytest.mark.parametrize("packed", [False, True])
def test_encode_options(ctx, oracle, staged, pred, want, packed):
    _run(ctx, oracle, 33, 1000, (0.5, "zero", "ones"), 3, 5, pred, True, True, packed, want)
    _run(ctx, oracle, 19, 4099, (0.02, 0.98, 0.5), 13, 0, pred, True, True, packed, want)


def test_launches(ctx, oracle, staged):
    """which kernels a call launches (bic_prof_collect's names): the raster count pass where it applies,
    bic_pbm_unpack per frame otherwise -- so that the cases above test the path they are meant to"""
    _, planes = _frames(oracle, 33, 1000, (0.5, 0.02, 0.98))
    d, stride, _ = _raster(ctx, planes, 1000, 3, 5)
    _, wide = _frames(oracle, 3, 16448, (0.5,))
    dw, _, _ = _raster(ctx, wide, 16448, 1)
    ctx.sync()
    ctx.prof_collect()
    ctx.prof_enable(True)
    try:
        ctx.prof_only(None)
        for pl in (None, True):
            ctx.encode_pbm(d, 33, 1000, 3, stride, planes=pl, wpr=16)
            got = ctx.prof_collect()
            assert got["bitplanes_count"][0] == 1 and "pbm_unpack" not in got and "encode_prefix" in got, got
        ctx.encode_pbm(d, 33, 1000, 3, stride, wpr=17)  # an odd row pitch: not the staged encoder's
        got = ctx.prof_collect()
        assert got["pbm_unpack"][0] == 3 and "bitplanes_count" not in got, got
        ctx.encode_pbm(dw, 3, 16448, 1, wpr=258)
        got = ctx.prof_collect()
        assert got["pbm_unpack"][0] == 1 and "bitplanes_count" not in got, got
        ctx.set_encoder("single-kernel")
        ctx.encode_pbm(d, 33, 1000, 3, stride, wpr=16)
        got = ctx.prof_collect()
        assert got["pbm_unpack"][0] == 3 and "bitplanes_count" not in got, got
    finally:
        ctx.prof_only(None)
        ctx.prof_enable(False)


# 3. the fallbacks: the automatic choice (a small batch: below the staged encoder's threshold), a forced
#    encoder, an odd row pitch
@pytest.mark.parametrize("enc", ["auto", "single-kernel"])
def test_fallback_encoders(ctx, oracle, enc):
    ctx.set_encoder(enc)
    try:
        for want in (False, True):
            _run(ctx, oracle, 33, 1000, (0.5, 0.02, 0.98), 3, 5, 1, True, True, True, want)
            _run(ctx, oracle, 3, 70, ("zero", "ones", 0.5), 1, 0, 0, True, True, False, want)
    finally:
        ctx.set_encoder("auto")


def test_odd_row_pitch(ctx, oracle, staged):
    for want in (False, True):
        _run(ctx, oracle, 17, 64, (0.5, 0.02, 0.98), 13, 5, 1, True, True, True, want, wpr=1)
        _run(ctx, oracle, 19, 4099, (0.5,), 1, 0, 1, True, True, False, want, wpr=65)


# 4. a pitch wider than the lanes' words: the pad words of the returned planes are written 0
def test_wide_row_pitch(ctx, oracle, staged):
    _run(ctx, oracle, 3, 70, (0.5, 0.98, 0.02), 3, 5, 1, True, True, False, True, wpr=260)
    _run(ctx, oracle, 5, 16384, (0.5,), 1, 0, 1, True, True, True, True, wpr=300)


# 5. many frames: more workgroups than one, frames at every alignment (stride 8 * 32 + 5)
def test_64_frames(ctx, oracle, staged):
    dens = tuple((0.5, 0.02, 0.98, "zero", "ones")[f % 5] for f in range(64))
    _run(ctx, oracle, 16, 256, dens, 1, 5, 1, True, True, True, False)
    _run(ctx, oracle, 16, 256, dens, 0, 0, 1, True, True, False, True)


# 6. pad bits of a row's last byte are ignored, whatever they hold
@pytest.mark.parametrize("rows,cols", [(3, 70), (33, 1000), (19, 4099), (4, 16321), (1, 1)])
def test_pad_bits_ignored(ctx, oracle, staged, rows, cols):
    for want in (False, True):
        _run(ctx, oracle, rows, cols, (0.5, 0.02, 0.98), 3, 0, 1, True, True, False, want, pad_ones=True)
        _run(ctx, oracle, rows, cols, (0.5,), 1, 0, 0, True, True, True, want, pad_ones=True)


# 7. the context's residual buffer keeps the larger call's size: a smaller call after it is exact
def test_stale_residual_buffer(ctx, oracle, staged):
    _run(ctx, oracle, 33, 1000, (0.5, 0.98, 0.02), 1, 5, 1, True, True, True, False)
    _run(ctx, oracle, 3, 70, (0.02, 0.5, "ones"), 3, 0, 1, True, True, True, False)
    _run(ctx, oracle, 17, 64, (0.5,), 0, 0, 1, True, True, False, False)
    _run(ctx, oracle, 33, 1000, (0.5, 0.98, 0.02), 1, 5, 1, True, True, True, False)


# 8. raster -> encode_pbm_packed(row_index) -> decode_pbm
def _p00(ctx, host, n, stride):
    return ctx.torch.from_numpy(np.array([host[f * stride] >> 7 for f in range(n)], np.uint8)).to(ctx.dev)


def _decode_check(ctx, coder, streams, bits, off, idx, n, rows, cols, pred, p00, planes, lead, gap):
    """decode_pbm into a 0xA5-filled buffer `lead` bytes in, frames fb + gap apart: the frames equal the
    packed planes, every other byte is untouched, and bic_decode_planes + bic_pbm_pack give the same"""
    nb = (cols + 7) // 8
    fb = rows * nb
    stride = fb + gap
    total = lead + (n - 1) * stride + fb + 40
    out = ctx.torch.full((total,), 0xA5, dtype=ctx.torch.uint8, device=ctx.dev)
    ctx.decode_pbm(coder, streams, bits, n, rows, cols, bool(pred), word_off=off, row_index=idx, p00=p00,
                   out=out[lead:], frame_stride=stride)
    back = ctx.decode_planes(coder, streams, bits, n, rows, cols, bool(pred), word_off=off, row_index=idx, p00=p00)
    packed = [ctx.pbm_pack(back[f], cols) for f in range(n)]
    ctx.sync()
    want = np.full(total, 0xA5, np.uint8)
    for f in range(n):
        want[lead + f * stride:lead + f * stride + fb] = plane_to_p4_rows(planes[f], cols).reshape(-1)
    got = out.cpu().numpy()
    assert np.array_equal(got, want), (coder, rows, cols, pred, lead, gap, np.flatnonzero(got != want)[:8])
    for f in range(n):
        assert np.array_equal(packed[f].cpu().numpy(), want[lead + f * stride:lead + f * stride + fb]), f


@pytest.mark.parametrize("rows,cols,off,n,gap,pred", [
    (3, 70, 3, 3, 5, 1),
    (130, 4160, 1, 2, 5, 1),   # more rows than one column chunk, 520-byte rows
    (128, 4096, 13, 1, 0, 1),  # whole column chunks (the Golomb decoder forms the chunk totals itself)
    (3, 70, 3, 3, 0, 0),
    (130, 4160, 1, 1, 0, 0),
    (33, 1000, 0, 3, 0, 1),    # 125-byte rows from an aligned base
    (70, 16321, 3, 1, 0, 1),
    (1, 1, 1, 3, 5, 1),
])
def test_round_trip(ctx, oracle, staged, rows, cols, off, n, gap, pred):
    dens = (0.5, "ones", 0.02)[:n]
    keys, planes = _frames(oracle, rows, cols, dens)
    d, stride, host = _raster(ctx, planes, cols, off, gap, pad_ones=True)
    idx = ctx.empty_i64(n * rows * 2)
    _, (og, bg, fg), (oe, be, fe) = ctx.encode_pbm_packed(d, rows, cols, n, stride, bool(pred), wpr=_even(cols),
                                                          row_index=idx)
    ctx.sync()
    for coder, out, off_w in ((G, og, fg), (E, oe, fe)):
        exp = [_stream(oracle, k, pred, coder) for k in keys]
        assert as_u64(out)[:int(as_u64(off_w)[-1])].tobytes() == b"".join(x[1] for x in exp)
    p00 = _p00(ctx, host, n, stride)
    _decode_check(ctx, G, og, bg, fg, idx, n, rows, cols, pred, p00, planes, off, gap)
    _decode_check(ctx, E, oe, be, fe, None, n, rows, cols, pred, p00, planes, off, gap)
    # adaptive EG: the streams and their index from the unpacked planes
    p2 = ctx.torch.stack([ctx.pbm_unpack(d[f * stride:], rows, cols) for f in range(n)])
    oa, ba = ctx.encode_planes(p2, cols, bool(pred), A)
    ia = ctx.egad_row_index(p2, cols, bool(pred))
    ctx.sync()
    for f, k in enumerate(keys):
        eb, est, _ = oracle.encode_plane(planes[f], cols, pred, A)
        assert int(as_u64(ba)[f]) == eb and stream_bytes(oa[f], eb) == est.tobytes()
        assert np.array_equal(as_u64(ia).reshape(n, 2 * rows)[f], oracle.egad_row_index(planes[f], cols, pred))
    _decode_check(ctx, A, oa, ba, None, ia, n, rows, cols, pred, p00, planes, off, gap)


# 9. a malformed stream is BIC_EDATA at the sync, and the context decodes the good stream afterwards
@pytest.mark.parametrize("coder", [G, E])
def test_malformed_stream(ctx, oracle, staged, coder):
    rows, cols, n = 30, 500, 2
    keys, planes = _frames(oracle, rows, cols, (0.5, 0.02))
    d, stride, host = _raster(ctx, planes, cols, 1, 0)
    idx = ctx.empty_i64(n * rows * 2)
    _, g, e = ctx.encode_pbm_packed(d, rows, cols, n, stride, True, wpr=_even(cols), row_index=idx)
    ctx.sync()
    out, bits, off = g if coder == G else e
    p00 = _p00(ctx, host, n, stride)
    bad = bits.clone()
    bad[0] -= 1
    ctx.decode_pbm(coder, out, bad, n, rows, cols, True, word_off=off, row_index=idx, p00=p00)
    with pytest.raises(pybic.BicError) as err:
        ctx.sync()
    assert err.value.code == pybic.BIC_EDATA
    _decode_check(ctx, coder, out, bits, off, idx, n, rows, cols, 1, p00, planes, 3, 5)


# 10. refusals
def test_rejects(ctx):
    t = ctx.torch
    r = t.zeros(4096, dtype=t.uint8, device=ctx.dev)
    o, b, f, idx = ctx.empty_i64(3 * 64), ctx.empty_i64(3), ctx.empty_i64(4), ctx.empty_i64(3 * 10 * 2)
    lib, h, p = ctx.lib, ctx.h, lambda x: None if x is None else x.data_ptr()

    def enc(raster=r, stride=20, n=3, rows=10, cols=16, wpr=2, og=o, bg=b, oe=None, be=None):
        return lib.bic_encode_pbm(h, p(raster), stride, n, rows, cols, None, wpr, 1, p(og), 64, p(bg), p(oe), 64, p(be))

    def encp(fg=f, og=o, oe=None, fe=None):
        return lib.bic_encode_pbm_packed(h, p(r), 20, 3, 10, 16, None, 2, 1, p(og), 64, p(b), p(fg), p(oe), 64, p(b),
                                         p(fe), None)

    def dec(coder=G, n=3, rows=10, cols=16, stride=20, index=idx, raster=r, streams=o, off=f):
        return lib.bic_decode_pbm(h, coder, p(streams), 0, p(off), p(b), p(index), n, rows, cols, 1, None, p(raster),
                                  stride)

    assert enc() == pybic.BIC_OK and encp() == pybic.BIC_OK
    ctx.sync()
    E_ = pybic.BIC_EINVAL
    assert enc(n=0) == E_ and enc(n=-1) == E_            # nframes < 1
    assert enc(stride=19) == E_                          # frames overlap
    assert enc(stride=0, n=1) == pybic.BIC_OK            # one frame: the stride is ignored
    assert enc(raster=None) == E_                        # no raster
    assert enc(cols=0) == E_ and enc(wpr=0) == E_        # geometry
    assert enc(rows=1 << 20, cols=1 << 12, stride=1 << 29) == E_  # rows * (cols + 1) >= 2^31
    assert enc(og=None, bg=None) == E_                   # no output requested
    assert enc(bg=None) == E_                            # a stream without its bit counts
    assert encp(fg=None) == E_                           # packed: out without off
    assert encp(oe=o, fe=None) == E_
    ctx.sync()
    assert dec(n=0) == E_
    assert dec(stride=19) == E_
    assert dec(index=None) == E_                         # Golomb needs the row index
    assert dec(coder=A, index=None) == E_                # and so does adaptive EG
    assert dec(coder=3) == E_
    assert dec(cols=16385, stride=1 << 20) == E_         # wider than the decoders take
    assert dec(cols=0) == E_
    assert dec(raster=None) == E_ and dec(streams=None) == E_ and dec(off=None) == E_
    ctx.sync()


# 11. rows = 0: BIC_OK, zero bit counts and offsets, nothing else written
def test_no_rows(ctx):
    t = ctx.torch
    r = t.zeros(64, dtype=t.uint8, device=ctx.dev)
    out = t.full((3 * 8,), 0x5A5A, dtype=t.int64, device=ctx.dev)
    _, (og, bg), (oe, be) = ctx.encode_pbm(r, 0, 16, 3, 0, slots=(8, 8), outs=(out.clone(), out.clone()),
                                          bits=(t.full((3,), 7, dtype=t.int64, device=ctx.dev),
                                                t.full((3,), 7, dtype=t.int64, device=ctx.dev)))
    _, (pg, cg, fg), (pe, ce, fe) = ctx.encode_pbm_packed(
        r, 0, 16, 3, 0, slots=(8, 8), outs=(out.clone(), out.clone()),
        offs=(t.full((4,), 7, dtype=t.int64, device=ctx.dev), t.full((4,), 7, dtype=t.int64, device=ctx.dev)))
    ctx.sync()
    for x in (bg, be, cg, ce):
        assert list(as_u64(x)) == [0, 0, 0]
    for x in (fg, fe):
        assert list(as_u64(x)) == [0, 0, 0, 0]
    for x in (og, oe, pg, pe):
        assert t.equal(x.reshape(-1), out)
    buf = t.full((64,), 0x5A, dtype=t.uint8, device=ctx.dev)
    ctx.decode_pbm(E, og, bg, 3, 0, 16, True, out=buf)
    ctx.sync()
    assert bool((buf == 0x5A).all())


# 12. from a file: the file's bytes on the device, the header parsed on the host
def test_from_file(ctx, oracle, staged, tmp_path):
    rows, cols = 40, 1000
    key, P = _plane(oracle, rows, cols, 0.5, 0)
    data = open(write_pbm(str(tmp_path / "frame.pbm"), P, cols), "rb").read()
    info = pybic.pnm_header(data)
    assert (info.type, info.rows, info.cols) == (4, rows, cols) and info.data_offset == len(data) - rows * 125
    dev = ctx.torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(ctx.dev)
    planes, (og, bg), (oe, be) = ctx.encode_pbm(dev[info.data_offset:], rows, cols, planes=True, wpr=16)
    ctx.sync()
    assert np.array_equal(as_u64(planes)[0], P)
    for coder, out, bits in ((G, og, bg), (E, oe, be)):
        eb, est = _stream(oracle, key, 1, coder)
        assert int(as_u64(bits)[0]) == eb and stream_bytes(out[0], eb) == est


# 13. the first row of a plane starts from a fresh coder, so its Golomb decoder reads the first stream
#     bytes bit by bit and only then from its byte table. In these rows (seeds found with the decoder
#     census, tests/decoder_census.py: g_stale_step_first_row) the last bit-by-bit byte ends inside a zero
#     run that has just crossed a 64-column word: the table steps after it must place their columns in the
#     word the run reached
@pytest.mark.parametrize("seed", [105, 111, 590])
def test_round_trip_first_row_run_across_word(ctx, oracle, staged, seed):
    rows, cols, n = 1, 256, 1
    P = oracle.gen_plane(seed, 0.5, rows, cols)
    d, stride, host = _raster(ctx, [P], cols, 1, 0)
    idx = ctx.empty_i64(n * rows * 2)
    _, (og, bg, fg), _ = ctx.encode_pbm_packed(d, rows, cols, n, stride, False, wpr=_even(cols), eg=False,
                                               row_index=idx)
    ctx.sync()
    eb, est, _ = oracle.encode_plane(P, cols, 0, G)
    assert int(as_u64(bg)[0]) == eb and as_u64(og)[:(eb + 63) // 64].tobytes() == est.tobytes()
    _decode_check(ctx, G, og, bg, fg, idx, n, rows, cols, 0, None, [P], 1, 0)
