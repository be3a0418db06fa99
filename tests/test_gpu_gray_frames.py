"""bic_encode_gray_frames / bic_encode_gray_frames_packed / bic_decode_gray_frames: a batch of gray frames to
streams and back in one call each. Expected planes, streams and row indices are the oracle's on each frame
taken alone (bo_bitplanes, bo_encode_plane, bo_row_index; with BIC_OPT_GRAY_CODE on graycode_ref.gray of the
frame), expected samples the input frames: never anything the library produced, except where a test says it
compares two paths. Inputs are seeded; the frames differ from one another, every frame's pixel (0,0) is all
ones (a row above or a kept R(0,0) would show), frame f's row 0 differs from frame f - 1's last row, and every
byte outside the samples holds a pattern that must never reach an output. All comparisons are exact."""
import numpy as np
import pytest

import pybic
from graycode_ref import gray
from pybic import as_u64, stream_bytes

pytestmark = pytest.mark.gpu
G, E, A = pybic.CODER_GOLOMB, pybic.CODER_EG, pybic.CODER_EG_ADAPTIVE
PAD, OUTSIDE = 0xC3, 0xA5  # pitch padding; gaps between frames and the bytes around the buffer


@pytest.fixture
def staged(ctx):
    """the staged encoder (and with it the frame-aware count kernel) at test sizes"""
    ctx.set_encoder("staged")
    yield
    ctx.set_encoder("auto")


@pytest.fixture
def gc(ctx):
    ctx.set_gray_code(True)
    yield
    ctx.set_gray_code(False)


_FRAMES, _STREAM, _INDEX = {}, {}, {}


def _frames(oracle, kind, n, rows, cols, bps=1, gcode=False):
    """n seeded frames, made once and read-only -> (key, the frames [n, rows, cols], the oracle's planes
    [n, 8 * bps, rows, used] of each frame alone). kind: "uniform" (every bit p = 0.5) or "smooth" (a ramp with
    a little noise: long runs in the high planes)"""
    key = (kind, n, rows, cols, bps, gcode)
    if key not in _FRAMES:
        dt = np.uint8 if bps == 1 else np.uint16
        imgs = np.zeros((n, rows, cols), dt)
        for f in range(n):
            seed = 0xF4A3E5 + 7919 * f + 131 * rows + cols + 17 * bps
            if kind == "uniform":
                imgs[f] = oracle.gen_bytes(seed, rows * cols * bps).view(dt).reshape(rows, cols)
            else:
                r, c = np.mgrid[0:rows, 0:cols]
                noise = oracle.gen_bytes(seed, rows * cols).reshape(rows, cols) & 1
                imgs[f] = ((c >> 4) + 3 * r + 41 * f + noise).astype(dt)
            imgs[f, 0, 0] = 0xFF if bps == 1 else 0xFFFF
            if f:
                assert not np.array_equal(imgs[f, 0], imgs[f - 1, -1]) and not np.array_equal(imgs[f], imgs[f - 1])
        planes = np.stack([oracle.bitplanes(gray(a) if gcode else a, 8 * bps) for a in imgs])
        imgs.setflags(write=False)
        planes.setflags(write=False)
        _FRAMES[key] = (imgs, planes)
    return (key,) + _FRAMES[key]


def _stream(oracle, key, f, b, pred, coder):
    """plane b of frame f: its expected (bits, stream bytes), computed once"""
    q = (key, f, b, pred, coder)
    if q not in _STREAM:
        eb, est, _ = oracle.encode_plane(_FRAMES[key][1][f, b], key[3], pred, coder)
        _STREAM[q] = (eb, est.tobytes())
    return _STREAM[q]


def _index(oracle, key, f, b, pred):
    q = (key, f, b, pred)
    if q not in _INDEX:
        _INDEX[q] = oracle.row_index(_FRAMES[key][1][f, b], key[3], pred)
    return _INDEX[q]


def _sample_bytes(imgs, be):
    n, rows, cols = imgs.shape
    if imgs.dtype == np.uint8:
        return imgs
    return imgs.astype(">u2" if be else "<u2").view(np.uint8).reshape(n, rows, 2 * cols)


def _buffer(ctx, imgs, be=1, pitch=None, off=16, gap=0):
    """the frames' sample bytes `off` bytes into a 16-byte aligned device buffer, rows `pitch` bytes and frames
    rows * pitch + gap bytes apart; PAD behind a row's samples, OUTSIDE between the frames, before frame 0 and
    after the last -> (the view at frame 0's first sample, pitch, frame stride)"""
    src = _sample_bytes(imgs, be)
    n, rows, rb = src.shape
    pitch = pitch or rb
    stride = rows * pitch + gap
    buf = np.full(off + n * stride + 80, OUTSIDE, np.uint8)
    for f in range(n):
        r = np.full((rows, pitch), PAD, np.uint8)
        r[:, :rb] = src[f]
        buf[off + f * stride:off + f * stride + rows * pitch] = r.reshape(-1)
    d = ctx.torch.from_numpy(buf).to(ctx.dev)
    assert d.data_ptr() % 16 == 0
    return d[off:], pitch, stride


def _even(cols):
    return ((cols + 63) // 64 + 1) & ~1


def _check(ctx, oracle, key, n, rows, cols, plane0, nplanes, pred, got, g, e, wpr, want_planes, packed, idx, tag):
    """one call's outputs against the oracle's for each frame alone"""
    planes, used, np_ = _FRAMES[key][1], (cols + 63) // 64, nplanes
    if want_planes:
        # (pad words are the caller's: the count pass writes the words that hold pixels and leaves the prefill, the
        # per-frame extraction writes them 0)
        have = as_u64(got)
        assert np.array_equal(have[:, :, :used], planes[:, plane0:plane0 + np_].reshape(n * np_, rows, used)), tag
        assert bool(np.all((have[:, :, used:] == 0) | (have[:, :, used:] == np.uint64(0xFFFFFFFFFFFFFFFF)))), tag
    else:
        assert got is None
    for coder, res in ((G, g), (E, e)):
        if res is None:
            continue
        exp = [_stream(oracle, key, f, plane0 + k, pred, coder) for f in range(n) for k in range(np_)]
        bits = [int(x) for x in as_u64(res[1])]
        print(tag, "coder", coder, "bits", bits[:24], "expected", [x[0] for x in exp][:24])
        assert bits == [x[0] for x in exp], (tag, coder)
        nw = [(x[0] + 63) // 64 for x in exp]
        if packed:
            offs = [int(x) for x in as_u64(res[2])]
            assert offs == [sum(nw[:i]) for i in range(n * np_ + 1)], (tag, coder)
            assert as_u64(res[0])[:offs[-1]].tobytes() == b"".join(x[1] for x in exp), (tag, coder)
        else:
            for i in range(n * np_):
                assert stream_bytes(res[0][i], bits[i]) == exp[i][1], (tag, coder, i)
    if idx is not None:
        ri = as_u64(idx).reshape(n * np_, 2 * rows)
        for f in range(n):
            for k in range(np_):
                assert np.array_equal(ri[f * np_ + k], _index(oracle, key, f, plane0 + k, pred)), (tag, f, k)


def _run(ctx, oracle, kind, n, rows, cols, bps=1, be=1, pitch=None, off=16, gap=0, pred=1, plane0=0, nplanes=None,
         want_planes=False, packed=False, wpr=None, gcode=False, golomb=True, eg=True, stride=None):
    key, imgs, _ = _frames(oracle, kind, n, rows, cols, bps, gcode)
    nplanes = nplanes or 8 * bps - plane0
    wpr = wpr or _even(cols)
    d, pitch, st = _buffer(ctx, imgs, be, pitch, off, gap)
    st = st if stride is None else stride
    tag = (kind, n, rows, cols, bps, be, pitch, off, gap, pred, plane0, nplanes, want_planes, packed, wpr, gcode)
    pl = ctx.torch.full((n * nplanes, rows, wpr), -1, dtype=ctx.torch.int64, device=ctx.dev) if want_planes else None
    idx = None
    kw = dict(nframes=n, frame_stride=st, pitch=pitch, sample_bytes=bps, big_endian=bool(be), nplanes=nplanes,
              plane0=plane0, predict=bool(pred), planes=pl, wpr=wpr, golomb=golomb, eg=eg)
    if packed:
        idx = ctx.empty_i64(n * nplanes * rows * 2)
        got, g, e = ctx.encode_gray_frames_packed(d, rows, cols, row_index=idx, **kw)
    else:
        got, g, e = ctx.encode_gray_frames(d, rows, cols, **kw)
    ctx.sync()
    _check(ctx, oracle, key, n, rows, cols, plane0, nplanes, pred, got, g, e, wpr, want_planes, packed, idx, tag)
    return d, pitch, st, g, e, idx


# ---- encode -------------------------------------------------------------------------------------------------------

# 1. planes NULL: with prediction and slots the count pass writes the EG streams itself (EG source); without
#    prediction, and with packed output, the residual planes go to the context's buffer
@pytest.mark.parametrize("pred", [1, 0])
def test_eg_source_and_residual_buffer(ctx, oracle, staged, pred):
    _run(ctx, oracle, "uniform", 3, 5, 4096, pred=pred)
    _run(ctx, oracle, "uniform", 3, 5, 4096, pred=pred, packed=True)


# 2. two strips; planes returned: four rows per wave, 7 rows = a block of 4 and one of 3 that ends with its frame
@pytest.mark.parametrize("pred", [1, 0])
def test_two_strips_planes_returned(ctx, oracle, staged, pred):
    _run(ctx, oracle, "uniform", 2, 7, 8192, pred=pred, want_planes=True)


# 3. four strips, a smooth input (long runs, rows of every k class)
def test_four_strips_smooth(ctx, oracle, staged):
    _run(ctx, oracle, "smooth", 5, 3, 16384)
    _run(ctx, oracle, "smooth", 5, 3, 16384, want_planes=True, packed=True)


# 4. partial words: a last word with pad bits, lanes beyond the row
@pytest.mark.parametrize("cols,pitch,wpr", [(100, 128, 2), (130, 192, 4)])
@pytest.mark.parametrize("want", [True, False])
def test_partial_words(ctx, oracle, staged, cols, pitch, wpr, want):
    _run(ctx, oracle, "uniform", 4, 9, cols, pitch=pitch, wpr=wpr, want_planes=want)
    _run(ctx, oracle, "uniform", 4, 9, cols, pitch=pitch, wpr=wpr, want_planes=want, off=19, gap=5, packed=True)


# 5. an aligned base and pitch with a frame stride that is not (frame 1 is misaligned where frame 0 is not), and
#    one that is
@pytest.mark.parametrize("gap", [37, 16])
@pytest.mark.parametrize("want", [False, True])
def test_odd_stride_aligned_base(ctx, oracle, staged, gap, want):
    _run(ctx, oracle, "uniform", 3, 6, 4096, gap=gap, want_planes=want)


# 6. concatenated P5 files as they lie: the headers parsed on the host, the bytes on the device
def test_p5_files(ctx, oracle, staged):
    n, rows, cols = 3, 6, 4096
    key, imgs, _ = _frames(oracle, "uniform", n, rows, cols)
    files = [b"P5\n# frame %d\n%d %d\n255\n" % (f, cols, rows) + imgs[f].tobytes() for f in range(n)]
    assert len({len(x) for x in files}) == 1
    data = b"".join(files)
    infos = [pybic.pnm_header(data[f * len(files[0]):]) for f in range(n)]
    for i in infos:
        assert (i.type, i.rows, i.cols, i.maxval, i.data_offset) == (5, rows, cols, 255, infos[0].data_offset)
    stride, off = len(files[0]), infos[0].data_offset
    assert stride % 16 and off % 16
    host = np.concatenate([np.full(16, OUTSIDE, np.uint8), np.frombuffer(data, np.uint8),
                           np.full(80, OUTSIDE, np.uint8)])
    dev = ctx.torch.from_numpy(host).to(ctx.dev)
    for want in (None, True):
        idx = ctx.empty_i64(n * 8 * rows * 2)
        got, g, e = ctx.encode_gray_frames_packed(dev[16 + off:], rows, cols, nframes=n, frame_stride=stride,
                                                  planes=want, wpr=64, row_index=idx)
        ctx.sync()
        _check(ctx, oracle, key, n, rows, cols, 0, 8, 1, got, g, e, 64, bool(want), True, idx, ("p5", want))


# 7. plane ranges
@pytest.mark.parametrize("plane0,nplanes", [(2, 3), (7, 1)])
def test_plane_ranges(ctx, oracle, staged, plane0, nplanes):
    _run(ctx, oracle, "uniform", 3, 5, 4096, plane0=plane0, nplanes=nplanes)
    _run(ctx, oracle, "uniform", 3, 5, 4096, plane0=plane0, nplanes=nplanes, want_planes=True, off=17, packed=True)


# 8. more than 1024 planes in one call
def test_many_planes(ctx, oracle, staged):
    _run(ctx, oracle, "uniform", 130, 2, 128, wpr=2, packed=True)
    _run(ctx, oracle, "uniform", 130, 2, 128, wpr=2, want_planes=True, gap=3)


# 9. packed output: the offsets run through all streams, the row index is each frame's own
def test_packed_output(ctx, oracle, staged):
    _run(ctx, oracle, "smooth", 3, 6, 4096, packed=True, off=21, gap=11)
    _run(ctx, oracle, "uniform", 3, 6, 4096, packed=True, eg=False)
    _run(ctx, oracle, "uniform", 3, 6, 4096, packed=True, golomb=False)  # the index from bic_row_index


# 10. BIC_OPT_GRAY_CODE
def test_gray_code(ctx, oracle, staged, gc):
    _run(ctx, oracle, "uniform", 2, 5, 4096, gcode=True)
    _run(ctx, oracle, "uniform", 2, 5, 4096, gcode=True, want_planes=True, off=29, packed=True)


# 11. two-byte samples, both byte orders, a range across the byte boundary
@pytest.mark.parametrize("be", [1, 0])
def test_two_byte_samples(ctx, oracle, staged, be):
    _run(ctx, oracle, "uniform", 3, 5, 4096, bps=2, be=be, plane0=4, nplanes=8)
    _run(ctx, oracle, "uniform", 3, 5, 4096, bps=2, be=be, plane0=4, nplanes=8, want_planes=True, off=17, gap=3,
         packed=True)


# 12. a single frame: the stride is ignored, and the outputs are bic_encode_gray_packed's word for word (a
#     comparison of two paths, after the comparison with the oracle)
@pytest.mark.parametrize("rows,cols", [(5, 4096), (9, 100)])
def test_single_frame(ctx, oracle, staged, rows, cols):
    pitch = 64 * ((cols + 63) // 64)
    d, pitch, _, g, e, idx = _run(ctx, oracle, "uniform", 1, rows, cols, pitch=pitch, packed=True, stride=0)
    img = d.as_strided((rows, pitch), (pitch, 1))
    idx1 = ctx.empty_i64(8 * rows * 2)
    _, g1, e1 = ctx.encode_gray_packed(img, cols, store_planes=False, row_index=idx1)
    ctx.sync()
    for a, b in ((g, g1), (e, e1)):
        assert ctx.torch.equal(a[1], b[1]) and ctx.torch.equal(a[2], b[2])
        nwords = int(as_u64(a[2])[-1])
        assert ctx.torch.equal(a[0].reshape(-1)[:nwords], b[0].reshape(-1)[:nwords])
    assert ctx.torch.equal(idx, idx1)


# 13. the automatic encoder at this size: the fallback (an extraction per frame, one encode of all planes)
def test_automatic_encoder(ctx, oracle):
    _run(ctx, oracle, "uniform", 3, 5, 4096)
    _run(ctx, oracle, "uniform", 3, 5, 4096, packed=True, want_planes=True, gap=37)


def test_launches(ctx, oracle, staged):
    """which kernels a call launches (bic_prof_collect's names), so that the cases above test the path they are
    meant to: one count pass for all frames where it applies, an extraction per frame otherwise"""
    _, imgs, _ = _frames(oracle, "uniform", 3, 5, 4096)
    d, pitch, st = _buffer(ctx, imgs, gap=37)
    _, imgs16, _ = _frames(oracle, "uniform", 3, 5, 4096, 2)
    d16, pitch16, st16 = _buffer(ctx, imgs16)
    ctx.sync()
    ctx.prof_collect()
    ctx.prof_enable(True)
    try:
        ctx.prof_only(None)
        for pl in (None, True):
            ctx.encode_gray_frames(d, 5, 4096, nframes=3, frame_stride=st, planes=pl)
            got = ctx.prof_collect()
            assert got["bitplanes_count"][0] == 1 and "bitplanes_u8" not in got and "encode_prefix" in got, got
        ctx.encode_gray_frames(d, 5, 4096, nframes=3, frame_stride=st, wpr=65)  # an odd row pitch
        got = ctx.prof_collect()
        assert "bitplanes_count" not in got and sum(v[0] for k, v in got.items() if k.startswith("bitplanes")) == 3, got
        ctx.encode_gray_frames(d16, 5, 4096, nframes=3, frame_stride=st16, sample_bytes=2)
        got = ctx.prof_collect()
        assert "bitplanes_count" not in got and sum(v[0] for k, v in got.items() if k.startswith("bitplanes")) == 3, got
    finally:
        ctx.prof_only(None)
        ctx.prof_enable(False)


def test_rejects(ctx):
    t = ctx.torch
    r = t.zeros(4096, dtype=t.uint8, device=ctx.dev)
    o, b, f, idx = ctx.empty_i64(24 * 64), ctx.empty_i64(24), ctx.empty_i64(25), ctx.empty_i64(24 * 10 * 2)
    lib, h, p = ctx.lib, ctx.h, lambda x: None if x is None else x.data_ptr()

    def enc(gray=r, stride=640, n=3, pitch=64, rows=10, cols=16, sb=1, plane0=0, npl=8, wpr=2, og=o, bg=b):
        return lib.bic_encode_gray_frames(h, p(gray), stride, n, pitch, rows, cols, sb, 1, plane0, npl, None, wpr, 1,
                                          p(og), 64, p(bg), None, 64, None)

    def encp(fg=f, og=o, oe=None, fe=None):
        return lib.bic_encode_gray_frames_packed(h, p(r), 640, 3, 64, 10, 16, 1, 1, 0, 8, None, 2, 1, p(og), 64, p(b),
                                                 p(fg), p(oe), 64, p(b), p(fe), None)

    def dec(coder=G, n=3, npl=8, plane0=0, rows=10, cols=16, sb=1, pitch=64, stride=640, index=idx, gray=r, streams=o,
            off=f):
        return lib.bic_decode_gray_frames(h, coder, p(streams), 0, p(off), p(b), p(index), n, plane0, npl, rows, cols,
                                          1, None, sb, 1, p(gray), pitch, stride)

    assert enc() == pybic.BIC_OK and encp() == pybic.BIC_OK
    ctx.sync()
    E_ = pybic.BIC_EINVAL
    assert enc(n=0) == E_ and enc(n=-1) == E_             # nframes < 1
    assert enc(n=8192) == E_                              # nframes * nplanes > 65535
    assert enc(sb=0) == E_ and enc(sb=3) == E_            # sample_bytes outside {1, 2}
    assert enc(plane0=1) == E_ and enc(plane0=-1, npl=2) == E_ and enc(npl=0) == E_   # a range outside the sample
    assert enc(sb=2, plane0=9, npl=8) == E_
    assert enc(pitch=15) == E_ and enc(sb=2, pitch=31, npl=16) == E_                  # pitch < cols * sample_bytes
    assert enc(stride=639) == E_                          # frames overlap
    assert enc(stride=0, n=1) == pybic.BIC_OK             # one frame: the stride is ignored
    assert enc(gray=None) == E_
    assert enc(cols=0) == E_ and enc(wpr=0) == E_         # geometry
    assert enc(rows=1 << 20, cols=1 << 12, pitch=1 << 12, stride=1 << 32) == E_      # rows * (cols + 1) >= 2^31
    assert enc(og=None, bg=None) == E_ and enc(bg=None) == E_
    assert encp(fg=None) == E_ and encp(oe=o, fe=None) == E_
    ctx.sync()
    assert dec(n=0) == E_ and dec(n=8192) == E_
    assert dec(sb=3) == E_ and dec(plane0=1) == E_ and dec(npl=0) == E_
    assert dec(pitch=15) == E_ and dec(stride=639) == E_
    assert dec(index=None) == E_ and dec(coder=A, index=None) == E_ and dec(coder=3) == E_
    assert dec(cols=16385, pitch=16385, stride=1 << 20) == E_
    assert dec(gray=None) == E_ and dec(streams=None) == E_ and dec(off=None) == E_
    ctx.sync()


def test_no_rows(ctx):
    t = ctx.torch
    r = t.zeros(64, dtype=t.uint8, device=ctx.dev)
    out = t.full((6 * 8,), 0x5A5A, dtype=t.int64, device=ctx.dev)
    seven = lambda k: t.full((k,), 7, dtype=t.int64, device=ctx.dev)
    _, (og, bg), (oe, be) = ctx.encode_gray_frames(r, 0, 16, nframes=3, nplanes=2, slots=(8, 8),
                                                   outs=(out.clone(), out.clone()), bits=(seven(6), seven(6)))
    _, (pg, cg, fg), (pe, ce, fe) = ctx.encode_gray_frames_packed(r, 0, 16, nframes=3, nplanes=2, slots=(8, 8),
                                                                  outs=(out.clone(), out.clone()),
                                                                  offs=(seven(7), seven(7)))
    ctx.sync()
    for x in (bg, be, cg, ce):
        assert list(as_u64(x)) == [0] * 6
    for x in (fg, fe):
        assert list(as_u64(x)) == [0] * 7
    for x in (og, oe, pg, pe):
        assert t.equal(x.reshape(-1), out)
    buf = t.full((64,), 0x5A, dtype=t.uint8, device=ctx.dev)
    ctx.decode_gray_frames(E, og, bg, 3, 2, 0, 16, out=buf)
    ctx.sync()
    assert bool((buf == 0x5A).all())


# ---- decode -------------------------------------------------------------------------------------------------------

def _p00(ctx, imgs, plane0, nplanes, gcode):
    """one byte per stream: bit plane0 + k of frame f's first sample (of its Gray code with the option on)"""
    v = [int(gray(a[0, 0]) if gcode else a[0, 0]) for a in imgs]
    bits = np.array([(x >> (plane0 + k)) & 1 for x in v for k in range(nplanes)], np.uint8)
    return ctx.torch.from_numpy(bits).to(ctx.dev)


def _decode_check(ctx, coder, streams, bits, off, idx, imgs, be, plane0, nplanes, pred, p00, lead, pitch, gap, tag):
    """decode into a buffer filled with a pattern, frame 0 `lead` bytes in: the samples equal the input's (the
    range's bits of them), every other byte keeps the pattern"""
    n, rows, cols = imgs.shape
    bps = imgs.dtype.itemsize
    stride = rows * pitch + gap
    total = lead + (n - 1) * stride + rows * pitch + 48
    out = ctx.torch.full((total,), 0x5A, dtype=ctx.torch.uint8, device=ctx.dev)
    assert out.data_ptr() % 16 == 0
    ctx.decode_gray_frames(coder, streams, bits, n, nplanes, rows, cols, bool(pred), word_off=off, row_index=idx,
                           p00=p00, plane0=plane0, sample_bytes=bps, big_endian=bool(be), out=out[lead:], pitch=pitch,
                           frame_stride=stride)
    ctx.sync()
    mask = ((1 << nplanes) - 1) << plane0
    src = _sample_bytes((imgs & mask).astype(imgs.dtype), be)
    want = np.full(total, 0x5A, np.uint8)
    for f in range(n):
        for r in range(rows):
            o = lead + f * stride + r * pitch
            want[o:o + cols * bps] = src[f, r]
    got = out.cpu().numpy()
    assert np.array_equal(got, want), (tag, coder, np.flatnonzero(got != want)[:8])


def _round_trip(ctx, oracle, n, rows, cols, bps=1, be=1, plane0=0, nplanes=None, gcode=False, places=None):
    key, imgs, planes = _frames(oracle, "uniform", n, rows, cols, bps, gcode)
    nplanes = nplanes or 8 * bps - plane0
    d, pitch, st = _buffer(ctx, imgs, be, pitch=64 * bps * ((cols + 63) // 64), off=16 + 3, gap=9)
    idx = ctx.empty_i64(n * nplanes * rows * 2)
    _, (og, bg, fg), (oe, be_, fe) = ctx.encode_gray_frames_packed(
        d, rows, cols, nframes=n, frame_stride=st, pitch=pitch, sample_bytes=bps, big_endian=bool(be), nplanes=nplanes,
        plane0=plane0, wpr=_even(cols), row_index=idx)
    # adaptive EG: the streams and their index from the oracle's planes
    pl = ctx.torch.from_numpy(np.array(planes[:, plane0:plane0 + nplanes]).view(np.int64)).to(ctx.dev)  # (a copy)
    pl = pl.reshape(n * nplanes, rows, -1)
    oa, ba = ctx.encode_planes(pl, cols, True, A)
    ia = ctx.egad_row_index(pl, cols, True)
    ctx.sync()
    p00 = _p00(ctx, imgs, plane0, nplanes, gcode)
    # (frame 0's offset, pitch beyond the samples, gap): odd everything; and 16-byte aligned everything (vector
    # stores); and aligned rows with an odd frame stride (frame 1 is then misaligned)
    rb = cols * bps
    places = places or [(16 + 3, rb + 5, 7), (16, (rb + 15) // 16 * 16, 32), (16, (rb + 15) // 16 * 16, 7)]
    for lead, opitch, gap in places:
        tag = (n, rows, cols, bps, be, plane0, nplanes, gcode, lead, opitch, gap)
        _decode_check(ctx, G, og, bg, fg, idx, imgs, be, plane0, nplanes, 1, p00, lead, opitch, gap, tag)
        _decode_check(ctx, E, oe, be_, fe, None, imgs, be, plane0, nplanes, 1, p00, lead, opitch, gap, tag)
        _decode_check(ctx, A, oa, ba, None, ia, imgs, be, plane0, nplanes, 1, p00, lead, opitch, gap, tag)


# rows 64 and 128: whole column chunks (the Golomb decoder forms the chunk totals itself); 1 and 70: the other route
@pytest.mark.parametrize("cols", [100, 4096])
@pytest.mark.parametrize("rows", [1, 64, 70, 128])
def test_round_trip(ctx, oracle, staged, rows, cols):
    _round_trip(ctx, oracle, 3, rows, cols)


def test_round_trip_plane_range(ctx, oracle, staged):
    _round_trip(ctx, oracle, 3, 70, 100, plane0=2, nplanes=3)


def test_round_trip_gray_code(ctx, oracle, staged, gc):
    _round_trip(ctx, oracle, 3, 70, 100, gcode=True)
    _round_trip(ctx, oracle, 3, 64, 4096, gcode=True, places=[(16, 4096, 16)])


@pytest.mark.parametrize("be", [1, 0])
def test_round_trip_two_byte_samples(ctx, oracle, staged, be):
    _round_trip(ctx, oracle, 3, 70, 100, bps=2, be=be)


def test_round_trip_without_prediction(ctx, oracle, staged):
    """predict off: the D buffer holds the planes themselves (no chunk totals)"""
    n, rows, cols = 3, 70, 100
    key, imgs, _ = _frames(oracle, "uniform", n, rows, cols)
    d, pitch, st = _buffer(ctx, imgs, pitch=128, gap=9)
    idx = ctx.empty_i64(n * 8 * rows * 2)
    _, (og, bg, fg), (oe, be_, fe) = ctx.encode_gray_frames_packed(d, rows, cols, nframes=n, frame_stride=st,
                                                                   pitch=pitch, predict=False, wpr=2, row_index=idx)
    ctx.sync()
    for lead, opitch, gap in [(19, 105, 7), (16, 112, 16)]:
        _decode_check(ctx, G, og, bg, fg, idx, imgs, 1, 0, 8, 0, None, lead, opitch, gap, "nopred")
        _decode_check(ctx, E, oe, be_, fe, None, imgs, 1, 0, 8, 0, None, lead, opitch, gap, "nopred")
