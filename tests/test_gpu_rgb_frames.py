"""bic_encode_rgb_frames / bic_encode_rgb_frames_packed: a batch of interleaved RGB frames to streams in one call.
Entry (f * 3 + c) * nplanes + k of every output is plane plane0 + k of channel c of frame f. Expected planes,
streams and row indices are the oracle's on channel c of frame f taken alone as a gray image (bo_bitplanes,
bo_encode_plane, bo_row_index; with BIC_OPT_COLOR_TRANSFORM on colour_ref.forward of the frame, with
BIC_OPT_GRAY_CODE on graycode_ref.gray of that): never anything the library produced. After that comparison every
call is also compared with encode_rgb / encode_rgb_packed of each frame alone (two paths of the library). Inputs
are seeded; the frames and their channels differ from one another, every frame's pixel (0,0) is all ones (a row
above or a kept R(0,0) would show), frame f's row 0 differs from frame f - 1's last row, and every byte outside
the samples holds a pattern that must never reach an output. All comparisons are exact."""
import numpy as np
import pytest

import colour_ref
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
def options(ctx):
    """set(gray_code, color_transform) for one test; both off again afterwards"""
    def set_(gcode, ct):
        ctx.set_gray_code(bool(gcode))
        ctx.set_color_transform(ct)
    yield set_
    ctx.set_gray_code(False)
    ctx.set_color_transform(0)


_FRAMES, _STREAM, _INDEX = {}, {}, {}


def frames(oracle, kind, n, rows, cols, ct=0, gcode=False):
    """n seeded frames, made once and read-only -> (key, the frames [n, rows, cols, 3], the oracle's planes
    [n, 24, rows, used] of each frame alone: plane 8 c + b = bit b of channel c after the transform and the Gray
    code). kind: "uniform" (every bit p = 0.5) or "smooth" (a different ramp with a little noise per channel)"""
    key = (kind, n, rows, cols, ct, gcode)
    if key not in _FRAMES:
        imgs = np.zeros((n, rows, cols, 3), np.uint8)
        for f in range(n):
            seed = 0x52F4A3 + 7919 * f + 131 * rows + cols
            if kind == "uniform":
                imgs[f] = oracle.gen_bytes(seed, rows * cols * 3).reshape(rows, cols, 3)
            else:
                r, c = np.mgrid[0:rows, 0:cols]
                noise = oracle.gen_bytes(seed, rows * cols * 3).reshape(3, rows, cols) & 1
                imgs[f] = np.stack([(c >> 4) + 3 * r + 41 * f + noise[0], (c >> 3) + 5 * r + 17 * f + noise[1],
                                    (c >> 5) + r + 29 * f + noise[2]], axis=2).astype(np.uint8)
            imgs[f, 0, 0] = 0xFF
            for c in range(3):
                assert not np.array_equal(imgs[f, :, :, c], imgs[f, :, :, (c + 1) % 3])
            if f:
                assert not np.array_equal(imgs[f, 0], imgs[f - 1, -1]) and not np.array_equal(imgs[f], imgs[f - 1])
        planes = []
        for a in imgs:
            v = colour_ref.forward(a, ct)
            v = gray(v) if gcode else v
            planes.append(np.concatenate([oracle.bitplanes(np.ascontiguousarray(v[:, :, c]), 8) for c in range(3)]))
        planes = np.stack(planes)
        imgs.setflags(write=False)
        planes.setflags(write=False)
        _FRAMES[key] = (imgs, planes)
    return (key,) + _FRAMES[key]


def _stream(oracle, key, f, p, pred, coder):
    """plane p (8 c + b) of frame f: its expected (bits, stream bytes), computed once"""
    q = (key, f, p, pred, coder)
    if q not in _STREAM:
        eb, est, _ = oracle.encode_plane(_FRAMES[key][1][f, p], key[3], pred, coder)
        _STREAM[q] = (eb, est.tobytes())
    return _STREAM[q]


def _index(oracle, key, f, p, pred):
    q = (key, f, p, pred)
    if q not in _INDEX:
        _INDEX[q] = oracle.row_index(_FRAMES[key][1][f, p], key[3], pred)
    return _INDEX[q]


def buffer(ctx, imgs, pitch=None, off=16, gap=0):
    """the frames' sample bytes `off` bytes into a 16-byte aligned device buffer, rows `pitch` bytes and frames
    rows * pitch + gap bytes apart; PAD behind a row's samples, OUTSIDE between the frames, before frame 0 and
    after the last (192 bytes: the fused read takes ceil(cols/64) * 192 bytes of a row) -> (the view at frame 0's
    first sample, pitch, frame stride)"""
    n, rows, cols, _ = imgs.shape
    src = imgs.reshape(n, rows, 3 * cols)
    pitch = pitch or 3 * cols
    stride = rows * pitch + gap
    buf = np.full(off + n * stride + 256, OUTSIDE, np.uint8)
    for f in range(n):
        r = np.full((rows, pitch), PAD, np.uint8)
        r[:, :3 * cols] = src[f]
        buf[off + f * stride:off + f * stride + rows * pitch] = r.reshape(-1)
    d = ctx.torch.from_numpy(buf).to(ctx.dev)
    assert d.data_ptr() % 16 == 0
    return d[off:], pitch, stride


def even(cols):
    return ((cols + 63) // 64 + 1) & ~1


def fused_pitch(cols, extra=0):
    """the shortest pitch the fused read takes: ceil(cols / 64) * 192"""
    return (cols + 63) // 64 * 192 + extra


def _entries(n, nplanes, plane0):
    """the outputs' order: (frame, plane 8 c + b) of entry (f * 3 + c) * nplanes + k"""
    return [(f, 8 * c + plane0 + k) for f in range(n) for c in range(3) for k in range(nplanes)]


def check(oracle, key, n, rows, cols, plane0, nplanes, pred, got, g, e, want_planes, packed, idx, tag):
    """one call's outputs against the oracle's for each channel of each frame alone"""
    planes, used = _FRAMES[key][1], (cols + 63) // 64
    ent = _entries(n, nplanes, plane0)
    if want_planes:
        # (pad words are the caller's: the count pass writes the words that hold pixels and leaves the prefill, the
        # per-frame extraction writes them 0)
        have = as_u64(got)
        assert np.array_equal(have[:, :, :used], np.stack([planes[f, p] for f, p in ent])), tag
        assert bool(np.all((have[:, :, used:] == 0) | (have[:, :, used:] == np.uint64(0xFFFFFFFFFFFFFFFF)))), tag
    else:
        assert got is None
    for coder, res in ((G, g), (E, e)):
        if res is None:
            continue
        exp = [_stream(oracle, key, f, p, pred, coder) for f, p in ent]
        bits = [int(x) for x in as_u64(res[1])]
        print(tag, "coder", coder, "bits", bits[:24], "expected", [x[0] for x in exp][:24])
        assert bits == [x[0] for x in exp], (tag, coder)
        nw = [(x[0] + 63) // 64 for x in exp]
        if packed:
            offs = [int(x) for x in as_u64(res[2])]
            assert offs == [sum(nw[:i]) for i in range(len(ent) + 1)], (tag, coder)
            assert as_u64(res[0])[:offs[-1]].tobytes() == b"".join(x[1] for x in exp), (tag, coder)
        else:
            for i in range(len(ent)):
                assert stream_bytes(res[0][i], bits[i]) == exp[i][1], (tag, coder, i)
    if idx is not None:
        ri = as_u64(idx).reshape(len(ent), 2 * rows)
        for i, (f, p) in enumerate(ent):
            assert np.array_equal(ri[i], _index(oracle, key, f, p, pred)), (tag, f, p)


def _alone(ctx, d, st, pitch, n, rows, cols, plane0, nplanes, pred, got, g, e, wpr, want_planes, packed, idx, which,
           golomb, eg, tag):
    """frame f's block of 3 * nplanes entries against encode_rgb / encode_rgb_packed of that frame alone, word
    for word (two paths of the library; the oracle comparison came first)"""
    t, m = ctx.torch, 3 * nplanes
    for f in which:
        pl = t.full((m, rows, wpr), -1, dtype=t.int64, device=ctx.dev) if want_planes else None
        kw = dict(rows=rows, cols=cols, pitch=pitch, nplanes=nplanes, plane0=plane0, predict=bool(pred), planes=pl,
                  store_planes=False, wpr=wpr, golomb=golomb, eg=eg)
        idx1 = ctx.empty_i64(m * rows * 2) if packed else None
        if packed:
            got1, g1, e1 = ctx.encode_rgb_packed(d[f * st:], row_index=idx1, **kw)
        else:
            got1, g1, e1 = ctx.encode_rgb(d[f * st:], **kw)
        ctx.sync()
        if want_planes:
            assert t.equal(got[f * m:(f + 1) * m], got1), (tag, f)
        for a, b in ((g, g1), (e, e1)):
            if a is None:
                assert b is None
                continue
            bits = as_u64(a[1])[f * m:(f + 1) * m]
            assert np.array_equal(bits, as_u64(b[1])), (tag, f)
            if packed:
                o, o1 = as_u64(a[2])[f * m:(f + 1) * m + 1], as_u64(b[2])
                assert np.array_equal(o - o[0], o1), (tag, f)
                assert np.array_equal(as_u64(a[0]).reshape(-1)[int(o[0]):int(o[-1])],
                                      as_u64(b[0]).reshape(-1)[:int(o1[-1])]), (tag, f)
            else:
                for i in range(m):
                    assert stream_bytes(a[0][f * m + i], int(bits[i])) == stream_bytes(b[0][i], int(bits[i])), (tag, f, i)
        if packed:
            assert t.equal(idx[f * m * rows * 2:(f + 1) * m * rows * 2], idx1), (tag, f)


def run(ctx, oracle, kind, n, rows, cols, pitch=None, off=16, gap=0, pred=1, plane0=0, nplanes=None, want_planes=False,
        packed=False, wpr=None, gcode=False, ct=0, golomb=True, eg=True, stride=None, alone=None):
    """one call checked against the oracle, then against the single-image call on the frames `alone` (default
    all). pitch defaults to the shortest the fused read takes."""
    key, imgs, _ = frames(oracle, kind, n, rows, cols, ct, gcode)
    nplanes = nplanes or 8 - plane0
    wpr = wpr or even(cols)
    d, pitch, st = buffer(ctx, imgs, pitch or fused_pitch(cols), off, gap)
    st = st if stride is None else stride
    tag = (kind, n, rows, cols, pitch, off, gap, pred, plane0, nplanes, want_planes, packed, wpr, gcode, ct)
    t = ctx.torch
    pl = t.full((n * 3 * nplanes, rows, wpr), -1, dtype=t.int64, device=ctx.dev) if want_planes else None
    idx = None
    kw = dict(nframes=n, frame_stride=st, pitch=pitch, nplanes=nplanes, plane0=plane0, predict=bool(pred), planes=pl,
              wpr=wpr, golomb=golomb, eg=eg)
    if packed:
        idx = ctx.empty_i64(n * 3 * nplanes * rows * 2)
        got, g, e = ctx.encode_rgb_frames_packed(d, rows, cols, row_index=idx, **kw)
    else:
        got, g, e = ctx.encode_rgb_frames(d, rows, cols, **kw)
    ctx.sync()
    check(oracle, key, n, rows, cols, plane0, nplanes, pred, got, g, e, want_planes, packed, idx, tag)
    if n > 1:
        _alone(ctx, d, st, pitch, n, rows, cols, plane0, nplanes, pred, got, g, e, wpr, want_planes, packed, idx,
               range(n) if alone is None else alone, golomb, eg, tag)
    return d, pitch, st, g, e, idx


# 1. planes NULL: with prediction and slots the count pass writes the EG streams itself (EG source, an EG stride
#    per frame and channel); without prediction, and with packed output, the residual planes go to the context's
#    buffer. Frame f's row 0 must not see frame f - 1's last row.
@pytest.mark.parametrize("pred", [1, 0])
def test_eg_source_and_residual_buffer(ctx, oracle, staged, pred):
    run(ctx, oracle, "uniform", 3, 5, 4096, pred=pred)
    run(ctx, oracle, "uniform", 3, 5, 4096, pred=pred, packed=True)


# 2. two strips; planes returned: four rows per wave, 7 rows = a block of 4 and one of 3 that ends with its frame
@pytest.mark.parametrize("pred", [1, 0])
def test_two_strips_planes_returned(ctx, oracle, staged, pred):
    run(ctx, oracle, "uniform", 2, 7, 8192, pred=pred, want_planes=True)


# 3. four strips (the widest row), a smooth input, packed: the EG source's next-segment byte at a frame's last row
def test_four_strips_smooth(ctx, oracle, staged):
    run(ctx, oracle, "smooth", 2, 3, 16384)
    run(ctx, oracle, "smooth", 2, 3, 16384, want_planes=True, packed=True)


# 4. partial words: a last word with pad bits, lanes beyond the row. Pitches 320 and 400 hold the pixels but not
#    the fused read's ceil(cols/64) * 192 bytes (the extraction per frame); 384 and 576 do (the count kernel)
@pytest.mark.parametrize("cols,pitch,wpr", [(100, 320, 2), (130, 400, 4), (100, 384, 2), (130, 576, 4)])
@pytest.mark.parametrize("want", [True, False])
def test_partial_words(ctx, oracle, staged, cols, pitch, wpr, want):
    run(ctx, oracle, "uniform", 4, 9, cols, pitch=pitch, wpr=wpr, want_planes=want)
    run(ctx, oracle, "uniform", 4, 9, cols, pitch=pitch, wpr=wpr, want_planes=want, off=19, gap=5, packed=True)


# 5. an aligned base and pitch with a frame stride that is not (frame 1 is misaligned where frame 0 is not), and
#    one that is: the misaligned-load form chosen from the stride alone
@pytest.mark.parametrize("gap", [37, 16])
@pytest.mark.parametrize("want", [False, True])
def test_odd_stride_aligned_base(ctx, oracle, staged, gap, want):
    run(ctx, oracle, "uniform", 3, 6, 4096, gap=gap, want_planes=want)


# 6. concatenated P6 files with comments as they lie: the headers parsed on the host, the bytes on the device
def test_p6_files(ctx, oracle, staged):
    n, rows, cols = 3, 6, 4096
    key, imgs, _ = frames(oracle, "uniform", n, rows, cols)
    files = [b"P6\n# frame %d\n%d %d\n255\n" % (f, cols, rows) + imgs[f].tobytes() for f in range(n)]
    assert len({len(x) for x in files}) == 1
    data = b"".join(files)
    infos = [pybic.pnm_header(data[f * len(files[0]):]) for f in range(n)]
    for i in infos:
        assert (i.type, i.rows, i.cols, i.maxval, i.data_offset) == (6, rows, cols, 255, infos[0].data_offset)
    stride, off = len(files[0]), infos[0].data_offset
    assert stride % 16 and off % 16
    host = np.concatenate([np.full(16, OUTSIDE, np.uint8), np.frombuffer(data, np.uint8),
                           np.full(80, OUTSIDE, np.uint8)])
    dev = ctx.torch.from_numpy(host).to(ctx.dev)
    for want in (None, True):
        idx = ctx.empty_i64(n * 24 * rows * 2)
        got, g, e = ctx.encode_rgb_frames_packed(dev[16 + off:], rows, cols, nframes=n, frame_stride=stride,
                                                 planes=want, wpr=64, row_index=idx)
        ctx.sync()
        check(oracle, key, n, rows, cols, 0, 8, 1, got, g, e, bool(want), True, idx, ("p6", want))


# 7. plane ranges: the outputs skip (f * 3 + c) * nplanes planes with nplanes < 8
@pytest.mark.parametrize("plane0,nplanes", [(2, 3), (7, 1)])
def test_plane_ranges(ctx, oracle, staged, plane0, nplanes):
    run(ctx, oracle, "uniform", 3, 5, 4096, plane0=plane0, nplanes=nplanes)
    run(ctx, oracle, "uniform", 3, 5, 4096, plane0=plane0, nplanes=nplanes, want_planes=True, off=17, packed=True)


# 8. 3,120 streams in one call: the waves of one workgroup straddle frames
def test_many_streams(ctx, oracle, staged):
    run(ctx, oracle, "uniform", 130, 2, 128, wpr=2, packed=True, alone=(0, 64, 129))
    run(ctx, oracle, "uniform", 130, 2, 128, wpr=2, want_planes=True, gap=3, alone=(1, 128))


# 9. BIC_OPT_COLOR_TRANSFORM 1 and 2, BIC_OPT_GRAY_CODE on and off: the pixel before a strip and the EG source's
#    next-segment byte take their own frame's green
@pytest.mark.parametrize("ct", [1, 2])
@pytest.mark.parametrize("gcode", [False, True])
def test_colour_transform_and_gray_code(ctx, oracle, staged, options, ct, gcode):
    options(gcode, ct)
    run(ctx, oracle, "uniform", 2, 5, 4096, ct=ct, gcode=gcode)
    run(ctx, oracle, "uniform", 2, 5, 4096, ct=ct, gcode=gcode, want_planes=True, off=29, gap=7, packed=True)
    run(ctx, oracle, "uniform", 2, 9, 100, ct=ct, gcode=gcode, wpr=2, packed=True)
    run(ctx, oracle, "uniform", 2, 9, 100, ct=ct, gcode=gcode, wpr=2, want_planes=True, off=21)


def test_gray_code_alone(ctx, oracle, staged, options):
    options(True, 0)
    run(ctx, oracle, "smooth", 2, 5, 4096, gcode=True)
    run(ctx, oracle, "uniform", 2, 9, 100, gcode=True, wpr=2, want_planes=True, packed=True)


def test_sample_predict_is_ignored(ctx, oracle, staged):
    ctx.set_sample_predict(1)
    try:
        run(ctx, oracle, "uniform", 3, 5, 4096, packed=True)
    finally:
        ctx.set_sample_predict(0)


# 10. rows crossing a row block: RPW + 1 rows for both values of the count pass's rows per wave (1 with planes
#     NULL and prediction, 4 otherwise) -- r0 is per frame
def test_rows_crossing_a_row_block(ctx, oracle, staged):
    run(ctx, oracle, "uniform", 2, 2, 4096)                      # RPW 1, the EG source
    run(ctx, oracle, "uniform", 2, 2, 4096, packed=True)         # RPW 1, the residual buffer
    run(ctx, oracle, "uniform", 2, 5, 4096, want_planes=True)    # RPW 4
    run(ctx, oracle, "uniform", 2, 5, 4096, pred=0)              # RPW 4, planes NULL


# 11. a single frame: the stride is ignored, and the outputs are bic_encode_rgb_packed's word for word (a
#     comparison of two paths, after the comparison with the oracle)
@pytest.mark.parametrize("rows,cols", [(5, 4096), (9, 100)])
def test_single_frame(ctx, oracle, staged, rows, cols):
    d, pitch, _, g, e, idx = run(ctx, oracle, "uniform", 1, rows, cols, packed=True, stride=0)
    idx1 = ctx.empty_i64(24 * rows * 2)
    _, g1, e1 = ctx.encode_rgb_packed(d, rows=rows, cols=cols, pitch=pitch, store_planes=False, row_index=idx1,
                                      wpr=even(cols))
    ctx.sync()
    for a, b in ((g, g1), (e, e1)):
        assert ctx.torch.equal(a[1], b[1]) and ctx.torch.equal(a[2], b[2])
        nwords = int(as_u64(a[2])[-1])
        assert ctx.torch.equal(a[0].reshape(-1)[:nwords], b[0].reshape(-1)[:nwords])
    assert ctx.torch.equal(idx, idx1)


# 12. the automatic encoder at this size: the fallback (an extraction per frame, one encode of all planes)
def test_automatic_encoder(ctx, oracle):
    run(ctx, oracle, "uniform", 3, 5, 4096)
    run(ctx, oracle, "uniform", 3, 5, 4096, packed=True, want_planes=True, gap=37)


def test_launches(ctx, oracle, staged):
    """which kernels a call launches (bic_prof_collect's names), so that the cases above test the path they are
    meant to: one count pass of its own name for all frames where it applies, an extraction per frame otherwise"""
    _, imgs, _ = frames(oracle, "uniform", 3, 5, 4096)
    d, pitch, st = buffer(ctx, imgs, gap=37)
    ctx.sync()
    ctx.prof_collect()
    ctx.prof_enable(True)
    try:
        ctx.prof_only(None)
        for pl in (None, True):
            ctx.encode_rgb_frames(d, 5, 4096, nframes=3, frame_stride=st, planes=pl)
            got = ctx.prof_collect()
            assert got["rgb_frames_count"][0] == 1 and "encode_prefix" in got, got
            assert not [k for k in got if k.startswith("bitplanes")], got
        ctx.encode_rgb_frames(d, 5, 4096, nframes=3, frame_stride=st)
        got = ctx.prof_collect()
        assert got["rgb_frames_count"][0] == 1 and "encode_rows_golomb_egsrc" in got, got
        ctx.encode_rgb_frames(d, 5, 4096, nframes=3, frame_stride=st, wpr=65)  # an odd row pitch
        got = ctx.prof_collect()
        assert "rgb_frames_count" not in got and "bitplanes_count" not in got and got["bitplanes_rgb"][0] == 3, got
        ctx.encode_rgb_frames(d, 5, 4096, nframes=1, frame_stride=st)  # one frame: the single-image call
        got = ctx.prof_collect()
        assert "rgb_frames_count" not in got and got["bitplanes_count"][0] == 1, got
    finally:
        ctx.prof_only(None)
        ctx.prof_enable(False)


def test_rejects(ctx):
    t = ctx.torch
    r = t.zeros(4096, dtype=t.uint8, device=ctx.dev)
    o, b, f, idx = ctx.empty_i64(72 * 64), ctx.empty_i64(72), ctx.empty_i64(73), ctx.empty_i64(72 * 10 * 2)
    o.fill_(0x5A5A)
    lib, h, p = ctx.lib, ctx.h, lambda x: None if x is None else x.data_ptr()

    def enc(rgb=r, stride=640, n=3, pitch=64, rows=10, cols=16, plane0=0, npl=8, wpr=2, og=o, bg=b):
        return lib.bic_encode_rgb_frames(h, p(rgb), stride, n, pitch, rows, cols, plane0, npl, None, wpr, 1, p(og), 64,
                                         p(bg), None, 64, None)

    def encp(fg=f, og=o, oe=None, fe=None, npl=8):
        return lib.bic_encode_rgb_frames_packed(h, p(r), 640, 3, 64, 10, 16, 0, npl, None, 2, 1, p(og), 64, p(b), p(fg),
                                                p(oe), 64, p(b), p(fe), None)

    def dec(coder=G, n=3, npl=8, plane0=0, rows=10, cols=16, pitch=64, stride=640, index=idx, rgb=r, streams=o, off=f):
        return lib.bic_decode_rgb_frames(h, coder, p(streams), 0, p(off), p(b), p(index), n, plane0, npl, rows, cols, 1,
                                         None, p(rgb), pitch, stride)

    ctx._bind_stream()
    assert enc() == pybic.BIC_OK and encp() == pybic.BIC_OK
    ctx.sync()
    keep = o.clone()
    E_ = pybic.BIC_EINVAL
    assert enc(n=0) == E_ and enc(n=-1) == E_             # nframes < 1
    assert enc(n=2731) == E_                              # nframes * 3 * nplanes > 65535
    assert enc(plane0=1) == E_ and enc(plane0=-1, npl=2) == E_ and enc(npl=0) == E_ and enc(npl=9) == E_
    assert encp(npl=0) == E_ and encp(npl=9) == E_
    assert enc(pitch=47) == E_                            # pitch < 3 * cols
    assert enc(stride=639) == E_                          # frames overlap
    assert enc(stride=0, n=1) == pybic.BIC_OK             # one frame: the stride is ignored
    ctx.sync()
    keep = o.clone()
    assert enc(rgb=None) == E_
    assert enc(cols=0) == E_ and enc(wpr=0) == E_         # geometry
    assert enc(rows=1 << 20, cols=1 << 12, pitch=3 << 12, stride=1 << 34) == E_      # rows * (cols + 1) >= 2^31
    assert enc(og=None, bg=None) == E_ and enc(bg=None) == E_
    assert encp(fg=None) == E_ and encp(oe=o, fe=None) == E_
    ctx.sync()
    assert t.equal(o, keep)                               # a rejected call writes nothing
    assert dec(n=0) == E_ and dec(n=2731) == E_
    assert dec(plane0=1) == E_ and dec(npl=0) == E_ and dec(npl=9) == E_
    assert dec(pitch=47) == E_ and dec(stride=639) == E_
    assert dec(index=None) == E_ and dec(coder=A, index=None) == E_ and dec(coder=3) == E_
    assert dec(cols=16385, pitch=3 * 16385, stride=1 << 20) == E_
    assert dec(rgb=None) == E_ and dec(streams=None) == E_ and dec(off=None) == E_
    ctx.sync()
    assert bool((r == 0).all())


def test_no_rows(ctx):
    t = ctx.torch
    r = t.zeros(64, dtype=t.uint8, device=ctx.dev)
    out = t.full((18 * 8,), 0x5A5A, dtype=t.int64, device=ctx.dev)
    seven = lambda k: t.full((k,), 7, dtype=t.int64, device=ctx.dev)  # noqa: E731
    _, (og, bg), (oe, be) = ctx.encode_rgb_frames(r, 0, 16, nframes=3, nplanes=2, slots=(8, 8),
                                                  outs=(out.clone(), out.clone()), bits=(seven(18), seven(18)))
    _, (pg, cg, fg), (pe, ce, fe) = ctx.encode_rgb_frames_packed(r, 0, 16, nframes=3, nplanes=2, slots=(8, 8),
                                                                 outs=(out.clone(), out.clone()),
                                                                 offs=(seven(19), seven(19)))
    ctx.sync()
    for x in (bg, be, cg, ce):
        assert list(as_u64(x)) == [0] * 18
    for x in (fg, fe):
        assert list(as_u64(x)) == [0] * 19
    for x in (og, oe, pg, pe):
        assert t.equal(x.reshape(-1), out)
    buf = t.full((64,), 0x5A, dtype=t.uint8, device=ctx.dev)
    ctx.decode_rgb_frames(E, og, bg, 3, 2, 0, 16, out=buf)
    ctx.sync()
    assert bool((buf == 0x5A).all())
