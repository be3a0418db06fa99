"""BIC_OPT_RGB_PREDICT on the device: the RGB calls code U(img) = T_sp(T_ct(img)) and give the image back.
Expected planes, streams and row indices are the oracle's (bo_bitplanes, bo_encode_plane, bo_row_index) on channel
c of rgb_predict_ref.forward(img) -- numpy arithmetic, Gray-coded with graycode_ref.gray where that option is on --
taken as a gray image; expected samples are the input image, or numpy arithmetic on it. Nothing the library
produced is ever an expected value. Inputs are uniform random bytes: U is a bijection on a row, so every plane of
U(img) is Bernoulli(0.5) and one wrong neighbour at one column changes a stream. All comparisons are exact; the
shapes are the smallest at which each mechanism (a strip boundary, a partial strip, the misaligned loader, the
separate calls, a carry across the inverse kernel's pieces) can go wrong."""
import numpy as np
import pytest

import pybic
import rgb_predict_ref
from graycode_ref import gray
from pybic import as_u64, stream_bytes

pytestmark = pytest.mark.gpu
G, E = pybic.CODER_GOLOMB, pybic.CODER_EG
PAD, OUTSIDE, SENTINEL = 0xC3, 0xA5, 0x5A


@pytest.fixture
def staged(ctx):
    """the staged encoder (and with it the fused count pass) at test sizes"""
    ctx.set_encoder("staged")
    yield
    ctx.set_encoder("auto")


@pytest.fixture
def opts(ctx):
    """set(mode, ct, gcode) for one test; options 7, 8 and 10 at their defaults again afterwards"""
    def set_(mode, ct=0, gcode=False):
        ctx.set_gray_code(bool(gcode))
        ctx.set_color_transform(ct)
        ctx.set_rgb_predict(mode)
    yield set_
    ctx.set_gray_code(False)
    ctx.set_color_transform(0)
    ctx.set_rgb_predict(0)
    ctx.set_sample_predict(0)


_IMG, _PLANES, _STREAM, _INDEX = {}, {}, {}, {}


def image(oracle, rows, cols, f=0):
    """a seeded uniform image [rows, cols, 3], made once and read-only; pixel (0,0) all ones"""
    key = (rows, cols, f)
    if key not in _IMG:
        a = oracle.gen_bytes(0x10A9D + 7919 * f + 131 * rows + cols, rows * cols * 3).reshape(rows, cols, 3).copy()
        a[0, 0] = 0xFF
        a.setflags(write=False)
        _IMG[key] = a
    return _IMG[key]


def planes_of(oracle, rows, cols, mode, ct, gcode, f=0):
    """-> (key, the oracle's planes [24, rows, used] of U(img): plane 8 c + b = bit b of channel c), made once"""
    key = (rows, cols, f, mode, ct, bool(gcode))
    if key not in _PLANES:
        v = rgb_predict_ref.forward(image(oracle, rows, cols, f), ct, mode)
        v = gray(v) if gcode else v
        p = np.concatenate([oracle.bitplanes(np.ascontiguousarray(v[:, :, c]), 8) for c in range(3)])
        p.setflags(write=False)
        _PLANES[key] = p
    return key, _PLANES[key]


def _stream(oracle, key, p, pred, coder):
    q = (key, p, pred, coder)
    if q not in _STREAM:
        eb, est, _ = oracle.encode_plane(_PLANES[key][p], key[1], pred, coder)
        _STREAM[q] = (eb, est.tobytes())
    return _STREAM[q]


def _index(oracle, key, p, pred):
    q = (key, p, pred)
    if q not in _INDEX:
        _INDEX[q] = oracle.row_index(_PLANES[key][p], key[1], pred)
    return _INDEX[q]


def even(cols):
    return ((cols + 63) // 64 + 1) & ~1


def fused_pitch(cols, extra=0):
    """the shortest pitch the fused read takes: ceil(cols / 64) * 192"""
    return (cols + 63) // 64 * 192 + extra


def buffer(ctx, imgs, pitch, off=16, gap=0):
    """the frames' bytes `off` bytes into a 16-byte aligned device buffer, rows `pitch` and frames rows * pitch +
    gap bytes apart; PAD behind a row's samples, OUTSIDE everywhere else -> (view at frame 0's first sample, stride)"""
    n, rows, cols, _ = imgs.shape
    stride = rows * pitch + gap
    buf = np.full(off + n * stride + 256, OUTSIDE, np.uint8)
    for f in range(n):
        r = np.full((rows, pitch), PAD, np.uint8)
        r[:, :3 * cols] = imgs[f].reshape(rows, 3 * cols)
        buf[off + f * stride:off + f * stride + rows * pitch] = r.reshape(-1)
    d = ctx.torch.from_numpy(buf).to(ctx.dev)
    assert d.data_ptr() % 16 == 0
    return d[off:], stride


def check(oracle, keys, cols, plane0, nplanes, pred, got, g, e, want_planes, packed, idx, tag):
    """one call's outputs (entry (f * 3 + c) * nplanes + k) against the oracle's for each channel of each frame"""
    used, rows = (cols + 63) // 64, keys[0][0]
    ent = [(key, 8 * c + plane0 + k) for key in keys for c in range(3) for k in range(nplanes)]
    if want_planes:
        have = as_u64(got)
        assert np.array_equal(have[:, :, :used], np.stack([_PLANES[key][p] for key, p in ent])), tag
    else:
        assert got is None
    for coder, res in ((G, g), (E, e)):
        exp = [_stream(oracle, key, p, pred, coder) for key, p in ent]
        bits = [int(x) for x in as_u64(res[1])]
        print(tag, "coder", coder, "bits", bits[:6], "expected", [x[0] for x in exp][:6])
        assert bits == [x[0] for x in exp], (tag, coder)
        if packed:
            nw = [(x[0] + 63) // 64 for x in exp]
            offs = [int(x) for x in as_u64(res[2])]
            assert offs == [sum(nw[:i]) for i in range(len(ent) + 1)], (tag, coder)
            assert as_u64(res[0])[:offs[-1]].tobytes() == b"".join(x[1] for x in exp), (tag, coder)
        else:
            for i in range(len(ent)):
                assert stream_bytes(res[0][i], bits[i]) == exp[i][1], (tag, coder, i)
    if idx is not None:
        ri = as_u64(idx).reshape(len(ent), 2 * rows)
        for i, (key, p) in enumerate(ent):
            assert np.array_equal(ri[i], _index(oracle, key, p, pred)), (tag, i)


def encode(ctx, oracle, rows, cols, mode, ct=0, gcode=False, pred=1, want_planes=False, pitch=None, off=16, plane0=0,
           nplanes=None, packed=False, prof=None):
    """one bic_encode_rgb / _packed call against the oracle. prof: "fused" -- one count kernel, no bitplanes_rgb"""
    key, _ = planes_of(oracle, rows, cols, mode, ct, gcode)
    nplanes = nplanes or 8 - plane0
    pitch = pitch or fused_pitch(cols)
    wpr = even(cols)
    d, _ = buffer(ctx, image(oracle, rows, cols)[None], pitch, off)
    t = ctx.torch
    pl = t.full((3 * nplanes, rows, wpr), -1, dtype=t.int64, device=ctx.dev) if want_planes else None
    kw = dict(rows=rows, cols=cols, pitch=pitch, nplanes=nplanes, plane0=plane0, predict=bool(pred), planes=pl,
              store_planes=False, wpr=wpr)
    idx = ctx.empty_i64(3 * nplanes * rows * 2) if packed else None
    tag = (rows, cols, mode, ct, gcode, pred, want_planes, pitch, off, plane0, nplanes, packed)
    if prof:
        ctx.sync()
        ctx.prof_collect()
        ctx.prof_enable(True)
    try:
        if packed:
            got, g, e = ctx.encode_rgb_packed(d, row_index=idx, **kw)
        else:
            got, g, e = ctx.encode_rgb(d, **kw)
        if prof:
            launches = ctx.prof_collect()
    finally:
        if prof:
            ctx.prof_enable(False)
    ctx.sync()
    check(oracle, [key], cols, plane0, nplanes, pred, got, g, e, want_planes, packed, idx, tag)
    if prof == "fused":
        assert launches["bitplanes_count"][0] == 1, launches
        assert not [k for k in launches if k.startswith("bitplanes_rgb")], launches
    return d, pitch, g, e, idx


# ---- encode ---------------------------------------------------------------------------------------------------
# 33 x 4096: one whole strip, with planes NULL and prediction the count pass writes the EG stream itself.
# 24 x 8192: lb and the EG source's next-segment bytes across a strip boundary.
@pytest.mark.parametrize("mode,ct,gcode", [(1, 0, False), (1, 1, False), (1, 2, False), (2, 0, False), (2, 1, False),
                                           (2, 2, False), (2, 1, True)])
@pytest.mark.parametrize("rows,cols", [(33, 4096), (24, 8192)])
def test_encode_whole_strips(ctx, oracle, staged, opts, rows, cols, mode, ct, gcode):
    opts(mode, ct, gcode)
    for pred in (1, 0):
        for want in (False, True):
            encode(ctx, oracle, rows, cols, mode, ct, gcode, pred=pred, want_planes=want, prof="fused")


# 9 x 4100 with a padded pitch: a partial second strip, pad bits; 5 x 70: one partial strip
@pytest.mark.parametrize("rows,cols,extra", [(9, 4100, 16), (5, 70, 0)])
def test_encode_partial_strips(ctx, oracle, staged, opts, rows, cols, extra):
    opts(2, 1)
    for pred in (1, 0):
        for want in (False, True):
            encode(ctx, oracle, rows, cols, 2, 1, pred=pred, want_planes=want, pitch=fused_pitch(cols, extra),
                   prof="fused")


# the misaligned loader: byte offset 3 and an odd pitch (exactness alone)
def test_encode_misaligned(ctx, oracle, staged, opts):
    opts(2, 1)
    for pred in (1, 0):
        for want in (False, True):
            encode(ctx, oracle, 33, 4096, 2, 1, pred=pred, want_planes=want, pitch=fused_pitch(4096, 5), off=16 + 3)


# the plane-range shift
def test_encode_plane_range(ctx, oracle, staged, opts):
    opts(2, 1)
    for pred in (1, 0):
        for want in (False, True):
            encode(ctx, oracle, 24, 8192, 2, 1, pred=pred, want_planes=want, plane0=3, nplanes=4, prof="fused")


# past 16384 columns: the separate calls (bic_bitplanes_rgb, then the chunk kernels)
def test_encode_wide_rows(ctx, oracle, staged, opts):
    opts(2, 1)
    for pred in (1, 0):
        for want in (False, True):
            encode(ctx, oracle, 2, 16448, 2, 1, pred=pred, want_planes=want, pitch=3 * 16448)


def test_encode_packed(ctx, oracle, staged, opts):
    """bic_encode_rgb_packed: offsets and row index"""
    opts(2, 1)
    for pred in (1, 0):
        for want in (False, True):
            encode(ctx, oracle, 24, 8192, 2, 1, pred=pred, want_planes=want, packed=True)


# ---- frames ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,rows,cols,extra,gap,off,fused", [(3, 20, 4096, 0, 32, 16, True),
                                                              (2, 9, 4100, 16, 48, 16 + 3, False)])
def test_frames(ctx, oracle, staged, opts, n, rows, cols, extra, gap, off, fused):
    """every frame's block is the oracle's on that frame alone (a frame's column 0 has no left neighbour, its row
    0 no row above) and, after that comparison, bit for bit the single-image call's on that frame"""
    mode, ct = 2, 1
    opts(mode, ct)
    keys = [planes_of(oracle, rows, cols, mode, ct, False, f)[0] for f in range(n)]
    imgs = np.stack([image(oracle, rows, cols, f) for f in range(n)])
    pitch, wpr, t = fused_pitch(cols, extra), even(cols), ctx.torch
    d, st = buffer(ctx, imgs, pitch, off, gap)
    for pred in (1, 0):
        for want in (False, True):
            for packed in (False, True):
                pl = t.full((n * 24, rows, wpr), -1, dtype=t.int64, device=ctx.dev) if want else None
                kw = dict(nframes=n, frame_stride=st, pitch=pitch, predict=bool(pred), planes=pl, wpr=wpr)
                idx = ctx.empty_i64(n * 24 * rows * 2) if packed else None
                ctx.sync()
                ctx.prof_collect()
                ctx.prof_enable(True)
                try:
                    if packed:
                        got, g, e = ctx.encode_rgb_frames_packed(d, rows, cols, row_index=idx, **kw)
                    else:
                        got, g, e = ctx.encode_rgb_frames(d, rows, cols, **kw)
                    launches = ctx.prof_collect()
                finally:
                    ctx.prof_enable(False)
                ctx.sync()
                tag = (n, rows, cols, pred, want, packed)
                check(oracle, keys, cols, 0, 8, pred, got, g, e, want, packed, idx, tag)
                if fused:
                    assert launches["rgb_frames_count"][0] == 1, launches
                    assert not [k for k in launches if k.startswith("bitplanes")], launches
                if packed:
                    continue
                for f in range(n):  # the single-image call on frame f (two paths of the library)
                    pl1 = t.full((24, rows, wpr), -1, dtype=t.int64, device=ctx.dev) if want else None
                    got1, g1, e1 = ctx.encode_rgb(d[f * st:], rows=rows, cols=cols, pitch=pitch, predict=bool(pred),
                                                  planes=pl1, store_planes=False, wpr=wpr)
                    ctx.sync()
                    if want:
                        assert t.equal(got[24 * f:24 * f + 24], got1), (tag, f)
                    for a, b in ((g, g1), (e, e1)):
                        bits = as_u64(a[1])[24 * f:24 * f + 24]
                        assert np.array_equal(bits, as_u64(b[1])), (tag, f)
                        for i in range(24):
                            assert stream_bytes(a[0][24 * f + i], int(bits[i])) == stream_bytes(b[0][i], int(bits[i]))


# ---- bic_bitplanes_rgb and bic_planes_to_rgb ------------------------------------------------------------------
_MODES = [(1, 0, False), (2, 0, False), (2, 1, False), (2, 1, True), (1, 2, True)]


def _sink(ctx, rows, pitch, lead):
    total = lead + rows * pitch + 48
    out = ctx.torch.full((total,), SENTINEL, dtype=ctx.torch.uint8, device=ctx.dev)
    assert out.data_ptr() % 16 == 0
    return out, total


def _sink_check(out, total, want, rows, cols, pitch, lead, tag):
    """the samples where they belong, the sentinel everywhere else (pitch padding, the bytes around)"""
    exp = np.full(total, SENTINEL, np.uint8)
    for r in range(rows):
        exp[lead + r * pitch:lead + r * pitch + 3 * cols] = want[r].reshape(-1)
    got = out.cpu().numpy()
    assert np.array_equal(got, exp), (tag, np.flatnonzero(got != exp)[:8])


# 21 x 1000: byte stores; 8 x 1024 at a 16-byte aligned row: vector stores, one piece; 6 x 2100: a carry across
# the inverse kernel's pieces of 1024 pixels (aligned rows: vector stores and a byte tail)
@pytest.mark.parametrize("rows,cols,lead,slack", [(21, 1000, 16 + 3, 5), (8, 1024, 16, 16), (6, 2100, 16, 12)])
@pytest.mark.parametrize("mode,ct,gcode", _MODES)
def test_bitplanes_and_back(ctx, oracle, opts, rows, cols, lead, slack, mode, ct, gcode):
    opts(mode, ct, gcode)
    img = image(oracle, rows, cols)
    _, planes = planes_of(oracle, rows, cols, mode, ct, gcode)
    pitch = 3 * cols + slack
    d, _ = buffer(ctx, img[None], pitch, lead)
    got = ctx.bitplanes_rgb(d, rows=rows, cols=cols, pitch=pitch)
    ctx.sync()
    assert np.array_equal(as_u64(got), planes), (rows, cols, mode, ct, gcode)
    # and back, from the oracle's planes
    pl = ctx.torch.from_numpy(planes.view(np.int64).copy()).to(ctx.dev)
    out, total = _sink(ctx, rows, pitch, lead)
    ctx.planes_to_rgb(pl, cols, out=out[lead:], pitch=pitch)
    ctx.sync()
    _sink_check(out, total, img, rows, cols, pitch, lead, (rows, cols, mode, ct, gcode))


def _range_formula(img, plane0, nplanes, mode, ct, gcode):
    """what a plane range gives back: each channel's z cut to the covered bits (after the un-Gray step and its
    mask), unfolded, summed along the row, then the inverse colour transform -- all eight bits"""
    m = np.uint8(((1 << nplanes) - 1) << plane0)
    z = rgb_predict_ref.forward(img, ct, mode)
    if gcode:
        x = gray(z) & m
        x = x ^ (x >> 1)
        x = x ^ (x >> 2)
        x = x ^ (x >> 4)
        z = x
    return rgb_predict_ref.inverse(z & m, ct, mode)


def test_planes_to_rgb_plane_range(ctx, oracle, opts):
    rows, cols, plane0, nplanes = 6, 2100, 2, 5
    img = image(oracle, rows, cols)
    for mode, ct, gcode in _MODES:
        opts(mode, ct, gcode)
        _, planes = planes_of(oracle, rows, cols, mode, ct, gcode)
        sel = np.concatenate([planes[8 * c + plane0:8 * c + plane0 + nplanes] for c in range(3)])
        pl = ctx.torch.from_numpy(sel.view(np.int64).copy()).to(ctx.dev)
        pitch, lead = 3 * cols + 12, 16
        out, total = _sink(ctx, rows, pitch, lead)
        ctx.planes_to_rgb(pl, cols, plane0=plane0, out=out[lead:], pitch=pitch)
        ctx.sync()
        want = _range_formula(img, plane0, nplanes, mode, ct, gcode)
        assert not np.array_equal(want, img)
        _sink_check(out, total, want, rows, cols, pitch, lead, (mode, ct, gcode))


# ---- round trips ----------------------------------------------------------------------------------------------
_TRIPS = [(1, 0, False), (2, 0, False), (2, 1, False), (2, 1, True)]


def _p00(ctx, imgs, plane0, nplanes, mode, ct, gcode):
    p = np.concatenate([pybic.rgb_p00_predict(ct, mode, gcode, a[0, 0], plane0, nplanes) for a in imgs])
    return ctx.torch.from_numpy(p).to(ctx.dev)


# 40 x 4096 at offset 0 (vector loads and stores); at offset 3 with 5 bytes of pitch slack; 24 x 4100
@pytest.mark.parametrize("rows,cols,lead,slack", [(40, 4096, 16, 0), (40, 4096, 16 + 3, 5), (24, 4100, 16, 4)])
@pytest.mark.parametrize("mode,ct,gcode", _TRIPS)
def test_round_trip(ctx, oracle, staged, opts, rows, cols, lead, slack, mode, ct, gcode):
    """bic_encode_rgb_packed -> bic_decode_rgb gives the input image, from the Golomb and the EG streams"""
    opts(mode, ct, gcode)
    img = image(oracle, rows, cols)
    for pred in (1, 0):
        d, pitch, g, e, idx = encode(ctx, oracle, rows, cols, mode, ct, gcode, pred=pred, packed=True,
                                     pitch=fused_pitch(cols, slack), off=lead)
        p00 = _p00(ctx, [img], 0, 8, mode, ct, gcode) if pred else None
        opitch = 3 * cols + slack
        for coder, (streams, bits, off), ri in ((G, g, idx), (E, e, None)):
            out, total = _sink(ctx, rows, opitch, lead)
            ctx.decode_rgb(coder, streams, bits, 8, rows, cols, bool(pred), word_off=off, row_index=ri, p00=p00,
                           out=out[lead:], pitch=opitch)
            ctx.sync()
            _sink_check(out, total, img, rows, cols, opitch, lead, (rows, cols, mode, ct, gcode, pred, coder))


@pytest.mark.parametrize("mode,ct,gcode", _TRIPS)
def test_round_trip_frames(ctx, oracle, staged, opts, mode, ct, gcode):
    """the same through the frame calls; the gap between the frames keeps the caller's bytes"""
    n, rows, cols, gap, lead = 3, 20, 4096, 37, 16 + 3
    opts(mode, ct, gcode)
    imgs = np.stack([image(oracle, rows, cols, f) for f in range(n)])
    pitch = fused_pitch(cols, 7)
    d, st = buffer(ctx, imgs, pitch, lead, 9)
    for pred in (1, 0):
        idx = ctx.empty_i64(n * 24 * rows * 2)
        _, g, e = ctx.encode_rgb_frames_packed(d, rows, cols, nframes=n, frame_stride=st, pitch=pitch,
                                               predict=bool(pred), wpr=even(cols), row_index=idx)
        p00 = _p00(ctx, imgs, 0, 8, mode, ct, gcode) if pred else None
        opitch = 3 * cols + 5
        stride = rows * opitch + gap
        for coder, (streams, bits, off), ri in ((G, g, idx), (E, e, None)):
            total = lead + (n - 1) * stride + rows * opitch + 48
            out = ctx.torch.full((total,), SENTINEL, dtype=ctx.torch.uint8, device=ctx.dev)
            ctx.decode_rgb_frames(coder, streams, bits, n, 8, rows, cols, bool(pred), word_off=off, row_index=ri,
                                  p00=p00, out=out[lead:], pitch=opitch, frame_stride=stride)
            ctx.sync()
            exp = np.full(total, SENTINEL, np.uint8)
            for f in range(n):
                for r in range(rows):
                    o = lead + f * stride + r * opitch
                    exp[o:o + 3 * cols] = imgs[f, r].reshape(-1)
            got = out.cpu().numpy()
            assert np.array_equal(got, exp), (mode, ct, gcode, pred, coder, np.flatnonzero(got != exp)[:8])


def test_decode_plane_range(ctx, oracle, staged, opts):
    """plane0 = 2, nplanes = 5: the result is the header's formula, computed in numpy"""
    rows, cols, plane0, nplanes = 24, 4100, 2, 5
    img = image(oracle, rows, cols)
    for mode, ct, gcode in _TRIPS:
        opts(mode, ct, gcode)
        d, pitch, g, e, idx = encode(ctx, oracle, rows, cols, mode, ct, gcode, packed=True, plane0=plane0,
                                     nplanes=nplanes)
        p00 = _p00(ctx, [img], plane0, nplanes, mode, ct, gcode)
        want = _range_formula(img, plane0, nplanes, mode, ct, gcode)
        opitch, lead = 3 * cols + 4, 16
        for coder, (streams, bits, off), ri in ((G, g, idx), (E, e, None)):
            out, total = _sink(ctx, rows, opitch, lead)
            ctx.decode_rgb(coder, streams, bits, nplanes, rows, cols, True, word_off=off, row_index=ri, p00=p00,
                           plane0=plane0, out=out[lead:], pitch=opitch)
            ctx.sync()
            _sink_check(out, total, want, rows, cols, opitch, lead, (mode, ct, gcode, coder))


# ---- option hygiene -------------------------------------------------------------------------------------------
def test_option_off_after_on(ctx, oracle, staged, opts):
    rows, cols = 33, 4096
    opts(2, 1)
    encode(ctx, oracle, rows, cols, 2, 1)
    opts(0, 0)
    for want in (False, True):
        encode(ctx, oracle, rows, cols, 0, 0, want_planes=want)  # the option-off oracle streams


def test_option_rejects_other_values(ctx, oracle, opts):
    rows, cols = 5, 70
    d, _ = buffer(ctx, image(oracle, rows, cols)[None], 3 * cols)
    for mode in (0, 1, 2):
        opts(mode)
        for bad in (3, -1):
            with pytest.raises(pybic.BicError) as err:
                ctx.set_rgb_predict(bad)
            assert err.value.code == pybic.BIC_EINVAL
        got = ctx.bitplanes_rgb(d, rows=rows, cols=cols, pitch=3 * cols)
        ctx.sync()
        assert np.array_equal(as_u64(got), planes_of(oracle, rows, cols, mode, 0, False)[1]), mode  # the setting stayed


def test_other_sample_kinds_ignore_option_10(ctx, oracle, staged, opts):
    """mode 2 on: one- and two-byte gray samples and P4 rasters still give the option-off oracle streams"""
    opts(2)

    def check_(planes, cols, g, e, tag):
        for k in range(planes.shape[0]):
            for coder, (out, bits) in ((G, g), (E, e)):
                eb, est, _ = oracle.encode_plane(planes[k], cols, 1, coder)
                nb = int(as_u64(bits)[k])
                assert nb == eb and stream_bytes(out[k], nb) == est.tobytes(), (tag, k, coder)

    rows, cols = 20, 4096
    gray8 = oracle.gen_bytes(0x8B17, rows * cols).reshape(rows, cols)
    _, g, e = ctx.encode_gray(ctx.torch.from_numpy(gray8.copy()).to(ctx.dev), store_planes=False)
    ctx.sync()
    check_(oracle.bitplanes(gray8, 8), cols, g, e, "gray")

    img16 = oracle.gen_bytes(0x16B17, 2 * rows * cols).view(np.uint16).reshape(rows, cols)
    d = ctx.torch.from_numpy(img16.astype("<u2").view(np.uint8).reshape(rows, 2 * cols).copy()).to(ctx.dev)
    _, g, e = ctx.encode_gray16(d, rows=rows, cols=cols, store_planes=False)
    ctx.sync()
    check_(oracle.bitplanes(img16, 16), cols, g, e, "gray16")

    bits = oracle.gen_bytes(0xB17, rows * cols // 8).reshape(rows, cols // 8)
    _, g, e = ctx.encode_pbm(ctx.torch.from_numpy(bits.reshape(-1).copy()).to(ctx.dev), rows, cols)
    ctx.sync()
    plane = bits.reshape(rows, cols // 64, 8).astype(np.uint64)
    word = np.zeros((rows, cols // 64), np.uint64)
    for b in range(8):  # big-endian: the first byte holds the leftmost pixels
        word |= plane[:, :, b] << np.uint64(56 - 8 * b)
    check_(word[None], cols, g, e, "pbm")


def test_rgb_calls_ignore_option_9(ctx, oracle, staged, opts):
    opts(0, 1)
    ctx.set_sample_predict(2)
    encode(ctx, oracle, 33, 4096, 0, 1)                      # the option-off result (CT 1 alone)
    encode(ctx, oracle, 33, 4096, 0, 1, want_planes=True)
    opts(2, 1)
    ctx.set_sample_predict(1)
    encode(ctx, oracle, 33, 4096, 2, 1)                      # and option 10's result with option 9 set to another mode


def test_profile_names_the_inverse_kernel(ctx, oracle, staged, opts):
    """rgb_unpredict: once in a decode with the option on, not at all with it off"""
    rows, cols = 24, 4100
    img = image(oracle, rows, cols)
    for mode in (2, 0):
        opts(mode, 1)
        d, pitch, g, e, idx = encode(ctx, oracle, rows, cols, mode, 1, packed=True)
        p00 = _p00(ctx, [img], 0, 8, mode, 1, False)
        ctx.sync()
        ctx.prof_collect()
        ctx.prof_enable(True)
        try:
            out = ctx.decode_rgb(G, g[0], g[1], 8, rows, cols, True, word_off=g[2], row_index=idx, p00=p00)
            launches = ctx.prof_collect()
        finally:
            ctx.prof_enable(False)
        assert np.array_equal(out.cpu().numpy().reshape(rows, cols, 3), img)
        if mode:
            assert launches["rgb_unpredict"][0] == 1, launches
        else:
            assert "rgb_unpredict" not in launches, launches
