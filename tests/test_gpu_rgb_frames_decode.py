"""bic_decode_rgb_frames: the device round trip RGB frames -> bic_encode_rgb_frames(_packed) ->
bic_decode_rgb_frames for the Golomb and EG streams (the encoder's outputs are checked against the oracle in
test_gpu_rgb_frames.py), and the adaptive EG streams of the oracle's planes. Every decode goes into a buffer filled
with a sentinel, frame 0 some bytes in: the samples must equal the input frames' (at plane0 = 0, nplanes = 8 the
image exactly; for a plane range the range's bits), and every byte outside the first 3 * cols bytes of each row of
each frame -- pitch padding, the gap between frames, the bytes around the buffer -- must keep the sentinel."""
import numpy as np
import pytest

import colour_ref
import pybic
from graycode_ref import gray
from test_gpu_rgb_frames import buffer, even, frames, fused_pitch

pytestmark = pytest.mark.gpu
G, E, A = pybic.CODER_GOLOMB, pybic.CODER_EG, pybic.CODER_EG_ADAPTIVE
SENTINEL = 0x5A


@pytest.fixture
def staged(ctx):
    ctx.set_encoder("staged")
    yield
    ctx.set_encoder("auto")


@pytest.fixture
def options(ctx):
    def set_(gcode, ct):
        ctx.set_gray_code(bool(gcode))
        ctx.set_color_transform(ct)
    yield set_
    ctx.set_gray_code(False)
    ctx.set_color_transform(0)


def _p00(ctx, imgs, plane0, nplanes, gcode, ct):
    """one byte per stream: rgb_frames_p00 of the frames' first pixels"""
    p = pybic.rgb_frames_p00(ct, gcode, [a[0, 0] for a in imgs], plane0, nplanes)
    return ctx.torch.from_numpy(p).to(ctx.dev)


def _expect(imgs, plane0, nplanes, gcode, ct):
    """the samples the range's planes give back: the transformed (and Gray-coded) samples cut to the covered bits,
    un-Gray-coded within them, then the inverse transform. The whole range: the image."""
    if plane0 == 0 and nplanes == 8:
        return imgs
    m = np.uint8(((1 << nplanes) - 1) << plane0)
    v = colour_ref.forward(imgs, ct)
    if gcode:
        x = gray(v) & m
        x = x ^ (x >> 1)
        x = x ^ (x >> 2)
        x = x ^ (x >> 4)
        v = x
    return colour_ref.inverse(v & m, ct)


def _decode_check(ctx, coder, streams, bits, off, idx, want, plane0, nplanes, pred, p00, lead, pitch, gap, tag):
    n, rows, cols, _ = want.shape
    stride = rows * pitch + gap
    total = lead + (n - 1) * stride + rows * pitch + 48
    out = ctx.torch.full((total,), SENTINEL, dtype=ctx.torch.uint8, device=ctx.dev)
    assert out.data_ptr() % 16 == 0
    ctx.decode_rgb_frames(coder, streams, bits, n, nplanes, rows, cols, bool(pred), word_off=off, row_index=idx,
                          p00=p00, plane0=plane0, out=out[lead:], pitch=pitch, frame_stride=stride)
    ctx.sync()
    exp = np.full(total, SENTINEL, np.uint8)
    src = want.reshape(n, rows, 3 * cols)
    for f in range(n):
        for r in range(rows):
            o = lead + f * stride + r * pitch
            exp[o:o + 3 * cols] = src[f, r]
    got = out.cpu().numpy()
    assert np.array_equal(got, exp), (tag, coder, np.flatnonzero(got != exp)[:8])


def _places(cols):
    """(frame 0's offset, pitch, gap): odd everything; 16-byte aligned everything (vector stores); aligned rows
    with an odd frame stride, gap 37 (frame 1 is then misaligned)"""
    rb = 3 * cols
    p16 = (rb + 15) // 16 * 16
    return [(16 + 3, rb + 5, 7), (16, p16, 32), (16, p16 + 16, 37)]


def _round_trip(ctx, oracle, n, rows, cols, plane0=0, nplanes=8, gcode=False, ct=0, pred=1, packed=True,
                places=None, adaptive=True):
    key, imgs, planes = frames(oracle, "uniform", n, rows, cols, ct, gcode)
    d, pitch, st = buffer(ctx, imgs, fused_pitch(cols, 7), off=16 + 3, gap=9)
    m = n * 3 * nplanes
    kw = dict(nframes=n, frame_stride=st, pitch=pitch, nplanes=nplanes, plane0=plane0, wpr=even(cols),
              predict=bool(pred))
    if packed:
        idx = ctx.empty_i64(m * rows * 2)
        _, (og, bg, fg), (oe, be, fe) = ctx.encode_rgb_frames_packed(d, rows, cols, row_index=idx, **kw)
    else:
        pl = ctx.empty_i64(m, rows, even(cols))
        _, (og, bg), (oe, be) = ctx.encode_rgb_frames(d, rows, cols, planes=pl, **kw)
        fg = fe = None
        idx = ctx.row_index(pl, cols, bool(pred))
    want = _expect(imgs, plane0, nplanes, gcode, ct)
    p00 = _p00(ctx, imgs, plane0, nplanes, gcode, ct) if pred else None
    if adaptive:  # the adaptive EG streams and their index from the oracle's planes, in the call's order
        sel = np.stack([planes[f, 8 * c + plane0:8 * c + plane0 + nplanes] for f in range(n) for c in range(3)])
        pa = ctx.torch.from_numpy(sel.reshape(m, rows, -1).view(np.int64).copy()).to(ctx.dev)
        oa, ba = ctx.encode_planes(pa, cols, bool(pred), A)
        ia = ctx.egad_row_index(pa, cols, bool(pred))
    ctx.sync()
    for lead, opitch, gap in places or _places(cols):
        tag = (n, rows, cols, plane0, nplanes, gcode, ct, pred, packed, lead, opitch, gap)
        _decode_check(ctx, G, og, bg, fg, idx, want, plane0, nplanes, pred, p00, lead, opitch, gap, tag)
        _decode_check(ctx, E, oe, be, fe, None, want, plane0, nplanes, pred, p00, lead, opitch, gap, tag)
        if adaptive:
            _decode_check(ctx, A, oa, ba, None, ia, want, plane0, nplanes, pred, p00, lead, opitch, gap, tag)


# rows 64 and 128: whole column chunks (the Golomb decoder forms the chunk totals itself); 1 and 70: the other route
@pytest.mark.parametrize("cols", [100, 4096])
@pytest.mark.parametrize("rows", [1, 64, 70, 128])
def test_round_trip(ctx, oracle, staged, rows, cols):
    _round_trip(ctx, oracle, 3, rows, cols)


def test_round_trip_slots(ctx, oracle, staged):
    _round_trip(ctx, oracle, 3, 70, 100, packed=False, adaptive=False)


def test_round_trip_plane_range(ctx, oracle, staged):
    _round_trip(ctx, oracle, 3, 70, 100, plane0=2, nplanes=3)


def test_round_trip_gray_code(ctx, oracle, staged, options):
    options(True, 0)
    _round_trip(ctx, oracle, 3, 70, 100, gcode=True)
    _round_trip(ctx, oracle, 3, 64, 4096, gcode=True, places=[(16, 3 * 4096, 16)])
    _round_trip(ctx, oracle, 3, 70, 100, plane0=2, nplanes=3, gcode=True)


@pytest.mark.parametrize("ct", [1, 2])
@pytest.mark.parametrize("gcode", [False, True])
def test_round_trip_colour_transform(ctx, oracle, staged, options, ct, gcode):
    options(gcode, ct)
    _round_trip(ctx, oracle, 3, 70, 100, gcode=gcode, ct=ct)
    _round_trip(ctx, oracle, 3, 64, 4096, gcode=gcode, ct=ct, places=[(16, 3 * 4096 + 16, 37)], adaptive=False)


def test_round_trip_without_prediction(ctx, oracle, staged):
    """predict off: the D buffer holds the planes themselves (no chunk totals)"""
    _round_trip(ctx, oracle, 3, 70, 100, pred=0, adaptive=False)
    _round_trip(ctx, oracle, 3, 70, 100, pred=0, packed=False, adaptive=False, places=[(16, 304, 16)])


def test_single_frame_is_decode_rgb(ctx, oracle, staged):
    """nframes = 1: the stride is not read, the bytes are bic_decode_rgb's"""
    rows, cols = 70, 100
    key, imgs, _ = frames(oracle, "uniform", 1, rows, cols)
    d, pitch, st = buffer(ctx, imgs, fused_pitch(cols))
    idx = ctx.empty_i64(24 * rows * 2)
    _, (og, bg, fg), _ = ctx.encode_rgb_frames_packed(d, rows, cols, nframes=1, pitch=pitch, wpr=2, row_index=idx,
                                                      eg=False)
    p00 = _p00(ctx, imgs, 0, 8, False, 0)
    a = ctx.decode_rgb_frames(G, og, bg, 1, 8, rows, cols, word_off=fg, row_index=idx, p00=p00, frame_stride=0)
    b = ctx.decode_rgb(G, og, bg, 8, rows, cols, word_off=fg, row_index=idx, p00=p00)
    ctx.sync()
    assert np.array_equal(a.cpu().numpy().reshape(rows, cols, 3), imgs[0])
    assert ctx.torch.equal(a.reshape(-1), b.reshape(-1))
