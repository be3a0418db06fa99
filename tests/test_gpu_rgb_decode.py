"""bic_decode_rgb: streams -> interleaved R G B samples in one call, and bic_planes_to_rgb. The streams, bit
counts and row indices decoded here are the oracle's (bo_encode_plane / bo_row_index on the planes of
img[:, :, c]), never the device encoder's; every result is compared byte for byte with the image masked to
the decoded planes' bits, and the bytes around every row must stay as they were."""
import ctypes as C

import numpy as np
import pytest

import pybic
from pybic import CODER_EG, CODER_GOLOMB, as_u64

pytestmark = pytest.mark.gpu

G, E = CODER_GOLOMB, CODER_EG
GUARD = 0x5A
_IMG, _ENC = {}, {}


@pytest.fixture
def gray_code(ctx):
    ctx.set_gray_code(True)
    yield
    ctx.set_gray_code(False)


def _gray(v):
    return v ^ (v >> 1)


def _img(oracle, rows, cols):
    """a seeded image whose channels all differ: R uniform bytes, G a ramp with noise (all-zero high planes,
    long runs: rows of k = 0, k = 1 and mixed k), B another ramp"""
    key = (rows, cols)
    if key not in _IMG:
        seed = 0xDEC0 + 131 * rows + cols
        n = oracle.gen_bytes(seed, 2 * rows * cols).reshape(2, rows, cols)
        i, j = np.mgrid[0:rows, 0:cols]
        a = np.stack([n[0], (3 * i + j // 7 + n[1] % 5) % 200, (i // 3 + 5 * j // 13) % 97], axis=2).astype(np.uint8)
        a.setflags(write=False)
        _IMG[key] = a
    return _IMG[key]


def _oracle_enc(oracle, rows, cols, plane0, nplanes, pred, coder, gc=False):
    """the oracle's streams of the 3 * nplanes planes in bic_encode_rgb's order, once:
    (bits [n3], [stream words], row index [n3, 2 rows] (Golomb), p00 [n3], the planes)"""
    key = (rows, cols, plane0, nplanes, pred, coder, gc)
    if key not in _ENC:
        img = _img(oracle, rows, cols)
        v = _gray(img) if gc else img
        P = np.concatenate([oracle.bitplanes(np.ascontiguousarray(v[:, :, c]), 8)[plane0:plane0 + nplanes]
                            for c in range(3)])
        n3 = 3 * nplanes
        bits, words = np.zeros(n3, np.uint64), []
        idx = np.zeros((n3, 2 * rows), np.uint64) if coder == G else None
        for p in range(n3):
            b, st, _ = oracle.encode_plane(P[p], cols, pred, coder)
            bits[p] = b
            words.append(np.frombuffer(st.tobytes(), np.uint64))
            if coder == G:
                idx[p] = oracle.row_index(P[p], cols, pred)
        p00 = np.array([(int(v[0, 0, c]) >> (plane0 + k)) & 1 for c in range(3) for k in range(nplanes)], np.uint8)
        _ENC[key] = (bits, words, idx, p00, P)
    return _ENC[key]


def _dev_streams(ctx, enc, rows, cols, coder, packed):
    """-> kwargs of Context.decode_rgb: slots, or packed words with odd gaps between the planes and a lead"""
    bits, words, idx, p00, _ = enc
    kw = dict(plane_bits=ctx.to_dev(bits), row_index=None if idx is None else ctx.to_dev(idx.reshape(-1)),
              p00=ctx.torch.from_numpy(p00.copy()).to(ctx.dev))
    if not packed:
        S = np.zeros((len(words), max(ctx.slot_words(rows, cols, coder), max(len(w) for w in words))), np.uint64)
        for k, w in enumerate(words):
            S[k, :len(w)] = w
        kw["streams"] = ctx.to_dev(S)
        return kw
    off, parts, at = [], [np.full(3, 0xA5A5A5A5A5A5A5A5, np.uint64)], 3
    for k, w in enumerate(words):
        off.append(at)
        gap = np.full(k % 3, 0xA5A5A5A5A5A5A5A5, np.uint64)
        parts += [w, gap]
        at += len(w) + len(gap)
    off.append(at)
    kw["streams"] = ctx.to_dev(np.concatenate(parts))
    kw["word_off"] = ctx.to_dev(np.array(off, np.uint64))
    return kw


def _expect(img, plane0, nplanes, gc=False):
    """the samples the decoded planes give: the covered bits (gc: of the samples whose Gray code, cut to the
    covered bits, the planes hold)"""
    m = np.uint8(((1 << nplanes) - 1) << plane0)
    if not gc:
        return img & m
    x = _gray(img) & m
    x = x ^ (x >> 1)
    x = x ^ (x >> 2)
    x = x ^ (x >> 4)
    return x & m


def _dests(cols):
    """(offset into the allocation, pitch): 16-byte aligned rows (the 16-byte stores), misaligned pointers,
    the tight pitch (no multiple of 16 at these widths) and padded odd ones"""
    p16 = (3 * cols + 15) // 16 * 16 + 16
    assert (3 * cols) % 16 != 0
    return [(0, p16), (0, 3 * cols), (5, 3 * cols), (1, 3 * cols + 7), (16, p16 + 16), (13, p16)]


def _decode_check(ctx, img, dkw, coder, pred, plane0, nplanes, off, pitch, want):
    rows, cols, _ = img.shape
    buf = ctx.torch.full((off + rows * pitch + 64,), GUARD, dtype=ctx.torch.uint8, device=ctx.dev)
    kw = dict(dkw)
    if not pred:
        kw.pop("p00")
    ctx.decode_rgb(coder, kw.pop("streams"), kw.pop("plane_bits"), nplanes, rows, cols, bool(pred), plane0=plane0,
                   out=buf[off:], pitch=pitch, **kw)
    ctx.sync()
    got = buf.cpu().numpy()
    assert (got[:off] == GUARD).all(), "bytes before the image"
    body = got[off:off + rows * pitch].reshape(rows, pitch)
    bad = np.argwhere(body[:, :3 * cols] != want.reshape(rows, 3 * cols))
    assert bad.size == 0, ("first differing (row, byte)", bad[:4].tolist(), len(bad), off, pitch)
    assert (body[:, 3 * cols:] == GUARD).all(), ("bytes past a row's 3 * cols", off, pitch)
    assert (got[off + rows * pitch:] == GUARD).all(), "bytes after the image"


# 1. the oracle's streams -> the image, byte for byte. rows: one more than a column chunk of 64 + 3 (two
#    chunks, the second partial), a whole chunk (the Golomb row kernel forms the chunk totals itself), a few;
#    cols: 130 (9 segments, the last of 2 pixels; three words, the last of 2 bits) and 4100 (65 words)
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("pred", [1, 0])
@pytest.mark.parametrize("coder", [G, E])
@pytest.mark.parametrize("rows,cols", [(67, 130), (64, 130), (5, 130), (67, 4100)])
def test_oracle_streams_to_rgb(ctx, oracle, rows, cols, coder, pred, packed):
    img = _img(oracle, rows, cols)
    dkw = _dev_streams(ctx, _oracle_enc(oracle, rows, cols, 0, 8, pred, coder), rows, cols, coder, packed)
    for off, pitch in _dests(cols):
        _decode_check(ctx, img, dkw, coder, pred, 0, 8, off, pitch, img)


# 2. plane ranges: stream c * nplanes + k sets bit plane0 + k of channel c, bits no plane covers are 0
@pytest.mark.parametrize("plane0,nplanes", [(3, 2), (7, 1), (0, 1)])
@pytest.mark.parametrize("coder,pred", [(G, 1), (E, 1), (E, 0)])
def test_plane_ranges(ctx, oracle, plane0, nplanes, coder, pred):
    rows, cols = 67, 130
    img = _img(oracle, rows, cols)
    dkw = _dev_streams(ctx, _oracle_enc(oracle, rows, cols, plane0, nplanes, pred, coder), rows, cols, coder, True)
    want = _expect(img, plane0, nplanes)
    assert want.any()
    for off, pitch in _dests(cols)[:4]:
        _decode_check(ctx, img, dkw, coder, pred, plane0, nplanes, off, pitch, want)


# 3. Gray code on: the streams are those of G(v)'s planes, the samples stored are v's
@pytest.mark.parametrize("plane0,nplanes", [(0, 8), (3, 2)])
@pytest.mark.parametrize("coder,pred", [(G, 1), (E, 0)])
def test_gray_code(ctx, oracle, gray_code, plane0, nplanes, coder, pred):
    for rows, cols in ((67, 130), (5, 4100)):
        img = _img(oracle, rows, cols)
        enc = _oracle_enc(oracle, rows, cols, plane0, nplanes, pred, coder, gc=True)
        dkw = _dev_streams(ctx, enc, rows, cols, coder, False)
        want = _expect(img, plane0, nplanes, gc=True)
        if nplanes == 8:
            assert np.array_equal(want, img)
        for off, pitch in _dests(cols)[:3]:
            _decode_check(ctx, img, dkw, coder, pred, plane0, nplanes, off, pitch, want)


# 4. bic_bitplanes_rgb, then bic_planes_to_rgb, is the identity on the covered bits (the planes between them
#    are the oracle's)
@pytest.mark.parametrize("gc", [False, True])
@pytest.mark.parametrize("rows,cols", [(67, 130), (5, 4100)])
def test_planes_round_trip(ctx, oracle, rows, cols, gc):
    img = _img(oracle, rows, cols)
    ctx.set_gray_code(gc)
    try:
        for plane0, nplanes in ((0, 8), (3, 2), (7, 1), (0, 1)):
            P = _oracle_enc(oracle, rows, cols, plane0, nplanes, 1, E, gc)[4]
            want = _expect(img, plane0, nplanes, gc)
            for off, pitch in _dests(cols)[:4]:
                src = ctx.torch.full((off + rows * pitch + 64,), 0xC3, dtype=ctx.torch.uint8, device=ctx.dev)
                src[off:off + rows * pitch].view(rows, pitch)[:, :3 * cols] = ctx.torch.from_numpy(
                    np.array(img).reshape(rows, 3 * cols)).to(ctx.dev)
                planes = ctx.bitplanes_rgb(src[off:], rows=rows, cols=cols, pitch=pitch, plane0=plane0, nplanes=nplanes)
                buf = ctx.torch.full((off + rows * pitch + 64,), GUARD, dtype=ctx.torch.uint8, device=ctx.dev)
                ctx.planes_to_rgb(planes, cols, plane0=plane0, out=buf[off:], pitch=pitch)
                ctx.sync()
                assert np.array_equal(as_u64(planes), P), (plane0, nplanes, off, pitch)
                got = buf.cpu().numpy()
                body = got[off:off + rows * pitch].reshape(rows, pitch)
                assert np.array_equal(body[:, :3 * cols], want.reshape(rows, 3 * cols)), (plane0, nplanes, off, pitch)
                assert (body[:, 3 * cols:] == GUARD).all() and (got[:off] == GUARD).all()
                assert (got[off + rows * pitch:] == GUARD).all()
    finally:
        ctx.set_gray_code(False)


# 5. the one call == the two calls it replaces (two paths of the library; both == the image)
@pytest.mark.parametrize("coder", [G, E])
def test_one_call_equals_two_calls(ctx, oracle, coder):
    rows, cols = 67, 4100
    img = _img(oracle, rows, cols)
    dkw = _dev_streams(ctx, _oracle_enc(oracle, rows, cols, 0, 8, 1, coder), rows, cols, coder, True)
    planes = ctx.decode_planes(coder, dkw["streams"], dkw["plane_bits"], 24, rows, cols, True, word_off=dkw["word_off"],
                               row_index=dkw["row_index"], p00=dkw["p00"])
    two = ctx.planes_to_rgb(planes, cols)
    one = ctx.decode_rgb(coder, dkw["streams"], dkw["plane_bits"], 8, rows, cols, True, word_off=dkw["word_off"],
                         row_index=dkw["row_index"], p00=dkw["p00"])
    ctx.sync()
    assert ctx.torch.equal(one, two)
    assert np.array_equal(one.cpu().numpy().reshape(rows, cols, 3), img)


# 6. a truncated stream is a malformed input: BIC_EDATA at the sync, and the context decodes the good stream
#    afterwards
@pytest.mark.parametrize("coder", [G, E])
def test_truncated_stream(ctx, oracle, coder):
    rows, cols = 5, 130
    img = _img(oracle, rows, cols)
    dkw = _dev_streams(ctx, _oracle_enc(oracle, rows, cols, 0, 8, 1, coder), rows, cols, coder, True)
    ctx.sync()
    bad = dict(dkw)
    bad["plane_bits"] = dkw["plane_bits"].clone()
    bad["plane_bits"][9] -= 1  # channel 1's plane 1: the stream is one bit longer than claimed
    ctx.decode_rgb(coder, bad["streams"], bad["plane_bits"], 8, rows, cols, True, word_off=bad["word_off"],
                   row_index=bad["row_index"], p00=bad["p00"])
    with pytest.raises(pybic.BicError) as e:
        ctx.sync()
    assert e.value.code == pybic.BIC_EDATA
    _decode_check(ctx, img, dkw, coder, 1, 0, 8, 0, 3 * cols, img)


# 7. refusals, rows = 0, and the profile's name
def test_rejects_and_no_rows(ctx):
    t, b, idx = ctx.empty_i64(24, 64), ctx.empty_i64(24), ctx.empty_i64(24 * 10 * 2)

    def einval(fn):
        with pytest.raises(pybic.BicError) as e:
            fn()
        assert e.value.code == pybic.BIC_EINVAL

    einval(lambda: ctx.decode_rgb(G, t, b, 8, 10, 64))  # Golomb without a row index
    einval(lambda: ctx.decode_rgb(E, t, b, 8, 10, 20000))  # rows wider than 16384 columns
    einval(lambda: ctx.decode_rgb(E, t, b, 8, 10, 64, plane0=1))
    einval(lambda: ctx.decode_rgb(E, t, b, 0, 10, 64))
    einval(lambda: ctx.decode_rgb(E, t, b, 8, 10, 64, pitch=191))
    einval(lambda: ctx.planes_to_rgb(ctx.empty_i64(24, 10, 1), 64, pitch=191))
    einval(lambda: ctx.planes_to_rgb(ctx.empty_i64(24, 10, 1), 64, plane0=1))
    ctx._bind_stream()
    rc = ctx.lib.bic_decode_rgb(ctx.h, G, C.c_void_p(t.data_ptr()), 64, None, C.c_void_p(b.data_ptr()),
                                C.c_void_p(idx.data_ptr()), 0, 8, 10, 64, 1, None, None, 192)  # NULL rgb
    assert rc == pybic.BIC_EINVAL
    buf = ctx.torch.full((768,), GUARD, dtype=ctx.torch.uint8, device=ctx.dev)
    ctx.decode_rgb(E, t, b, 8, 0, 64, out=buf, pitch=192)  # rows = 0: BIC_OK, nothing written
    ctx.sync()
    assert (buf.cpu().numpy() == GUARD).all()


def test_profile_name(ctx, oracle):
    """the whole call is one stage of the profile, decode_rgb: neither bic_decode_planes' nor
    bic_planes_to_rgb's stage runs"""
    rows, cols = 5, 130
    dkw = _dev_streams(ctx, _oracle_enc(oracle, rows, cols, 0, 8, 1, G), rows, cols, G, True)
    ctx.sync()
    ctx.prof_collect()
    ctx.prof_enable(True)
    try:
        ctx.prof_only(None)
        ctx.decode_rgb(G, dkw["streams"], dkw["plane_bits"], 8, rows, cols, True, word_off=dkw["word_off"],
                       row_index=dkw["row_index"], p00=dkw["p00"])
        got = ctx.prof_collect()
    finally:
        ctx.prof_enable(False)
    assert got["decode_rgb"][0] == 1 and "decode" not in got and "planes_to_rgb" not in got, got
