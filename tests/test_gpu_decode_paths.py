"""The device decoders on the structured path inputs of tests/decoder_inputs.py (which lane paths they
reach: tests/decoder_census.py, asserted by tests/test_decoder_census.py without a GPU).

Every comparison is bit-exact against the input planes themselves (or the image / raster bytes made from
them on the host). The first leg decodes the oracle's own streams with the oracle's row indices, so the
device encoder is not involved; the second is the device round trip; the third sends a subset through the
gray and P4 sinks, whose column-apply kernels differ; the last takes more than 16384 rows through the
column scan's second and third rounds."""
import numpy as np
import pytest

import decoder_inputs as di
from pnm_io import plane_to_p4_rows
from pybic import CODER_EG, CODER_EG_ADAPTIVE, CODER_GOLOMB, as_u64

pytestmark = pytest.mark.gpu

G, E, A = CODER_GOLOMB, CODER_EG, CODER_EG_ADAPTIVE
CODERS = {"golomb": G, "eg": E, "egad": A}
NAMES = list(di.PATH_INPUTS)
_IDS = [f"{di.family(n)}:{n}" for n in NAMES]
_ORACLE = {}


def _oracle_streams(oracle, name, pred, coder, P=None):
    """the oracle's streams of an input's planes (or of planes P made from it), once:
    (bits[n], [stream words], index [n, 2 rows] or None)"""
    key = (name, pred, coder, P is None)
    if key not in _ORACLE:
        cols = di.get(oracle, name)[1]
        P = di.get(oracle, name)[0] if P is None else P
        n, rows = P.shape[0], P.shape[1]
        bits, words = np.zeros(n, np.uint64), []
        idx = None if coder == E else np.zeros((n, 2 * rows), np.uint64)
        for k in range(n):
            b, st, _ = oracle.encode_plane(P[k], cols, pred, coder)
            bits[k] = b
            words.append(np.frombuffer(st.tobytes(), np.uint64))  # the stream's bytes are the slot's
            if coder == G:
                idx[k] = oracle.row_index(P[k], cols, pred)
            elif coder == A:
                idx[k] = oracle.egad_row_index(P[k], cols, pred)
        _ORACLE[key] = (bits, words, idx)
    return _ORACLE[key]


def _slots(ctx, words, rows, cols, coder):
    S = np.zeros((len(words), max(ctx.slot_words(rows, cols, coder), max(len(w) for w in words))), np.uint64)
    for k, w in enumerate(words):
        S[k, :len(w)] = w
    return ctx.to_dev(S)


def _packed(ctx, words):
    """plane k's words at word_off[k], odd gaps between the planes (a plane's capacity is word_off[k + 1] -
    word_off[k]) and a lead: -> (streams, word_off)"""
    off, parts, at = [], [], 3
    parts.append(np.full(3, 0xA5A5A5A5A5A5A5A5, np.uint64))
    for k, w in enumerate(words):
        off.append(at)
        parts.append(w)
        gap = np.full(k % 3, 0xA5A5A5A5A5A5A5A5, np.uint64)
        parts.append(gap)
        at += len(w) + len(gap)
    off.append(at)
    return ctx.to_dev(np.concatenate(parts)), ctx.to_dev(np.array(off, np.uint64))


def _plane_words(out, off):
    """a packed encode's words per plane"""
    w, f = as_u64(out), [int(x) for x in as_u64(off)]
    return [w[f[k]:f[k + 1]] for k in range(len(f) - 1)]


def _p00(ctx, P):
    return ctx.torch.tensor([int(P[k, 0, 0] >> np.uint64(63)) for k in range(P.shape[0])], dtype=ctx.torch.uint8,
                            device=ctx.dev)


def _check_planes(back, P, what):
    """the decoded planes [n, rows, wpr] equal the input bit for bit; pad words 0"""
    got = as_u64(back)
    used = P.shape[2]
    bad = np.argwhere(got[:, :, :used] != P)
    assert bad.size == 0, (what, "first differing (plane, row, word)", bad[:4].tolist(), len(bad))
    assert not got[:, :, used:].any(), (what, "pad words")


# 1. oracle streams in, planes out: slots and packed, every coder
@pytest.mark.parametrize("pred", [0, 1])
@pytest.mark.parametrize("name", NAMES, ids=_IDS)
def test_oracle_streams(ctx, oracle, name, pred):
    P, cols = di.get(oracle, name)
    n, rows, used = P.shape
    p00 = _p00(ctx, P) if pred else None
    for cname, coder in CODERS.items():
        bits, words, idx = _oracle_streams(oracle, name, pred, coder)
        if coder == G:
            for k in range(n):
                rc, back = oracle.decode_plane_golomb(words[k].view(np.uint8), int(bits[k]), rows, cols, pred,
                                                      int(P[k, 0, 0] >> np.uint64(63)))
                assert rc == 0 and np.array_equal(back, P[k]), (name, "oracle decoder", k)
        dbits = ctx.to_dev(bits)
        didx = None if idx is None else ctx.to_dev(idx.reshape(-1))
        back = ctx.decode_planes(coder, _slots(ctx, words, rows, cols, coder), dbits, n, rows, cols, pred,
                                 row_index=didx, p00=p00)
        ctx.sync()
        _check_planes(back, P, (name, pred, cname, "slots"))
        streams, off = _packed(ctx, words)
        out = ctx.torch.full((n, rows, used + 1), -1, dtype=ctx.torch.int64, device=ctx.dev)
        back = ctx.decode_planes(coder, streams, dbits, n, rows, cols, pred, word_off=off, row_index=didx, p00=p00,
                                 out=out, wpr=used + 1)
        ctx.sync()
        _check_planes(back, P, (name, pred, cname, "packed"))


# 2. the device round trip: encode (staged and automatic encoder) with the row index, then decode
@pytest.mark.parametrize("enc", ["staged", "auto"])
@pytest.mark.parametrize("pred", [0, 1])
@pytest.mark.parametrize("name", NAMES, ids=_IDS)
def test_device_round_trip(ctx, oracle, name, pred, enc):
    P, cols = di.get(oracle, name)
    n, rows, used = P.shape
    p00 = _p00(ctx, P) if pred else None
    d = ctx.to_dev(np.array(P))
    ctx.set_encoder(enc)
    try:
        idx = ctx.empty_i64(n * rows * 2)
        (og, bg, fg), (oe, be, fe) = ctx.encode_planes_packed(d, cols, pred, golomb=True, eg=True, row_index=idx)
        oa, ba = ctx.encode_planes(d, cols, pred, A)
        ia = ctx.egad_row_index(d, cols, pred)
        back_g = ctx.decode_planes(G, og, bg, n, rows, cols, pred, word_off=fg, row_index=idx, p00=p00)
        back_e = ctx.decode_planes(E, oe, be, n, rows, cols, pred, word_off=fe, p00=p00)
        back_a = ctx.decode_planes(A, oa, ba, n, rows, cols, pred, row_index=ia, p00=p00)
        ctx.sync()
    finally:
        ctx.set_encoder("auto")
    assert np.array_equal(as_u64(idx).reshape(n, 2 * rows), _oracle_streams(oracle, name, pred, G)[2]), name
    assert np.array_equal(as_u64(ia).reshape(n, 2 * rows), _oracle_streams(oracle, name, pred, A)[2]), name
    # (the streams themselves are the oracle's: bit counts and words)
    for cname, bits, words in (("golomb", bg, _plane_words(og, fg)), ("eg", be, _plane_words(oe, fe)),
                               ("egad", ba, [as_u64(oa[k]) for k in range(n)])):
        ebits, ewords, _ = _oracle_streams(oracle, name, pred, CODERS[cname])
        assert np.array_equal(as_u64(bits), ebits), (name, pred, enc, cname, "bit counts")
        for k in range(n):
            assert np.array_equal(words[k][:len(ewords[k])], ewords[k]), (name, pred, enc, cname, "stream", k)
    _check_planes(back_g, P, (name, pred, enc, "golomb"))
    _check_planes(back_e, P, (name, pred, enc, "eg"))
    _check_planes(back_a, P, (name, pred, enc, "egad"))


# 3. the other two sinks (k_col_apply_gray, k_col_apply_pbm): one input per family, rows a multiple of the
#    column chunk of 64 (Golomb with prediction then forms the chunk totals in the row kernel) and not
#    (k_col_chunks)
SINK_NAMES = [
    "dense_then_sparse-128x2048", "sparse_then_dense-64x1024", "density_step_col-33x700", "density_ramp-192x512",
    "gaps-45x333", "alternating-70x255", "first_row_run-known", "all_zero-64x1000", "all_one-7x1000",
    "single_one-c63", "mixed_wave-40x1024", "widths-65", "widths-1000", "tail_across_block-96x260",
    "burst_to_word_end-40x520", "ones_tail_k1-96x456", "eg_first-9x200",
]
_P8 = {}


def _planes8(oracle, name):
    """8 structured planes out of the input's: plane b is the input's plane b % n, its rows rotated by b // n"""
    if name not in _P8:
        P, cols = di.get(oracle, name)
        n = P.shape[0]
        P8 = np.stack([np.roll(P[b % n], b // n, axis=0) for b in range(8)])
        P8.setflags(write=False)
        _P8[name] = P8
    return _P8[name]


def test_sink_subset_covers_the_families():
    assert {di.family(n) for n in SINK_NAMES} == {di.family(n) for n in NAMES}


@pytest.mark.parametrize("cname", list(CODERS))
@pytest.mark.parametrize("pred", [0, 1])
@pytest.mark.parametrize("name", SINK_NAMES, ids=[f"{di.family(n)}:{n}" for n in SINK_NAMES])
def test_other_sinks(ctx, oracle, name, pred, cname):
    coder = CODERS[cname]
    cols = di.get(oracle, name)[1]
    P8 = _planes8(oracle, name)
    n, rows, used = P8.shape
    bits, words, idx = _oracle_streams(oracle, name, pred, coder, P8)
    p00 = _p00(ctx, P8) if pred else None
    dbits = ctx.to_dev(bits)
    didx = None if idx is None else ctx.to_dev(idx.reshape(-1))
    slots = _slots(ctx, words, rows, cols, coder)
    img = oracle.planes_to_gray(P8, cols).astype(np.uint8)
    gray = ctx.decode_gray(coder, slots, dbits, 8, rows, cols, pred, row_index=didx, p00=p00)
    # the same planes as 8 P4 frames, 3 bytes into a buffer and fb + 5 bytes apart
    nb = (cols + 7) // 8
    fb, lead = rows * nb, 3
    stride = fb + 5
    total = lead + 7 * stride + fb + 40
    out = ctx.torch.full((total,), 0xA5, dtype=ctx.torch.uint8, device=ctx.dev)
    streams, off = _packed(ctx, words)
    ctx.decode_pbm(coder, streams, dbits, 8, rows, cols, pred, word_off=off, row_index=didx, p00=p00, out=out[lead:],
                   frame_stride=stride)
    ctx.sync()
    got = gray.cpu().numpy()
    bad = np.argwhere(got != img)
    assert bad.size == 0, (name, pred, cname, "gray: first differing (row, col)", bad[:4].tolist(), len(bad))
    want = np.full(total, 0xA5, np.uint8)
    for f in range(8):
        want[lead + f * stride:lead + f * stride + fb] = plane_to_p4_rows(P8[f], cols).reshape(-1)
    got = out.cpu().numpy()
    assert np.array_equal(got, want), (name, pred, cname, "P4: first differing bytes", np.flatnonzero(got != want)[:8])


# 4. more than 16384 rows: k_col_scan_par's carry across its rounds of 256 chunks (257, 257 and 516 chunks)
@pytest.mark.parametrize("name", list(di.TALL_INPUTS))
def test_tall(ctx, oracle, name):
    P, cols = di.get(oracle, name)
    n, rows, used = P.shape
    p00 = _p00(ctx, P)
    for cname, coder in CODERS.items():
        bits, words, idx = _oracle_streams(oracle, name, 1, coder)
        didx = None if idx is None else ctx.to_dev(idx.reshape(-1))
        streams, off = _packed(ctx, words)
        back = ctx.decode_planes(coder, streams, ctx.to_dev(bits), n, rows, cols, True, word_off=off, row_index=didx,
                                 p00=p00)
        ctx.sync()
        _check_planes(back, P, (name, cname))


@pytest.mark.parametrize("cname", list(CODERS))
def test_tall_gray(ctx, oracle, cname):
    name, coder = "tall-16448x65", CODERS[cname]
    P, cols = di.get(oracle, name)
    n, rows, used = P.shape
    bits, words, idx = _oracle_streams(oracle, name, 1, coder)
    didx = None if idx is None else ctx.to_dev(idx.reshape(-1))
    gray = ctx.decode_gray(coder, _slots(ctx, words, rows, cols, coder), ctx.to_dev(bits), n, rows, cols, True,
                           row_index=didx, p00=_p00(ctx, P))
    ctx.sync()
    assert np.array_equal(gray.cpu().numpy(), oracle.planes_to_gray(P, cols).astype(np.uint8))
