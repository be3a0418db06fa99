"""bic_dict_encode (csrc/bic_dict.hip: the growing-dictionary tile loop of compress2_test.cpp:79-129 and
compress3_test.cpp:87-149) against the restatement tests/dict_ref.py, itself pinned to the drivers' output by
tests/test_dict_ref.py. Bit-exact: every per-tile array, the dictionary, the totals and, variant 3, both Golomb
streams against the oracle's coding of the restatement's samples. atom_step = 1 is also compared with the
drivers' records (tests/golden/dict.npz)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import dict_cases
import dict_ref
import dropin_expect
import pybic
from pybic import as_u64, stream_bytes

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(dict_cases.GOLDEN, "dict.npz"), allow_pickle=False)
GLYPH = next(n for n, c in enumerate(dict_cases.CASES) if c["name"] == "glyph")
RUNS = [(n, v, step) for n, c in enumerate(dict_cases.CASES) for v in c["variants"] for step in (1, c["W"])]


@functools.lru_cache(maxsize=None)
def table(W):
    t = np.array([dropin_expect.enumL(W * W, w) for w in range(W * W + 1)], np.float64)
    assert np.array_equal(t, GOLD[f"enuml_W{W}"])  # the table the drivers' build used
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def expected(n, v, step):
    """the restatement's result and the input, computed once and shared (read-only)"""
    case = dict_cases.CASES[n]
    plane, rows, cols = dict_cases.make_input(case)
    return plane, cols, dict_ref.dict_encode(plane, cols, v, case["W"], case["T"], step, table(case["W"]))


def compare(ctx, oracle, got, exp, v):
    ctx.sync()
    nt = len(exp["bestk"])
    for k in ("bestk", "bestd", "dsize", "weights"):
        assert np.array_equal(got[k].cpu().numpy().view(np.uint32), exp[k]), k
    assert got["modes"].cpu().numpy().tobytes().decode() == exp["modes"]
    assert np.array_equal(got["joined"].cpu().numpy(), exp["joined"])
    st = [int(x) for x in as_u64(got["stats"])]
    bm = bn = 0
    if v == 3:
        bm, sm, _, _ = oracle.golomb_samples(exp["samples_match"])
        bn, sn, _, _ = oracle.golomb_samples(exp["samples_nomatch"])
    assert st == [exp["matches"], bm, bn, exp["L"], exp["nD"]]
    assert np.array_equal(got["dict_tiles"].cpu().numpy().view(np.uint32)[:exp["nD"]], exp["dict_tiles"])
    if v == 3 and got["stream_match"] is not None:
        assert stream_bytes(got["stream_match"], bm) == sm.tobytes()
        assert stream_bytes(got["stream_nomatch"], bn) == sn.tobytes()
    assert nt == got["bestk"].numel()


@pytest.mark.parametrize("n,v,step", RUNS)
def test_dict_encode(ctx, oracle, n, v, step):
    case = dict_cases.CASES[n]
    plane, cols, exp = expected(n, v, step)
    got = ctx.dict_encode(ctx.to_dev(plane), cols, v, case["W"], case["T"], step, table(case["W"]))
    compare(ctx, oracle, got, exp, v)
    if step == 1:  # what the drivers printed
        for k in ("bestk", "bestd", "dsize"):
            assert np.array_equal(got[k].cpu().numpy().view(np.uint32), GOLD[f"c{n}_v{v}_{k}"]), k
        x = got["modes"].cpu().numpy() == ord("x")
        assert np.array_equal(x, GOLD[f"c{n}_v{v}_use_match"] != 0)
        assert np.array_equal(got["joined"].cpu().numpy()[1:], GOLD[f"c{n}_v{v}_add"][1:])


@pytest.mark.parametrize("block", [1, 7, 64, 0])
@pytest.mark.parametrize("v,step", [(2, 1), (2, 16), (3, 1), (3, 16)])
def test_dict_block(ctx, oracle, v, step, block):
    """the number of tiles resolved per block does not change the result"""
    case = dict_cases.CASES[GLYPH]
    plane, cols, exp = expected(GLYPH, v, step)
    ctx.set_dict_block(block)
    try:
        got = ctx.dict_encode(ctx.to_dev(plane), cols, v, case["W"], case["T"], step, table(case["W"]))
        compare(ctx, oracle, got, exp, v)
    finally:
        ctx.set_dict_block(0)


def test_dict_repeat_and_padded_pitch(ctx, oracle):
    """repeated calls reuse the arena; a plane with a pitch above ceil(cols/64) reads the same windows (the
    flat indexing runs over the used words of a row, not the pitch)"""
    n = next(i for i, c in enumerate(dict_cases.CASES) if c["name"] == "w33")
    case = dict_cases.CASES[n]
    plane, cols, exp = expected(n, 3, 1)
    wide = np.full((plane.shape[0], plane.shape[1] + 2), 0xFFFFFFFFFFFFFFFF, np.uint64)
    wide[:, :plane.shape[1]] = plane
    for _ in range(2):
        got = ctx.dict_encode(ctx.to_dev(wide), cols, 3, case["W"], case["T"], 1, table(case["W"]))
        compare(ctx, oracle, got, exp, 3)


def test_dict_null_outputs_and_lengths_only(ctx, oracle):
    """every per-tile output and both streams null (cap_words = 0): the totals alone, and no BIC_ENOSPC"""
    case = dict_cases.CASES[GLYPH]
    plane, cols, exp = expected(GLYPH, 3, 16)
    d = ctx.to_dev(plane)
    stats = ctx.empty_i64(5)
    e = table(case["W"])
    ctx._bind_stream()
    rc = ctx.lib.bic_dict_encode(ctx.h, 3, C.c_void_p(d.data_ptr()), plane.shape[0], cols, plane.shape[1], case["W"],
                                 case["T"], 16, e.ctypes.data_as(C.c_void_p), None, None, None, None, None, None, None,
                                 None, None, 0, C.c_void_p(stats.data_ptr()))
    assert rc == pybic.BIC_OK
    ctx.sync()  # (raises on a deferred BIC_ENOSPC)
    bm = oracle.golomb_samples(exp["samples_match"], False)[0]
    bn = oracle.golomb_samples(exp["samples_nomatch"], False)[0]
    assert [int(x) for x in as_u64(stats)] == [exp["matches"], bm, bn, exp["L"], exp["nD"]]


def test_dict_stream_overflow(ctx, oracle):
    """cap_words one word too small for golomb_nomatch's stream: BIC_ENOSPC from bic_sync, nothing past it"""
    case = dict_cases.CASES[GLYPH]
    plane, cols, exp = expected(GLYPH, 3, 1)
    bm = oracle.golomb_samples(exp["samples_match"], False)[0]
    bn = oracle.golomb_samples(exp["samples_nomatch"], False)[0]
    need = (max(bm, bn) + 63) // 64
    assert need >= 2
    cap, canary = need - 1, 0x5A5A5A5A5A5A5A5A
    t = ctx.torch
    d = ctx.to_dev(plane)
    bufs = [t.full((cap + 8,), canary, dtype=t.int64, device=ctx.dev) for _ in range(2)]
    stats = ctx.empty_i64(5)
    e = table(case["W"])
    ctx._bind_stream()
    rc = ctx.lib.bic_dict_encode(ctx.h, 3, C.c_void_p(d.data_ptr()), plane.shape[0], cols, plane.shape[1], case["W"],
                                 case["T"], 1, e.ctypes.data_as(C.c_void_p), None, None, None, None, None, None, None,
                                 C.c_void_p(bufs[0].data_ptr()), C.c_void_p(bufs[1].data_ptr()), cap,
                                 C.c_void_p(stats.data_ptr()))
    assert rc == pybic.BIC_OK
    with pytest.raises(pybic.BicError) as err:
        ctx.sync()
    assert err.value.code == pybic.BIC_ENOSPC
    for b in bufs:
        assert (as_u64(b)[cap:] == np.uint64(canary)).all()
    # the context works again afterwards, with room
    got = ctx.dict_encode(d, cols, 3, case["W"], case["T"], 1, e)
    compare(ctx, oracle, got, exp, 3)
