"""Kernel timing API (include/bic.h bic_prof_enable / bic_prof_only / bic_prof_collect): what
bench.py's roofline timing relies on."""
import pytest

pytestmark = pytest.mark.gpu


def test_prof_only_brackets_named_launches(ctx):
    t = ctx.torch
    gray = t.randint(0, 256, (64, 200), dtype=t.uint8, device=ctx.dev)
    ctx.sync()
    ctx.prof_collect()  # drop anything earlier tests left
    ctx.prof_enable(True)
    try:
        ctx.prof_only(None)
        ctx.bitplanes_u8(gray, nplanes=8)
        ctx.bitplanes_u8(gray, nplanes=8)
        allp = ctx.prof_collect()
        assert allp["bitplanes_u8"][0] == 2 and allp["bitplanes_u8"][1] >= 0
        ctx.prof_only("no_such_kernel")
        ctx.bitplanes_u8(gray, nplanes=8)
        assert ctx.prof_collect() == {}
        ctx.prof_only("bitplanes_u8")
        ctx.bitplanes_u8(gray, nplanes=8)
        assert ctx.prof_collect()["bitplanes_u8"][0] == 1
    finally:
        ctx.prof_only(None)
        ctx.prof_enable(False)


@pytest.mark.parametrize("encoder", ["auto", "staged", "single-kernel", "two-pass"])
def test_prof_rows_timing_every_encoder(ctx, encoder):
    """the emission's kernel timing (bic_ctx.h timed_rows) on every row encoder: the single and
    two-pass encoders have no separate main kernel, and their end event must still be recorded --
    an event left unrecorded fails the elapsed-time query, and that HIP error used to stay pending and
    fail the NEXT call (bench.py --gpus 2 --shard planes: bic error 3)"""
    t = ctx.torch
    g = t.Generator(device=ctx.dev)
    g.manual_seed(7)
    planes = t.randint(-2**62, 2**62, (2, 96, 64), dtype=t.int64, device=ctx.dev, generator=g)
    ctx.sync()
    ctx.prof_collect()
    ref, ref_bits = ctx.encode_planes(planes, 4096)
    ctx.sync()
    ref, ref_bits = ref.clone(), ref_bits.clone()
    ctx.set_encoder(encoder)
    ctx.prof_enable(True)
    try:
        ctx.prof_only(None)
        out, bits = ctx.encode_planes(planes, 4096)
        got = ctx.prof_collect()
        rows = [k for k in got if k.startswith("encode_rows")]
        assert rows and all(got[k][1] >= 0 for k in rows), got
        out2, bits2 = ctx.encode_planes(planes, 4096)  # the next call must not inherit an error
        ctx.sync()
        assert t.equal(bits, ref_bits) and t.equal(bits2, ref_bits)
        for p in range(2):
            nw = (int(ref_bits[p]) + 63) // 64
            assert t.equal(out[p, :nw], ref[p, :nw]) and t.equal(out2[p, :nw], ref[p, :nw])
    finally:
        ctx.prof_only(None)
        ctx.prof_enable(False)
        ctx.set_encoder("auto")


def _planes2(predict):
    return lambda ctx, planes, gray: ctx.encode_planes2(planes, 4096, predict=predict)


def _packed_index(ctx, planes, gray):
    return ctx.encode_planes_packed(planes, 4096, golomb=True, eg=True, row_index=ctx.empty_i64(2 * 70 * 2))


def _gray(store_planes):
    return lambda ctx, planes, gray: ctx.encode_gray(gray, store_planes=store_planes)


_STAGED = [("encode_finish", 1), ("encode_prefix", 1)]
_LOOKBACK = [("encode_finish", 1)]
_ROWS_GE = [("encode_rows_golomb_eg", 1), ("encode_rows_golomb_eg_stage", 1)]
_GRAY = [("bitplanes_count", 1)] + _STAGED
# (path, encoder, BIC_OPT_EG_SOURCE, the call, bic_prof_collect's lines: name and launch count, in its
# order) -- the lists are those of a run of the commit before the host side of the row encoders was
# reorganised into one driver (bic_capi_rows.cpp run_fused), on these inputs
_RECORD_PATHS = [
    ("planes2-staged-predict", "staged", 1, _planes2(True), _STAGED + _ROWS_GE),
    ("planes2-staged-nopredict", "staged", 1, _planes2(False), _STAGED + _ROWS_GE),
    ("planes2-single-kernel", "single-kernel", 1, _planes2(True), _LOOKBACK + _ROWS_GE),
    ("planes2-two-pass", "two-pass", 1, _planes2(True), _LOOKBACK + _ROWS_GE),
    ("packed-index-staged", "staged", 1, _packed_index, _STAGED + _ROWS_GE),
    ("packed-index-single-kernel", "single-kernel", 1, _packed_index,
     _LOOKBACK + _ROWS_GE + [("pack", 2), ("row_index", 1)]),
    ("gray-eg-source", "staged", 1, _gray(False),
     _GRAY + [("encode_rows_golomb_egsrc", 1), ("encode_rows_golomb_egsrc_stage", 1)]),
    ("gray-resid", "staged", 0, _gray(False), _GRAY + _ROWS_GE),
    ("gray-planes", "staged", 1, _gray(True), _GRAY + _ROWS_GE),
    ("row-index", "auto", 1, lambda ctx, planes, gray: ctx.row_index(planes, 4096), [("row_index", 1)]),
]


@pytest.fixture(scope="module")
def record_inputs(ctx):
    t = ctx.torch
    g = t.Generator(device=ctx.dev)
    g.manual_seed(11)
    planes = t.randint(-2**62, 2**62, (2, 70, 64), dtype=t.int64, device=ctx.dev, generator=g)
    gray = t.randint(0, 256, (70, 4096), dtype=t.uint8, device=ctx.dev, generator=g)
    ctx.sync()
    return planes, gray


@pytest.mark.parametrize("path", _RECORD_PATHS, ids=[p[0] for p in _RECORD_PATHS])
def test_record_names_per_path(ctx, record_inputs, path):
    """what one call of each encode path records with profiling on and no bic_prof_only: the stages
    the driver runs for it (70 x 4096: 2 planes, or the 8 of a gray image), pinned against the lists
    above"""
    _, encoder, eg_source, call, expected = path
    planes, gray = record_inputs
    ctx.prof_collect()
    ctx.set_encoder(encoder)
    ctx.set_eg_source(eg_source)
    ctx.prof_enable(True)
    try:
        ctx.prof_only(None)
        call(ctx, planes, gray)
        got = ctx.prof_collect()
        assert [(k, v[0]) for k, v in got.items()] == expected
        assert all(v[1] >= 0 for v in got.values()), got
    finally:
        ctx.prof_only(None)
        ctx.prof_enable(False)
        ctx.set_eg_source(1)
        ctx.set_encoder("auto")
