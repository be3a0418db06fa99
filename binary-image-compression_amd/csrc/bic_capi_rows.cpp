// bic_capi_rows.cpp -- the row encoders' entry points (bic_encode_*, bic_row_index, bic_med_residual,
// the adaptive EG coder): one driver for the staged and look-back encoders (run_fused), four sources
// (planes, gray or RGB samples, a batch of gray or RGB frames, P4 rasters) and the multi-pass fallback for rows wider than 16384 columns.
#include "bic_ctx.h"

namespace {

// The staged encoder's second stream and its fork / join events, made on first use; left null
// (one stream) when HIP cannot make them. Work on it is always joined back into ctx->cur.
void set_aux(bic_ctx* ctx, bic::EmitStreams& es) {
  if (ctx->one_stream) return;
  if (!ctx->aux) {
    hipStream_t st = nullptr;
    hipEvent_t a = nullptr, b = nullptr;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return;
    // device-scope fork / join events: they order two streams of this device, and a system-scope
    // release would write back L2 at every fork (emission 167-170 vs 172-174 us, same box). Round 4 had
    // switched them to system scope over a first-encode failure that the scope did not cause: that
    // build's k_emit_k1 lost bits of k = 1 rows with either scope (6 of 6 fresh processes each), and
    // only its LDS image zeroing decided it; these kernels measured 0 of 8 with either.
#ifndef BIC_FORK_EVENT_FLAGS
#define BIC_FORK_EVENT_FLAGS (hipEventDisableTiming | hipEventDisableSystemFence)
#endif
    const unsigned fl = BIC_FORK_EVENT_FLAGS;
    if (hipEventCreateWithFlags(&a, fl) != hipSuccess || hipEventCreateWithFlags(&b, fl) != hipSuccess) {
      if (a) (void)hipEventDestroy(a);
      (void)hipStreamDestroy(st);
      return;
    }
    ctx->aux = st;
    ctx->ev_fork = a;
    ctx->ev_join = b;
  }
  es.aux = ctx->aux;
  es.fork = ctx->ev_fork;
  es.join = ctx->ev_join;
}

// The staged encoder's ~8 dependent launches cost more than the single kernel's look-back waits
// on small batches (C2, one 4096^2 plane: 81 vs 45 us); from kStagedMinRows rows or kStagedMinWords
// plane words (all planes) on it is the faster one (C3: 131,072 rows; one 16384^2 plane, 16,384 rows
// of 256 words: 0.181 vs 0.252 ms). BIC_OPT_STAGED forces it.
constexpr uint64_t kStagedMinRows = 32768, kStagedMinWords = 1ull << 20;
bool staged_pays(const bic_ctx* ctx, const bic::Geom& g) {
  const uint64_t rows = (uint64_t)g.rows * g.nplanes;
  return ctx->force_staged || rows >= kStagedMinRows || rows * g.used >= kStagedMinWords;
}

// nplanes planes of rows x cols pixels, wpr words per row
struct Shape {
  int nplanes;
  size_t rows, cols, wpr;
};
// bps: bytes per sample -- 1 (bic_encode_gray*), or 2 (bic_encode_gray16*: big_endian = 1 the P5 order of
// pnm.cpp:73, 0 the host's uint16_t), or 3 (bic_encode_rgb*: interleaved R G B pixels of one-byte samples,
// pnm.cpp:194-239; the call's planes are then three groups, channel c's planes plane0 .. first)
struct GrayImage {
  const uint8_t* data;
  size_t pitch;
  int bps, big_endian;
};

// Packed output where the encoder cannot write it in place (encoders other than the staged one, the
// multi-pass path): ONE encode of both coders into slots in stream-ordered temporaries, then
// bic_pack_streams' kernel once per coder.
template <typename Encode>
int pack_after(bic_ctx* ctx, int nplanes, const bic::CoderOut& g, const bic::CoderOut& e, Encode&& encode) {
  bic::CoderOut tg{nullptr, g.slot, g.bits, nullptr}, te{nullptr, e.slot, e.bits, nullptr};
  if (g.out) BIC_HIP(hipMallocAsync(reinterpret_cast<void**>(&tg.out), (size_t)nplanes * g.slot * 8, ctx->cur));
  if (e.out && hipMallocAsync(reinterpret_cast<void**>(&te.out), (size_t)nplanes * e.slot * 8, ctx->cur) != hipSuccess) {
    if (tg.out) (void)hipFreeAsync(tg.out, ctx->cur);
    return BIC_EDEVICE;
  }
  const int rc = encode(tg, te);
  if (rc == BIC_OK && tg.out)
    timed(ctx, "pack", [&] { bic::launch_pack(ctx->cur, tg.out, nplanes, g.slot, g.bits, g.out, g.off); });
  if (rc == BIC_OK && te.out)
    timed(ctx, "pack", [&] { bic::launch_pack(ctx->cur, te.out, nplanes, e.slot, e.bits, e.out, e.off); });
  if (tg.out) (void)hipFreeAsync(tg.out, ctx->cur);
  if (te.out) (void)hipFreeAsync(te.out, ctx->cur);
  BIC_HIP(hipGetLastError());
  return rc;
}

bool outs_ok(const bic::CoderOut& g, const bic::CoderOut& e) {
  return (g.out || e.out) && (!g.out || (g.bits && g.slot)) && (!e.out || (e.bits && e.slot));
}

// One call of the row encoders (bic_fused*.hip) on ctx->cur: the scratch arena, then clear -> count
// pass -> prefix -> rows -> finish. c comes as {g, planes, predict, mode, rq}.
// count: the caller's count pass (bic_encode_gray*'s bitplane kernel, rq.counted), given the arena;
// without one the staged prefix counts for itself. prefix_only (bic_row_index): the staged prefix
// alone, recorded as "row_index". count_name: the count pass's profile name.
template <typename Count>
int run_fused(bic_ctx* ctx, bic::FusedCall& c, Count&& count, bool prefix_only = false,
              const char* count_name = "bitplanes_count") {
  int rc = ensure_scratch(ctx, bic::fused_scratch_bytes(c.g));
  if (rc) return rc;
  c.ar = bic::carve_fused_arena(ctx->scratch, c.g);
  c.lut = ctx->lut;
  c.flags = ctx->flags;
  const bool staged = c.mode == bic::kEncStaged;
  // (look-back encoders: no memset when the previous call's k_fixup left the counters and records
  // zero: C2 0.036 -> 0.032 ms. A call on another stream without synchronisation would share the arena
  // anyway: calls on one context are ordered by the caller)
  c.rq.zero_ready = !staged && !ctx->captured && ctx->scratch_zero_prev >= c.ar.zero_bytes;
  if (!staged) bic::launch_lookback_clear(ctx->cur, c);
  if (c.rq.counted) timed(ctx, count_name, [&] { count(c.ar); });
  // staged encoder: per-row counts, scans and Golomb lengths (every row's offsets known up front)
  if (staged)
    timed(ctx, prefix_only ? "row_index" : "encode_prefix",
          [&] { bic::launch_staged_prefix(ctx->cur, c, c.rq.g.out || c.rq.index); });
  if (!prefix_only) {
    // the row kernel alone is timed under the encoder's name (bench.py's roofline kernel)
    bic::EmitStreams es;
    if (staged) set_aux(ctx, es);
    const char* name = c.rq.eg_src ? "encode_rows_golomb_egsrc"
                       : c.rq.g.out ? (c.rq.e.out ? "encode_rows_golomb_eg" : "encode_rows_golomb") : "encode_rows_eg";
    timed_rows(ctx, es, name, [&] {
      if (staged) bic::launch_staged_emit(ctx->cur, c, es);
      else bic::launch_lookback_rows(ctx->cur, c);
    });
    timed(ctx, "encode_finish", [&] { bic::launch_fused_finish(ctx->cur, c); });
  }
  BIC_HIP(hipGetLastError());
  if (!staged && !ctx->captured) ctx->scratch_zero = c.ar.zero_bytes;  // (k_fixup cleared them)
  return BIC_OK;
}

int encode_planes_impl(bic_ctx* ctx, const uint64_t* planes, const Shape& sh, int predict, const bic::CoderOut& og,
                       const bic::CoderOut& oe, uint64_t* row_index = nullptr) {
  const int nplanes = sh.nplanes;
  int rc = bind(ctx);
  if (rc) return rc;
  if (nplanes < 1 || !geom_ok(sh.rows, sh.cols, sh.wpr) || !outs_ok(og, oe) || (sh.rows && !planes)) return BIC_EINVAL;
  if (sh.rows == 0) {
    if (og.out) BIC_HIP((bic::launch_fill(ctx->cur, og.bits, 0, sizeof(uint64_t) * nplanes), hipGetLastError()));
    if (oe.out) BIC_HIP((bic::launch_fill(ctx->cur, oe.bits, 0, sizeof(uint64_t) * nplanes), hipGetLastError()));
    if (og.off) BIC_HIP((bic::launch_fill(ctx->cur, og.off, 0, sizeof(uint64_t) * (nplanes + 1)), hipGetLastError()));
    if (oe.off) BIC_HIP((bic::launch_fill(ctx->cur, oe.off, 0, sizeof(uint64_t) * (nplanes + 1)), hipGetLastError()));
    return BIC_OK;
  }
  const int pr = predict ? 1 : 0;
  const bic::Geom g = bic::make_geom(sh.rows, sh.cols, sh.wpr, nplanes);
  // packed output via slots + pack
  auto packed_after = [&] {
    return pack_after(ctx, nplanes, og, oe, [&](const bic::CoderOut& tg, const bic::CoderOut& te) {
      return encode_planes_impl(ctx, planes, sh, predict, tg, te);
    });
  };
  if (bic::fused_supported(g) && !ctx->force_multipass) {
    // one pass: residual -> runs -> both streams (bic_fused.hip, bic_fused_lookback.hip)
    const int mode = ctx->two_pass ? bic::kEncTwoPass
                     : (ctx->single_kernel || !staged_pays(ctx, g) || !bic::med_rows_supported(g, planes, nullptr))
                         ? bic::kEncSingle
                         : bic::kEncStaged;
    if (row_index && (mode != bic::kEncStaged || !og.out)) {  // the index from the staged prefix kernels
      if ((rc = encode_planes_impl(ctx, planes, sh, predict, og, oe))) return rc;
      return bic_row_index(ctx, planes, nplanes, sh.rows, sh.cols, sh.wpr, predict, row_index);
    }
    if ((og.off || oe.off) && mode != bic::kEncStaged) return packed_after();
    bic::FusedCall c{g, planes, pr, mode, {og, oe, row_index}};
    return run_fused(ctx, c, [](const bic::FusedArena&) {});
  }
  // rows wider than 16384 columns: multi-pass chunk kernels (bic_kernels.hip)
  if (row_index) return BIC_EINVAL;  // (the decoders take rows of up to 16384 columns)
  if (og.off || oe.off) return packed_after();
  if ((rc = ensure_scratch(ctx, bic::chunk_scratch_bytes(g)))) return rc;
  const bic::ChunkScratch cs = bic::carve_chunk_scratch(ctx->scratch, g);
  timed(ctx, "med_count", [&] { bic::launch_count(ctx->cur, g, planes, pr, cs, nullptr, nullptr); });
  timed(ctx, "scan_rows", [&] { bic::launch_scan_rows(ctx->cur, g, cs); });
  if (og.out) {
    timed(ctx, "golomb_bits", [&] { bic::launch_golomb_bits(ctx->cur, g, planes, pr, cs); });
    timed(ctx, "golomb_offsets", [&] {
      bic::launch_golomb_offsets(ctx->cur, g, cs, og.out, og.slot, og.bits, ctx->flags);
    });
    timed(ctx, "golomb_emit", [&] { bic::launch_golomb_emit(ctx->cur, g, planes, pr, cs, og.out, og.slot); });
  }
  if (oe.out)
    timed(ctx, "eg_emit", [&] { bic::launch_eg_emit(ctx->cur, g, planes, pr, cs, oe.out, oe.slot, oe.bits, ctx->flags); });
  BIC_HIP(hipGetLastError());
  return BIC_OK;
}

// Only the count pass (and the fallback's plane extraction) knows the sample size; everything after
// it is per (plane, row).
int encode_gray_impl(bic_ctx* ctx, const GrayImage& img, int plane0, uint64_t* planes, const Shape& sh, int predict,
                     const bic::CoderOut& og, const bic::CoderOut& oe, uint64_t* row_index = nullptr) {
  const int nplanes = sh.nplanes, bps = img.bps;
  const int nchan = bps == 3 ? 3 : 1, cplanes = nplanes / nchan;  // a sample's planes: of one channel
  const size_t rows = sh.rows, cols = sh.cols, wpr = sh.wpr;
  int rc = bind(ctx);
  if (rc) return rc;
  if (plane0 < 0 || cplanes < 1 || plane0 + cplanes > (bps == 2 ? 16 : 8) || cols > SIZE_MAX / 4 ||
      img.pitch < cols * (size_t)bps || !geom_ok(rows, cols, wpr) || !outs_ok(og, oe) || (rows && !img.data))
    return BIC_EINVAL;
  const bic::Geom g = bic::make_geom(rows, cols, wpr, nplanes);
  // EG source: no bitplanes wanted and the EG stream into slots -- the count pass writes the EG
  // stream (its uniform layout) instead of the residual planes, and the Golomb kernels read the
  // residual rows back from it (bic_internal.h FusedRequest::eg_src): no residual buffer at all
  const uint64_t eg_words = ((uint64_t)rows * (cols + 1) + 1 + 63) / 64;
  const bool fuse = rows && bic::fused_supported(g) && !ctx->force_multipass && !ctx->two_pass && !ctx->single_kernel &&
                    staged_pays(ctx, g) && bic::med_rows_supported(g, planes, nullptr) &&
                    bic::gray_rows_supported(g, img.data, img.pitch, planes, bps);
  const bool eg_src = fuse && !planes && predict && oe.out && !oe.off && bic::gray_eg_supported(g) &&
                      eg_words <= oe.slot && (og.out || !row_index) && !ctx->eg_src_off;
  if (!planes && rows && !eg_src) {
    // no bitplanes wanted: the count pass stores the med residual planes into the context's buffer
    // (the same bytes the bitplanes would take) and the encoder reads them with prediction off --
    // no row above, no med in the emission. Same streams (predict off on R = med on P).
    if ((rc = ensure_rbuf(ctx, (size_t)nplanes * rows * wpr * 8))) return rc;
  }
  const bool store_resid = !planes && predict;
  if (!planes && !eg_src) planes = ctx->rbuf;
  if (!fuse) {  // the same result through the two separate calls
    if ((rc = bps == 3 ? bic_bitplanes_rgb(ctx, img.data, img.pitch, rows, cols, plane0, cplanes, planes, wpr)
              : bps == 2 ? bic_bitplanes_u16(ctx, img.data, img.pitch, rows, cols, img.big_endian, plane0, nplanes, planes, wpr)
                       : bic_bitplanes_u8_range(ctx, img.data, img.pitch, rows, cols, plane0, nplanes, planes, wpr)))
      return rc;
    return encode_planes_impl(ctx, planes, sh, predict, og, oe, row_index);
  }
  const int pr = predict && !store_resid ? 1 : 0;  // R stored: the encoder codes it as given
  bic::FusedCall c{g, planes, pr, bic::kEncStaged, {og, oe, og.out ? row_index : nullptr}};
  c.rq.eg_src = eg_src;
  c.rq.eg_src_one = ctx->eg_src_one;
  c.rq.counted = true;
  c.rq.ns = bic::gray_strips(g);
  // (EG source: the emission is Golomb's alone, reading the residual rows from the EG stream)
  if ((rc = run_fused(ctx, c, [&](const bic::FusedArena& ar) {
         bic::launch_gray_rows(ctx->cur, img.data, img.pitch, g, predict ? 1 : 0, plane0, planes, ar.sones, ar.krec,
                               ar.kpos, ar.counter, store_resid, eg_src ? oe.out : nullptr, oe.slot, bps,
                               img.big_endian, ctx->gray_code, bps == 3 ? ctx->color_transform : 0,
                               bps == 1 ? ctx->sample_predict : bps == 3 ? ctx->rgb_predict : 0);
       })))
    return rc;
  if (row_index && !og.out) return bic_row_index(ctx, planes, nplanes, rows, cols, wpr, pr, row_index);
  return BIC_OK;
}

// nframes gray images of one geometry (frame f at img.data + f * stride) in one encode: fplanes planes per
// frame, output entry f * fplanes + k = plane plane0 + k of frame f. As in encode_gray_impl only the count pass
// (k_gray_strips_frames, one-byte samples) and the fallback's plane extraction know the frames; everything
// after them is per (plane, row) over nframes * fplanes planes. One frame is encode_gray_impl itself.
// bps = 3 (bic_encode_rgb_frames): interleaved RGB frames, fplanes = 3 x one channel's planes as in
// encode_gray_impl, entry (f * 3 + c) * (fplanes / 3) + k = plane plane0 + k of channel c of frame f; the count
// pass is k_gray_strips_rgb_frames ("rgb_frames_count" in the profile), the fallback bic_bitplanes_rgb per frame.
int encode_gray_frames_impl(bic_ctx* ctx, const GrayImage& img, size_t stride, int nframes, int plane0, int fplanes,
                            uint64_t* planes, size_t rows, size_t cols, size_t wpr, int predict,
                            const bic::CoderOut& og, const bic::CoderOut& oe, uint64_t* row_index = nullptr) {
  const int bps = img.bps;
  const int nchan = bps == 3 ? 3 : 1, cplanes = fplanes / nchan;  // a sample's planes: of one channel
  int rc = bind(ctx);
  if (rc) return rc;
  if (nframes < 1 || cplanes < 1 || (uint64_t)nframes * (uint64_t)fplanes > 65535 || bps < 1 || bps > 3 ||
      plane0 < 0 || plane0 + cplanes > (bps == 2 ? 16 : 8) || cols > SIZE_MAX / 4 || img.pitch < cols * (size_t)bps ||
      !geom_ok(rows, cols, wpr) || !outs_ok(og, oe) || (rows && !img.data))
    return BIC_EINVAL;
  if (nframes > 1 && (rows > SIZE_MAX / img.pitch || stride < rows * img.pitch)) return BIC_EINVAL;
  if (nframes == 1)
    return encode_gray_impl(ctx, img, plane0, planes, {fplanes, rows, cols, wpr}, predict, og, oe, row_index);
  const int nplanes = nframes * fplanes;
  const Shape sh{nplanes, rows, cols, wpr};
  if (rows == 0) return encode_planes_impl(ctx, planes, sh, predict, og, oe, row_index);  // zero counts and offsets
  const bic::Geom g = bic::make_geom(rows, cols, wpr, nplanes);
  const bool store_resid = !planes && predict;
  const uint64_t eg_words = ((uint64_t)rows * (cols + 1) + 1 + 63) / 64;
  const bool fuse = bps != 2 && bic::fused_supported(g) && !ctx->force_multipass && !ctx->two_pass &&
                    !ctx->single_kernel && staged_pays(ctx, g) && bic::med_rows_supported(g, planes, nullptr) &&
                    bic::gray_rows_supported(g, img.data, img.pitch, planes, bps);
  if (fuse && !(bps == 3 ? bic::rgb_frames_supported(g, (uint64_t)nframes, predict ? 1 : 0, store_resid)
                         : bic::gray_frames_supported(g, (uint64_t)nframes, predict ? 1 : 0, store_resid)))
    return BIC_EINVAL;
  const bool eg_src = fuse && !planes && predict && oe.out && !oe.off && bic::gray_eg_supported(g) &&
                      eg_words <= oe.slot && (og.out || !row_index) && !ctx->eg_src_off;
  // no bitplanes wanted: the residual planes (or the fallback's planes) of all frames in the context's buffer
  if (!planes && !eg_src && (rc = ensure_rbuf(ctx, (size_t)nplanes * rows * wpr * 8))) return rc;
  if (!planes && !eg_src) planes = ctx->rbuf;
  if (!fuse) {  // the same result through the separate calls, one extraction per frame
    for (int f = 0; f < nframes; ++f) {
      const uint8_t* fr = img.data + (size_t)f * stride;
      uint64_t* fp = planes + (size_t)f * fplanes * rows * wpr;
      if ((rc = bps == 3 ? bic_bitplanes_rgb(ctx, fr, img.pitch, rows, cols, plane0, cplanes, fp, wpr)
                : bps == 2 ? bic_bitplanes_u16(ctx, fr, img.pitch, rows, cols, img.big_endian, plane0, fplanes, fp, wpr)
                         : bic_bitplanes_u8_range(ctx, fr, img.pitch, rows, cols, plane0, fplanes, fp, wpr)))
        return rc;
    }
    return encode_planes_impl(ctx, planes, sh, predict, og, oe, row_index);
  }
  const int pr = predict && !store_resid ? 1 : 0;  // R stored: the encoder codes it as given
  bic::FusedCall c{g, planes, pr, bic::kEncStaged, {og, oe, og.out ? row_index : nullptr}};
  c.rq.eg_src = eg_src;
  c.rq.eg_src_one = ctx->eg_src_one;
  c.rq.counted = true;
  c.rq.ns = bic::gray_strips(g);
  if ((rc = run_fused(
           ctx, c,
           [&](const bic::FusedArena& ar) {
             if (bps == 3)
               bic::launch_rgb_frames(ctx->cur, img.data, img.pitch, stride, (uint32_t)nframes, g, predict ? 1 : 0,
                                      plane0, planes, ar.sones, ar.krec, ar.kpos, ar.counter, store_resid,
                                      eg_src ? oe.out : nullptr, oe.slot, ctx->gray_code, ctx->color_transform,
                                      ctx->rgb_predict);
             else
               bic::launch_gray_frames(ctx->cur, img.data, img.pitch, stride, (uint32_t)nframes, g, predict ? 1 : 0,
                                       plane0, planes, ar.sones, ar.krec, ar.kpos, ar.counter, store_resid,
                                       eg_src ? oe.out : nullptr, oe.slot, ctx->gray_code, ctx->sample_predict);
           },
           false, bps == 3 ? "rgb_frames_count" : "bitplanes_count")))
    return rc;
  if (row_index && !og.out) return bic_row_index(ctx, planes, nplanes, rows, cols, wpr, pr, row_index);
  return BIC_OK;
}

// nframes P4 rasters (frame f at raster + f * stride) as the planes of one encode. Only the count pass
// (and the fallback's unpacking) knows the source; everything after it is per (plane, row).
int encode_pbm_impl(bic_ctx* ctx, const uint8_t* raster, size_t stride, uint64_t* planes, const Shape& sh, int predict,
                    const bic::CoderOut& og, const bic::CoderOut& oe, uint64_t* row_index = nullptr) {
  const int nframes = sh.nplanes;
  const size_t rows = sh.rows, cols = sh.cols, wpr = sh.wpr;
  int rc = bind(ctx);
  if (rc) return rc;
  if (nframes < 1 || !geom_ok(rows, cols, wpr) || !outs_ok(og, oe) || (rows && !raster)) return BIC_EINVAL;
  const size_t frame_bytes = rows * ((cols + 7) / 8);
  if (nframes == 1) stride = frame_bytes;
  else if (stride < frame_bytes) return BIC_EINVAL;
  if (rows == 0) return encode_planes_impl(ctx, planes, sh, predict, og, oe, row_index);  // zero counts and offsets
  const bic::Geom g = bic::make_geom(rows, cols, wpr, nframes);
  // no planes wanted: the context's buffer takes the count pass's residual planes (or the fallback's planes)
  if (!planes && (rc = ensure_rbuf(ctx, (size_t)nframes * rows * wpr * 8))) return rc;
  const bool store_resid = !planes && predict;
  if (!planes) planes = ctx->rbuf;
  const bool fuse = bic::fused_supported(g) && !ctx->force_multipass && !ctx->two_pass && !ctx->single_kernel &&
                    staged_pays(ctx, g) && bic::med_rows_supported(g, planes, nullptr);
  if (!fuse) {  // the same result through the separate calls
    for (int f = 0; f < nframes; ++f)
      if ((rc = bic_pbm_unpack(ctx, raster + (size_t)f * stride, rows, cols, planes + (size_t)f * rows * wpr, wpr)))
        return rc;
    return encode_planes_impl(ctx, planes, sh, predict, og, oe, row_index);
  }
  const int pr = predict && !store_resid ? 1 : 0;  // R stored: the encoder codes it as given
  bic::FusedCall c{g, planes, pr, bic::kEncStaged, {og, oe, og.out ? row_index : nullptr}};
  c.rq.counted = true;
  c.rq.ns = 1;
  if ((rc = run_fused(ctx, c, [&](const bic::FusedArena& ar) {
         bic::launch_pbm_rows(ctx->cur, raster, stride, g, predict ? 1 : 0, planes, store_resid, ar.sones, ar.krec,
                              ar.kpos, ar.counter);
       })))
    return rc;
  if (row_index && !og.out) return bic_row_index(ctx, planes, nframes, rows, cols, wpr, pr, row_index);
  return BIC_OK;
}

}  // namespace

extern "C" {

int bic_med_residual(bic_ctx* ctx, const uint64_t* planes, int nplanes, size_t rows, size_t cols,
                     size_t wpr, int predict, uint64_t* resid, uint64_t* weight_out) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (nplanes < 1 || !geom_ok(rows, cols, wpr) || (rows && !planes)) return BIC_EINVAL;
  if (weight_out) BIC_HIP((bic::launch_fill(ctx->cur, weight_out, 0, sizeof(uint64_t) * nplanes), hipGetLastError()));
  if (rows == 0) return BIC_OK;
  const bic::Geom g = bic::make_geom(rows, cols, wpr, nplanes);
  if ((rc = ensure_scratch(ctx, bic::chunk_scratch_bytes(g)))) return rc;
  const bic::ChunkScratch cs = bic::carve_chunk_scratch(ctx->scratch, g);
  if (bic::med_rows_supported(g, planes, resid)) {
    timed(ctx, "med_count", [&] {
      bic::launch_med_rows(ctx->cur, g, planes, predict ? 1 : 0, resid, cs.ones, weight_out);
    });
  } else {
    timed(ctx, "med_count", [&] { bic::launch_count(ctx->cur, g, planes, predict ? 1 : 0, cs, resid, weight_out); });
  }
  BIC_HIP(hipGetLastError());
  return BIC_OK;
}

int bic_encode_pbm(bic_ctx* ctx, const uint8_t* raster, size_t frame_stride, int nframes, size_t rows, size_t cols,
                   uint64_t* planes, size_t wpr, int predict, uint64_t* out_golomb, size_t slot_golomb,
                   uint64_t* bits_golomb, uint64_t* out_eg, size_t slot_eg, uint64_t* bits_eg) {
  return encode_pbm_impl(ctx, raster, frame_stride, planes, {nframes, rows, cols, wpr}, predict,
                         {out_golomb, slot_golomb, bits_golomb}, {out_eg, slot_eg, bits_eg});
}

int bic_encode_pbm_packed(bic_ctx* ctx, const uint8_t* raster, size_t frame_stride, int nframes, size_t rows,
                          size_t cols, uint64_t* planes, size_t wpr, int predict, uint64_t* out_golomb,
                          size_t slot_golomb, uint64_t* bits_golomb, uint64_t* off_golomb, uint64_t* out_eg,
                          size_t slot_eg, uint64_t* bits_eg, uint64_t* off_eg, uint64_t* row_index) {
  if ((out_golomb && !off_golomb) || (out_eg && !off_eg)) return BIC_EINVAL;
  return encode_pbm_impl(ctx, raster, frame_stride, planes, {nframes, rows, cols, wpr}, predict,
                         {out_golomb, slot_golomb, bits_golomb, off_golomb}, {out_eg, slot_eg, bits_eg, off_eg},
                         row_index);
}

int bic_encode_planes2(bic_ctx* ctx, const uint64_t* planes, int nplanes, size_t rows, size_t cols,
                       size_t wpr, int predict, uint64_t* out_golomb, size_t slot_golomb,
                       uint64_t* bits_golomb, uint64_t* out_eg, size_t slot_eg, uint64_t* bits_eg) {
  return encode_planes_impl(ctx, planes, {nplanes, rows, cols, wpr}, predict, {out_golomb, slot_golomb, bits_golomb},
                            {out_eg, slot_eg, bits_eg});
}

int bic_encode_planes_packed(bic_ctx* ctx, const uint64_t* planes, int nplanes, size_t rows, size_t cols,
                             size_t wpr, int predict, uint64_t* out_golomb, size_t slot_golomb,
                             uint64_t* bits_golomb, uint64_t* off_golomb, uint64_t* out_eg, size_t slot_eg,
                             uint64_t* bits_eg, uint64_t* off_eg, uint64_t* row_index) {
  if ((out_golomb && !off_golomb) || (out_eg && !off_eg)) return BIC_EINVAL;
  return encode_planes_impl(ctx, planes, {nplanes, rows, cols, wpr}, predict,
                            {out_golomb, slot_golomb, bits_golomb, off_golomb}, {out_eg, slot_eg, bits_eg, off_eg},
                            row_index);
}

int bic_encode_gray_range(bic_ctx* ctx, const uint8_t* gray, size_t pitch, size_t rows, size_t cols, int plane0,
                          int nplanes, uint64_t* planes, size_t wpr, int predict, uint64_t* out_golomb,
                          size_t slot_golomb, uint64_t* bits_golomb, uint64_t* out_eg, size_t slot_eg,
                          uint64_t* bits_eg) {
  return encode_gray_impl(ctx, {gray, pitch, 1, 0}, plane0, planes, {nplanes, rows, cols, wpr}, predict,
                          {out_golomb, slot_golomb, bits_golomb}, {out_eg, slot_eg, bits_eg});
}

int bic_encode_gray16(bic_ctx* ctx, const void* gray, size_t pitch, size_t rows, size_t cols, int big_endian,
                      int plane0, int nplanes, uint64_t* planes, size_t wpr, int predict, uint64_t* out_golomb,
                      size_t slot_golomb, uint64_t* bits_golomb, uint64_t* out_eg, size_t slot_eg, uint64_t* bits_eg) {
  return encode_gray_impl(ctx, {static_cast<const uint8_t*>(gray), pitch, 2, big_endian ? 1 : 0}, plane0, planes,
                          {nplanes, rows, cols, wpr}, predict, {out_golomb, slot_golomb, bits_golomb},
                          {out_eg, slot_eg, bits_eg});
}

int bic_encode_gray16_packed(bic_ctx* ctx, const void* gray, size_t pitch, size_t rows, size_t cols, int big_endian,
                             int plane0, int nplanes, uint64_t* planes, size_t wpr, int predict, uint64_t* out_golomb,
                             size_t slot_golomb, uint64_t* bits_golomb, uint64_t* off_golomb, uint64_t* out_eg,
                             size_t slot_eg, uint64_t* bits_eg, uint64_t* off_eg, uint64_t* row_index) {
  if ((out_golomb && !off_golomb) || (out_eg && !off_eg)) return BIC_EINVAL;
  return encode_gray_impl(ctx, {static_cast<const uint8_t*>(gray), pitch, 2, big_endian ? 1 : 0}, plane0, planes,
                          {nplanes, rows, cols, wpr}, predict, {out_golomb, slot_golomb, bits_golomb, off_golomb},
                          {out_eg, slot_eg, bits_eg, off_eg}, row_index);
}

int bic_encode_gray_packed(bic_ctx* ctx, const uint8_t* gray, size_t pitch, size_t rows, size_t cols, int plane0,
                           int nplanes, uint64_t* planes, size_t wpr, int predict, uint64_t* out_golomb,
                           size_t slot_golomb, uint64_t* bits_golomb, uint64_t* off_golomb, uint64_t* out_eg,
                           size_t slot_eg, uint64_t* bits_eg, uint64_t* off_eg, uint64_t* row_index) {
  if ((out_golomb && !off_golomb) || (out_eg && !off_eg)) return BIC_EINVAL;
  return encode_gray_impl(ctx, {gray, pitch, 1, 0}, plane0, planes, {nplanes, rows, cols, wpr}, predict,
                          {out_golomb, slot_golomb, bits_golomb, off_golomb}, {out_eg, slot_eg, bits_eg, off_eg},
                          row_index);
}

int bic_encode_gray_frames(bic_ctx* ctx, const void* gray, size_t frame_stride, int nframes, size_t pitch, size_t rows,
                           size_t cols, int sample_bytes, int big_endian, int plane0, int nplanes, uint64_t* planes,
                           size_t wpr, int predict, uint64_t* out_golomb, size_t slot_golomb, uint64_t* bits_golomb,
                           uint64_t* out_eg, size_t slot_eg, uint64_t* bits_eg) {
  if (sample_bytes != 1 && sample_bytes != 2) return BIC_EINVAL;
  return encode_gray_frames_impl(
      ctx, {static_cast<const uint8_t*>(gray), pitch, sample_bytes, sample_bytes == 2 && big_endian ? 1 : 0},
      frame_stride, nframes, plane0, nplanes, planes, rows, cols, wpr, predict, {out_golomb, slot_golomb, bits_golomb},
      {out_eg, slot_eg, bits_eg});
}

int bic_encode_gray_frames_packed(bic_ctx* ctx, const void* gray, size_t frame_stride, int nframes, size_t pitch,
                                  size_t rows, size_t cols, int sample_bytes, int big_endian, int plane0, int nplanes,
                                  uint64_t* planes, size_t wpr, int predict, uint64_t* out_golomb, size_t slot_golomb,
                                  uint64_t* bits_golomb, uint64_t* off_golomb, uint64_t* out_eg, size_t slot_eg,
                                  uint64_t* bits_eg, uint64_t* off_eg, uint64_t* row_index) {
  if ((sample_bytes != 1 && sample_bytes != 2) || (out_golomb && !off_golomb) || (out_eg && !off_eg)) return BIC_EINVAL;
  return encode_gray_frames_impl(
      ctx, {static_cast<const uint8_t*>(gray), pitch, sample_bytes, sample_bytes == 2 && big_endian ? 1 : 0},
      frame_stride, nframes, plane0, nplanes, planes, rows, cols, wpr, predict,
      {out_golomb, slot_golomb, bits_golomb, off_golomb}, {out_eg, slot_eg, bits_eg, off_eg}, row_index);
}

int bic_encode_rgb_frames(bic_ctx* ctx, const uint8_t* rgb, size_t frame_stride, int nframes, size_t pitch, size_t rows,
                          size_t cols, int plane0, int nplanes, uint64_t* planes, size_t wpr, int predict,
                          uint64_t* out_golomb, size_t slot_golomb, uint64_t* bits_golomb, uint64_t* out_eg,
                          size_t slot_eg, uint64_t* bits_eg) {
  if (nplanes < 1 || nplanes > 8) return BIC_EINVAL;
  return encode_gray_frames_impl(ctx, {rgb, pitch, 3, 0}, frame_stride, nframes, plane0, 3 * nplanes, planes, rows, cols,
                                 wpr, predict, {out_golomb, slot_golomb, bits_golomb}, {out_eg, slot_eg, bits_eg});
}

int bic_encode_rgb_frames_packed(bic_ctx* ctx, const uint8_t* rgb, size_t frame_stride, int nframes, size_t pitch,
                                 size_t rows, size_t cols, int plane0, int nplanes, uint64_t* planes, size_t wpr,
                                 int predict, uint64_t* out_golomb, size_t slot_golomb, uint64_t* bits_golomb,
                                 uint64_t* off_golomb, uint64_t* out_eg, size_t slot_eg, uint64_t* bits_eg,
                                 uint64_t* off_eg, uint64_t* row_index) {
  if (nplanes < 1 || nplanes > 8 || (out_golomb && !off_golomb) || (out_eg && !off_eg)) return BIC_EINVAL;
  return encode_gray_frames_impl(ctx, {rgb, pitch, 3, 0}, frame_stride, nframes, plane0, 3 * nplanes, planes, rows, cols,
                                 wpr, predict, {out_golomb, slot_golomb, bits_golomb, off_golomb},
                                 {out_eg, slot_eg, bits_eg, off_eg}, row_index);
}

int bic_encode_rgb(bic_ctx* ctx, const uint8_t* rgb, size_t pitch, size_t rows, size_t cols, int plane0, int nplanes,
                   uint64_t* planes, size_t wpr, int predict, uint64_t* out_golomb, size_t slot_golomb,
                   uint64_t* bits_golomb, uint64_t* out_eg, size_t slot_eg, uint64_t* bits_eg) {
  if (nplanes < 1 || nplanes > 8) return BIC_EINVAL;
  return encode_gray_impl(ctx, {rgb, pitch, 3, 0}, plane0, planes, {3 * nplanes, rows, cols, wpr}, predict,
                          {out_golomb, slot_golomb, bits_golomb}, {out_eg, slot_eg, bits_eg});
}

int bic_encode_rgb_packed(bic_ctx* ctx, const uint8_t* rgb, size_t pitch, size_t rows, size_t cols, int plane0,
                          int nplanes, uint64_t* planes, size_t wpr, int predict, uint64_t* out_golomb,
                          size_t slot_golomb, uint64_t* bits_golomb, uint64_t* off_golomb, uint64_t* out_eg,
                          size_t slot_eg, uint64_t* bits_eg, uint64_t* off_eg, uint64_t* row_index) {
  if (nplanes < 1 || nplanes > 8 || (out_golomb && !off_golomb) || (out_eg && !off_eg)) return BIC_EINVAL;
  return encode_gray_impl(ctx, {rgb, pitch, 3, 0}, plane0, planes, {3 * nplanes, rows, cols, wpr}, predict,
                          {out_golomb, slot_golomb, bits_golomb, off_golomb}, {out_eg, slot_eg, bits_eg, off_eg},
                          row_index);
}

int bic_encode_gray(bic_ctx* ctx, const uint8_t* gray, size_t pitch, size_t rows, size_t cols, int nplanes,
                    uint64_t* planes, size_t wpr, int predict, uint64_t* out_golomb, size_t slot_golomb,
                    uint64_t* bits_golomb, uint64_t* out_eg, size_t slot_eg, uint64_t* bits_eg) {
  return bic_encode_gray_range(ctx, gray, pitch, rows, cols, 0, nplanes, planes, wpr, predict, out_golomb,
                               slot_golomb, bits_golomb, out_eg, slot_eg, bits_eg);
}

int bic_row_index(bic_ctx* ctx, const uint64_t* planes, int nplanes, size_t rows, size_t cols, size_t wpr,
                  int predict, uint64_t* index) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (nplanes < 1 || !geom_ok(rows, cols, wpr) || (rows && (!planes || !index))) return BIC_EINVAL;
  if (rows == 0) return BIC_OK;
  const bic::Geom g = bic::make_geom(rows, cols, wpr, nplanes);
  if (!bic::fused_supported(g)) return BIC_EINVAL;
  if (!bic::med_rows_supported(g, planes, nullptr)) {
    // the count kernel reads 16-byte pairs of words: an even-pitched, aligned copy of the planes
    const size_t wpr2 = (wpr + 1) & ~(size_t)1;
    uint64_t* tmp = nullptr;
    BIC_HIP(hipMallocAsync(reinterpret_cast<void**>(&tmp), (size_t)nplanes * rows * wpr2 * 8, ctx->cur));
    rc = BIC_OK;
    if (hipMemcpy2DAsync(tmp, wpr2 * 8, planes, wpr * 8, wpr * 8, (size_t)nplanes * rows, hipMemcpyDeviceToDevice,
                         ctx->cur) != hipSuccess)
      rc = BIC_EDEVICE;
    if (rc == BIC_OK) rc = bic_row_index(ctx, tmp, nplanes, rows, cols, wpr2, predict, index);
    (void)hipFreeAsync(tmp, ctx->cur);
    return rc;
  }
  // the staged encoder's prefix kernels alone (counts, scans, the walk of mixed-k rows, the
  // length scan): they touch no output words, only the scratch and the index
  const bic::CoderOut slot_only{nullptr, bic_encode_slot_words(rows, cols, BIC_CODER_GOLOMB)};
  bic::FusedCall c{g, planes, predict ? 1 : 0, bic::kEncStaged, {slot_only, {}, index}};
  return run_fused(ctx, c, [](const bic::FusedArena&) {}, /*prefix_only=*/true);
}

int bic_encode_planes(bic_ctx* ctx, const uint64_t* planes, int nplanes, size_t rows, size_t cols,
                      size_t wpr, int predict, int coder, uint64_t* out, size_t slot_words,
                      uint64_t* plane_bits) {
  if (coder == BIC_CODER_GOLOMB)
    return bic_encode_planes2(ctx, planes, nplanes, rows, cols, wpr, predict, out, slot_words, plane_bits,
                              nullptr, 0, nullptr);
  if (coder == BIC_CODER_EG)
    return bic_encode_planes2(ctx, planes, nplanes, rows, cols, wpr, predict, nullptr, 0, nullptr, out,
                              slot_words, plane_bits);
  if (coder == BIC_CODER_EG_ADAPTIVE) {  // bic_egad.hip
    int rc = bind(ctx);
    if (rc) return rc;
    if (nplanes < 1 || !geom_ok(rows, cols, wpr) || (rows && (!planes || !out || !plane_bits)) || slot_words == 0)
      return BIC_EINVAL;
    if (rows == 0) {
      BIC_HIP((bic::launch_fill(ctx->cur, plane_bits, 0, sizeof(uint64_t) * nplanes), hipGetLastError()));
      return BIC_OK;
    }
    if ((rc = ensure_scratch(ctx, bic::egad_scratch_bytes((uint64_t)rows * nplanes)))) return rc;
    timed(ctx, "encode_eg_adaptive", [&] {
      bic::launch_egad(ctx->cur, planes, (uint32_t)rows, (uint32_t)cols, (uint32_t)wpr, (uint32_t)nplanes,
                       predict ? 1 : 0, out, slot_words, plane_bits, ctx->scratch, ctx->flags, nullptr,
                       ctx->lut + bic::kLutEgadNib);
    });
    BIC_HIP(hipGetLastError());
    return BIC_OK;
  }
  return BIC_EINVAL;
}

int bic_egad_row_index(bic_ctx* ctx, const uint64_t* planes, int nplanes, size_t rows, size_t cols, size_t wpr,
                       int predict, uint64_t* index) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (nplanes < 1 || !geom_ok(rows, cols, wpr) || (rows && (!planes || !index))) return BIC_EINVAL;
  if (rows == 0) return BIC_OK;
  const uint64_t n = (uint64_t)rows * nplanes;
  const size_t sb = (bic::egad_scratch_bytes(n) + 255) & ~(size_t)255;
  if ((rc = ensure_scratch(ctx, sb + (size_t)nplanes * 8))) return rc;
  // a slot no row can overflow: <= 17 bits per column and end-of-row (a '1' per zero or block, a
  // '0' and <= 15 remainder bits per 1)
  const uint64_t slot = ((uint64_t)rows * (cols + 1) * 17 + 63) / 64;
  uint64_t* bits = reinterpret_cast<uint64_t*>(static_cast<char*>(ctx->scratch) + sb);
  timed(ctx, "egad_row_index", [&] {
    bic::launch_egad(ctx->cur, planes, (uint32_t)rows, (uint32_t)cols, (uint32_t)wpr, (uint32_t)nplanes,
                     predict ? 1 : 0, nullptr, slot, bits, ctx->scratch, ctx->flags, index, ctx->lut + bic::kLutEgadNib);
  });
  BIC_HIP(hipGetLastError());
  return BIC_OK;
}

}  // extern "C"
