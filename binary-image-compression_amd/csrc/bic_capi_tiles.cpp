// bic_capi_tiles.cpp -- the sample coder, the tile coder and the match loop's entry points
// (bic_kernels.hip, bic_match.hip).
#include "bic_ctx.h"

namespace {

int match_encode_impl(bic_ctx* ctx, const uint64_t* plane, size_t rows, size_t cols, size_t wpr, unsigned W,
                      unsigned T, unsigned R, const double* enuml, uint32_t* besti, uint32_t* bestj,
                      uint32_t* bestd, uint32_t* weights, uint8_t* modes, uint64_t* resid,
                      uint64_t* stream_match, uint64_t* stream_nomatch, size_t cap_words, uint64_t* stats,
                      int invert, uint8_t* inverted, int var = 0) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (!plane || !resid || !enuml || !stream_match || !stream_nomatch || !stats || cap_words == 0)
    return BIC_EINVAL;
  if (W < 1 || W > 64 || rows % W || cols % W || !geom_ok(rows, cols, wpr)) return BIC_EINVAL;
  if (R > 32767 || T > 0x7fffffffu || rows > 0x3fffffffu || cols > 0x3fffffffu) return BIC_EINVAL;
  const size_t M = (size_t)W * W;
  const size_t ntiles = (rows / W) * (cols / W);
  if (ntiles >= 0x80000000ull / 64 || (unsigned long long)ntiles * M >= 0x80000000ull) return BIC_EINVAL;
  for (size_t w = 0; w <= M; ++w)
    if (!(enuml[w] >= 0.0 && enuml[w] < 1e15)) return BIC_EINVAL;  // lengths stay exact in double
  if ((rc = ctx->enuml.upload(ctx->cur, enuml, M + 1))) return rc;
  if (ntiles == 0) {
    BIC_HIP((bic::launch_fill(ctx->cur, stats, 0, 4 * sizeof(uint64_t)), hipGetLastError()));
    return BIC_OK;
  }
  const bic::MatchSched sched = bic::match_schedule(W, R, (uint32_t)cols, ctx->match_parts, (uint32_t)var,
                                                    (uint32_t)rows);
  if ((rc = ensure_scratch(ctx, bic::match_scratch_bytes(ntiles, sched)))) return rc;
  if (resid != plane)
    BIC_HIP(hipMemcpyAsync(resid, plane, rows * wpr * sizeof(uint64_t), hipMemcpyDeviceToDevice, ctx->cur));
  bic::MatchArgs a{};
  a.I = resid;
  a.rows = (uint32_t)rows;
  a.cols = (uint32_t)cols;
  a.wpr = (uint32_t)wpr;
  a.used = (uint32_t)((cols + 63) / 64);
  a.W = W;
  a.nx = (uint32_t)(cols / W);
  a.ny = (uint32_t)(rows / W);
  a.T = T;
  a.R = (int)R;
  a.enuml = ctx->enuml.dev;
  a.besti = besti;
  a.bestj = bestj;
  a.bestd = bestd;
  a.weights = weights;
  a.modes = modes;
  a.flags = ctx->flags;
  a.inv = invert ? 1u : 0u;
  a.inverted = inverted;
  a.var = (uint32_t)var;
  timed(ctx, "match_tiles", [&] { bic::launch_match_tiles(ctx->cur, a, sched, ctx->scratch); });
  timed(ctx, "match_code", [&] {
    bic::launch_match_code(ctx->cur, a, reinterpret_cast<unsigned long long*>(stream_match),
                           reinterpret_cast<unsigned long long*>(stream_nomatch), cap_words, stats);
  });
  BIC_HIP(hipGetLastError());
  return BIC_OK;
}

}  // namespace

extern "C" {

int bic_golomb_encode_samples(bic_ctx* ctx, const uint32_t* samples, size_t n, uint64_t n0,
                              uint64_t a0, unsigned bit0, uint64_t* out, size_t cap_words,
                              uint64_t* bits_out) {
  int rc = bind(ctx);
  if (rc) return rc;
  // out == NULL with cap_words == 0: the lengths only (bits_out), no stream written
  if ((!samples && n) || !bits_out || bit0 >= 64 || (out ? cap_words == 0 : cap_words != 0)) return BIC_EINVAL;
  if (n0 + n >= 0x80000000ull || a0 >= 0x80000000ull) return BIC_EINVAL;
  if ((rc = ensure_scratch(ctx, bic::sample_scratch_bytes(n)))) return rc;
  const bic::SampleScratch ss = bic::carve_sample_scratch(ctx->scratch, n);
  timed(ctx, "golomb_samples", [&] {
    bic::launch_golomb_samples(ctx->cur, samples, n, n0, a0, bit0, out, cap_words, bits_out, ss, ctx->flags);
  });
  BIC_HIP(hipGetLastError());
  return BIC_OK;
}

int bic_patch_encode(bic_ctx* ctx, const uint64_t* plane, size_t rows, size_t cols, size_t wpr,
                     unsigned W, const uint64_t* lentab, uint32_t* weights, uint32_t* w_nonpred,
                     uint32_t* w_pred, uint8_t* modes, uint64_t* resid, uint64_t* stream,
                     size_t cap_words, uint64_t* stats) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (!plane || !lentab || !stream || !stats || cap_words == 0) return BIC_EINVAL;
  if (W < 1 || W > 64 || rows % W || cols % W || !geom_ok(rows, cols, wpr)) return BIC_EINVAL;
  const size_t M = (size_t)W * W;
  const size_t ntiles = (rows / W) * (cols / W);
  if (ntiles >= 0x80000000ull || (unsigned long long)ntiles * M >= 0x80000000ull) return BIC_EINVAL;
  // (the usual case, one W per run: the table is already on the device)
  if ((rc = ctx->lentab.upload(ctx->cur, lentab, M + 1))) return rc;
  // per-tile chosen weights feed the sample coder: use the caller's array or scratch
  const size_t wbytes = ((ntiles * sizeof(uint32_t)) + 255) & ~(size_t)255;
  const uint32_t nsplit = bic::tiles_split_blocks((uint32_t)rows, (uint32_t)cols, W);
  const size_t lbytes = ((size_t)nsplit * 8 + 255) & ~(size_t)255;
  if ((rc = ensure_scratch(ctx, wbytes + lbytes + bic::sample_scratch_bytes(ntiles)))) return rc;
  uint32_t* wts = weights ? weights : reinterpret_cast<uint32_t*>(ctx->scratch);
  uint64_t* lpart = reinterpret_cast<uint64_t*>(reinterpret_cast<char*>(ctx->scratch) + wbytes);
  const bic::SampleScratch ss =
      bic::carve_sample_scratch(reinterpret_cast<char*>(ctx->scratch) + wbytes + lbytes, ntiles);
  if (nsplit) {
    // three launches: tiles (which zero the coder's scratch and leave per-block length sums), the
    // coder's scan and emit (stats[0..1] from the scan, stats[2] = the length sums, from the emit)
    timed(ctx, "tiles", [&] {
      bic::launch_tiles_split(ctx->cur, plane, (uint32_t)rows, (uint32_t)cols, (uint32_t)wpr, W, ctx->lentab.dev, wts,
                              w_nonpred, w_pred, modes, resid, lpart, ss.counter, (uint32_t)(ss.zero_bytes / 4));
    });
    timed(ctx, "golomb_samples", [&] {
      bic::launch_golomb_samples(ctx->cur, wts, ntiles, 0, 0, 0, stream, cap_words, stats, ss, ctx->flags, true, lpart,
                                 nsplit, stats + 2);
    });
    BIC_HIP(hipGetLastError());
    return BIC_OK;
  }
  BIC_HIP((bic::launch_fill(ctx->cur, stats, 0, 3 * sizeof(uint64_t)), hipGetLastError()));
  timed(ctx, "tiles", [&] {
    bic::launch_tiles(ctx->cur, plane, (uint32_t)rows, (uint32_t)cols, (uint32_t)wpr, W, ctx->lentab.dev, wts,
                      w_nonpred, w_pred, modes, resid, stats);
  });
  timed(ctx, "golomb_samples", [&] {
    bic::launch_golomb_samples(ctx->cur, wts, ntiles, 0, 0, 0, stream, cap_words, stats, ss, ctx->flags);
  });
  BIC_HIP(hipGetLastError());
  return BIC_OK;
}

int bic_patch_search(bic_ctx* ctx, const uint64_t* plane, size_t rows, size_t cols, size_t wpr, unsigned W,
                     uint32_t* besti, uint32_t* bestj, uint32_t* bestd) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (W < 1 || W > 64 || !geom_ok(rows, cols, wpr) || rows > 0x7fffffffu) return BIC_EINVAL;
  const size_t ntiles = ((W - 1 + rows) / W) * ((W - 1 + cols) / W);
  if (ntiles && (!plane || !besti || !bestj || !bestd)) return BIC_EINVAL;
  if ((unsigned long long)rows * cols >= (1ull << 40)) return BIC_EINVAL;  // scan index field
  timed(ctx, "patch_search", [&] {
    bic::launch_patch_search(ctx->cur, plane, (uint32_t)rows, (uint32_t)cols, (uint32_t)wpr, W, besti, bestj, bestd);
  });
  BIC_HIP(hipGetLastError());
  return BIC_OK;
}

int bic_match_encode(bic_ctx* ctx, const uint64_t* plane, size_t rows, size_t cols, size_t wpr, unsigned W,
                     unsigned T, unsigned R, const double* enuml, uint32_t* besti, uint32_t* bestj,
                     uint32_t* bestd, uint32_t* weights, uint8_t* modes, uint64_t* resid,
                     uint64_t* stream_match, uint64_t* stream_nomatch, size_t cap_words, uint64_t* stats) {
  return match_encode_impl(ctx, plane, rows, cols, wpr, W, T, R, enuml, besti, bestj, bestd, weights, modes, resid,
                           stream_match, stream_nomatch, cap_words, stats, 0, nullptr);
}

int bic_match_encode_inv(bic_ctx* ctx, const uint64_t* plane, size_t rows, size_t cols, size_t wpr, unsigned W,
                         unsigned T, unsigned R, const double* enuml, uint32_t* besti, uint32_t* bestj,
                         uint32_t* bestd, uint32_t* weights, uint8_t* modes, uint8_t* inverted, uint64_t* resid,
                         uint64_t* stream_match, uint64_t* stream_nomatch, size_t cap_words, uint64_t* stats) {
  return match_encode_impl(ctx, plane, rows, cols, wpr, W, T, R, enuml, besti, bestj, bestd, weights, modes, resid,
                           stream_match, stream_nomatch, cap_words, stats, 1, inverted);
}

int bic_match_encode_var(bic_ctx* ctx, int variant, const uint64_t* plane, size_t rows, size_t cols, size_t wpr,
                         unsigned W, unsigned T, unsigned R, const double* enuml, uint32_t* besti, uint32_t* bestj,
                         uint32_t* bestd, uint32_t* weights, uint8_t* modes, uint64_t* resid, uint64_t* stream_match,
                         uint64_t* stream_nomatch, size_t cap_words, uint64_t* stats) {
  if (variant == 7 || variant == 8)
    return match_encode_impl(ctx, plane, rows, cols, wpr, W, T, R, enuml, besti, bestj, bestd, weights, modes, resid,
                             stream_match, stream_nomatch, cap_words, stats, variant == 8, nullptr);
  if (variant < 4 || variant > 6) return BIC_EINVAL;
  return match_encode_impl(ctx, plane, rows, cols, wpr, W, T, R, enuml, besti, bestj, bestd, weights, modes, resid,
                           stream_match, stream_nomatch, cap_words, stats, 0, nullptr, variant);
}

int bic_set_match_parts(bic_ctx* ctx, unsigned parts) {
  if (!ctx) return BIC_EINVAL;
  ctx->match_parts = parts;
  return BIC_OK;
}

}  // extern "C"
