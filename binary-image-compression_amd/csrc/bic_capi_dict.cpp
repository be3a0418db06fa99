// bic_capi_dict.cpp -- the growing-dictionary tile coder's entry points (bic_dict.hip).
#include "bic_ctx.h"

#include <cmath>

extern "C" {

int bic_dict_encode(bic_ctx* ctx, int variant, const uint64_t* plane, size_t rows, size_t cols, size_t wpr, unsigned W,
                    unsigned T, unsigned atom_step, const double* enuml, uint32_t* bestk, uint32_t* bestd,
                    uint32_t* dsize, uint32_t* weights, uint8_t* modes, uint8_t* joined, uint32_t* dict_tiles,
                    uint64_t* stream_match, uint64_t* stream_nomatch, size_t cap_words, uint64_t* stats) {
  if (!ctx || (variant != 2 && variant != 3) || W < 1 || W > 64 || (atom_step != 1 && atom_step != W))
    return BIC_EINVAL;
  if (!plane || !enuml || !stats || !geom_ok(rows, cols, wpr)) return BIC_EINVAL;
  if ((stream_match == nullptr) != (stream_nomatch == nullptr) || (stream_match ? cap_words == 0 : cap_words != 0))
    return BIC_EINVAL;
  const size_t M = (size_t)W * W;
  const size_t ntiles = ((W - 1 + rows) / W) * ((W - 1 + cols) / W);
  if (ntiles >= 0x80000000ull / 64) return BIC_EINVAL;
  for (size_t w = 0; w <= M; ++w)
    if (!(enuml[w] >= 0.0 && enuml[w] < 1e15)) return BIC_EINVAL;  // lengths stay exact in double
  int rc = bind(ctx);
  if (rc) return rc;
  if ((rc = ctx->enuml.upload(ctx->cur, enuml, M + 1))) return rc;
  if (ntiles == 0) {
    BIC_HIP((bic::launch_fill(ctx->cur, stats, 0, 5 * sizeof(uint64_t)), hipGetLastError()));
    return BIC_OK;
  }
  if ((rc = ensure_scratch(ctx, bic::dict_scratch_bytes(ntiles, W)))) return rc;
  bic::DictArgs a{};
  a.I = plane;
  a.rows = (uint32_t)rows;
  a.cols = (uint32_t)cols;
  a.wpr = (uint32_t)wpr;
  a.used = (uint32_t)((cols + 63) / 64);
  a.W = W;
  a.nx = (uint32_t)((W - 1 + cols) / W);
  a.ny = (uint32_t)((W - 1 + rows) / W);
  a.T = T;
  a.step = atom_step;
  a.variant = (uint32_t)variant;
  a.h = variant == 2 ? 0.5 * std::log2((double)M) : 0.0;  // compress3_test.cpp:111-115: weight_len = 0
  a.enuml = ctx->enuml.dev;
  a.bestk = bestk;
  a.bestd = bestd;
  a.dsize = dsize;
  a.weights = weights;
  a.modes = modes;
  a.joined = joined;
  a.dict_tiles = dict_tiles;
  bic::dict_carve(a, ctx->scratch);
  // Every launch below is enqueued at once: a distance grid is sized for one atom per earlier tile and
  // reads |D| on the device, so the host never waits for a block.
  const uint32_t nt = (uint32_t)ntiles, B = bic::dict_block_tiles(W, ctx->dict_block);
  timed(ctx, "dict_gather", [&] { bic::launch_dict_gather(ctx->cur, a); });
  for (uint32_t t0 = 0; t0 < nt; t0 += B) {
    const uint32_t bn = nt - t0 < B ? nt - t0 : B;
    if (t0) timed(ctx, "dict_dist", [&] { bic::launch_dict_dist(ctx->cur, a, t0, bn); });
    timed(ctx, "dict_resolve", [&] { bic::launch_dict_resolve(ctx->cur, a, t0, bn); });
  }
  if (variant == 3) {  // every tile but the first codes a sample (compress3_test.cpp:117-122, 131-141)
    bic::MatchArgs m{};
    m.weights = a.weights + 1;
    m.modes = a.modes + 1;
    m.lens = a.lens + 1;
    m.nx = nt - 1;
    m.ny = 1;
    m.flags = stream_match ? ctx->flags : a.noflags;  // without streams the lengths only: nothing can overflow
    timed(ctx, "dict_code", [&] {
      bic::launch_match_code(ctx->cur, m, reinterpret_cast<unsigned long long*>(stream_match),
                             reinterpret_cast<unsigned long long*>(stream_nomatch), cap_words, stats);
    });
  }
  timed(ctx, "dict_finish", [&] { bic::launch_dict_finish(ctx->cur, a, stats); });
  BIC_HIP(hipGetLastError());
  return BIC_OK;
}

int bic_set_dict_block(bic_ctx* ctx, unsigned tiles) {
  if (!ctx) return BIC_EINVAL;
  ctx->dict_block = tiles;
  return BIC_OK;
}

}  // extern "C"
