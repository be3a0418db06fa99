// bic_capi_patch.cpp -- the image mode of the dictionary-learning driver (bsvd_test.cpp:78-151): a plane's tiles as
// samples, samples back as tiles, render_mosaic's image, and the driver's image-mode body as one call, over the
// kernels of bic_patch.hip, bic_bsvd_initialize and bic_bsvd_learn_lm.
#include "bic_ctx.h"

namespace {

constexpr size_t kPatchMaxW = 1024, kPatchMaxM = 1048576, kImageMaxW = 64;

struct PatchGeom {
  size_t nx, ny, n, used, xw;
};

// rows x cols in tiles of W: false outside the domain of bic_patches_gather / bic_patches_scatter
bool patch_geom(size_t rows, size_t cols, size_t wpr, unsigned W, size_t x_wpr, PatchGeom* g) {
  if (rows < 1 || rows > 0x7fffffffu || cols < 1 || cols > 0x7ffffffeu || W < 1 || W > kPatchMaxW) return false;
  g->nx = (cols + W - 1) / W;
  g->ny = (rows + W - 1) / W;
  g->n = g->nx * g->ny;
  g->used = (cols + 63) / 64;
  g->xw = ((size_t)W * W + 63) / 64;
  return g->n <= 0x7fffffffu && wpr >= g->used && wpr <= 0xffffffffu && x_wpr >= g->xw && x_wpr <= 0xffffffffu;
}

// floor(sqrt(v)) and ceil(sqrt(v)) in integers
size_t isqrt_floor(size_t v) {
  size_t r = 0;
  while ((r + 1) * (r + 1) <= v) ++r;
  return r;
}
size_t isqrt_ceil(size_t v) {
  const size_t r = isqrt_floor(v);
  return r * r == v ? r : r + 1;
}

struct MosaicGeom {
  size_t w, gn, rows, cols;
};
bool mosaic_geom(size_t n, size_t m, MosaicGeom* g) {
  if (n < 1 || n > 0x7fffffffu || m < 1 || m > kPatchMaxM) return false;
  g->w = isqrt_floor(m);
  g->gn = isqrt_ceil(n);
  g->rows = ((n + g->gn - 1) / g->gn) * (g->w + 1);
  g->cols = g->gn * (g->w + 1);
  return true;
}

}  // namespace

extern "C" {

int bic_patches_gather(bic_ctx* ctx, const uint64_t* plane, size_t rows, size_t cols, size_t wpr, unsigned W,
                       uint64_t* X, size_t x_wpr) {
  int rc = bind(ctx);
  if (rc) return rc;
  PatchGeom g;
  if (!plane || !X || !patch_geom(rows, cols, wpr, W, x_wpr, &g)) return BIC_EINVAL;
  timed(ctx, "patches_gather", [&] {
    bic::launch_patches_gather(ctx->cur, plane, (uint32_t)rows, (uint32_t)cols, (uint32_t)wpr, W, X, (uint32_t)x_wpr);
  });
  BIC_HIP(hipGetLastError());
  return BIC_OK;
}

int bic_patches_scatter(bic_ctx* ctx, const uint64_t* X, size_t x_wpr, unsigned W, uint64_t* plane, size_t rows,
                        size_t cols, size_t wpr) {
  int rc = bind(ctx);
  if (rc) return rc;
  PatchGeom g;
  if (!plane || !X || !patch_geom(rows, cols, wpr, W, x_wpr, &g)) return BIC_EINVAL;
  timed(ctx, "patches_scatter", [&] {
    bic::launch_patches_scatter(ctx->cur, X, (uint32_t)x_wpr, W, plane, (uint32_t)rows, (uint32_t)cols, (uint32_t)wpr);
  });
  BIC_HIP(hipGetLastError());
  return BIC_OK;
}

int bic_mosaic_dims(size_t n, size_t m, size_t* rows, size_t* cols) {
  MosaicGeom g;
  if (!rows || !cols || !mosaic_geom(n, m, &g)) return BIC_EINVAL;
  *rows = g.rows;
  *cols = g.cols;
  return BIC_OK;
}

int bic_mosaic(bic_ctx* ctx, const uint64_t* D, size_t n, size_t m, size_t d_wpr, uint64_t* image, size_t i_wpr) {
  int rc = bind(ctx);
  if (rc) return rc;
  MosaicGeom g;
  if (!D || !image || !mosaic_geom(n, m, &g)) return BIC_EINVAL;
  if (d_wpr < (m + 63) / 64 || d_wpr > 0xffffffffu || i_wpr < (g.cols + 63) / 64 || i_wpr > 0xffffffffu)
    return BIC_EINVAL;
  timed(ctx, "mosaic", [&] {
    bic::launch_mosaic(ctx->cur, D, (uint32_t)n, (uint32_t)d_wpr, (uint32_t)g.w, (uint32_t)g.gn, (uint32_t)g.rows,
                       (uint32_t)g.cols, image, (uint32_t)i_wpr);
  });
  BIC_HIP(hipGetLastError());
  return BIC_OK;
}

int bic_bsvd_learn_image(bic_ctx* ctx, int mi, int lm, int du, const uint64_t* plane, size_t rows, size_t cols,
                         size_t wpr, unsigned W, uint64_t* X, size_t x_wpr, uint64_t* E, size_t e_wpr, uint64_t* D,
                         size_t p, size_t d_wpr, uint64_t* A, size_t a_wpr, uint64_t* rng_state, size_t max_iter,
                         size_t* iters, uint64_t* residual, size_t r_wpr) {
  int rc = bind(ctx);
  if (rc) return rc;
  // the intersection of the five calls' domains, so that nothing is launched for a call that one of them refuses
  PatchGeom g;
  if (!plane || !X || !E || !D || !A || W > kImageMaxW || !patch_geom(rows, cols, wpr, W, x_wpr, &g)) return BIC_EINVAL;
  if (mi < BIC_BSVD_MI_NEIGHBOR || mi > BIC_BSVD_MI_CENTROIDS_XOR || (mi != BIC_BSVD_MI_PARTITION && !rng_state))
    return BIC_EINVAL;
  if (lm < BIC_BSVD_LM_TRADITIONAL || lm > BIC_BSVD_LM_ALTER3 || (lm != BIC_BSVD_LM_TRADITIONAL && g.n > 1048576))
    return BIC_EINVAL;
  if (du != BIC_BSVD_DU_STEEPEST && du != BIC_BSVD_DU_PROXIMUS) return BIC_EINVAL;
  if (p < 1 || p > 4096 || e_wpr < g.xw || e_wpr > 0xffffffffu || d_wpr < g.xw || d_wpr > 0xffffffffu ||
      a_wpr < (p + 63) / 64 || a_wpr > 0xffffffffu)
    return BIC_EINVAL;
  if (residual && (r_wpr < g.used || r_wpr > 0xffffffffu)) return BIC_EINVAL;
  const size_t m = (size_t)W * W;
  if ((rc = bic_patches_gather(ctx, plane, rows, cols, wpr, W, X, x_wpr))) return rc;
  timed(ctx, "bsvd_mdl_copy", [&] {  // E = X, the rows' own words (bsvd_test.cpp:114-119)
    bic::launch_bsvd_mdl_copy(ctx->cur, E, (uint32_t)e_wpr, X, (uint32_t)x_wpr, (uint32_t)g.n, (uint32_t)g.xw);
  });
  BIC_HIP(hipGetLastError());
  if ((rc = bic_bsvd_initialize(ctx, mi, E, g.n, m, e_wpr, D, p, d_wpr, A, a_wpr, rng_state))) return rc;
  if ((rc = bic_bsvd_learn_lm(ctx, lm, du, X, x_wpr, E, g.n, m, e_wpr, D, p, d_wpr, A, a_wpr, max_iter, iters)))
    return rc;
  if (residual) return bic_patches_scatter(ctx, E, e_wpr, W, residual, rows, cols, r_wpr);
  return BIC_OK;
}

}  // extern "C"
