// bic_capi_raster.cpp -- the raster converters' entry points (samples and P4 rasters to planes and
// back, bic_raster.hip and bic_kernels.hip) and bic_pack_streams. None of them uses the arena.
#include "bic_ctx.h"

extern "C" {

int bic_bitplanes_u8_range(bic_ctx* ctx, const uint8_t* gray, size_t pitch, size_t rows, size_t cols, int plane0,
                           int nplanes, uint64_t* planes, size_t wpr) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (plane0 < 0 || nplanes < 1 || plane0 + nplanes > 8 || pitch < cols || (rows && (!gray || !planes)))
    return BIC_EINVAL;
  if (!geom_ok(rows, cols, wpr)) return BIC_EINVAL;
  if (rows == 0) return BIC_OK;
  timed(ctx, "bitplanes_u8", [&] {
    bic::launch_bitplanes_u8(ctx->cur, gray, pitch, (uint32_t)rows, (uint32_t)cols, plane0, nplanes, planes,
                             (uint32_t)wpr, ctx->gray_code, ctx->sample_predict);
  });
  BIC_HIP(hipGetLastError());
  return BIC_OK;
}

int bic_bitplanes_u16(bic_ctx* ctx, const void* gray, size_t pitch, size_t rows, size_t cols, int big_endian,
                      int plane0, int nplanes, uint64_t* planes, size_t wpr) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (plane0 < 0 || nplanes < 1 || plane0 + nplanes > 16 || cols > SIZE_MAX / 2 || pitch < 2 * cols ||
      (rows && (!gray || !planes)))
    return BIC_EINVAL;
  if (!geom_ok(rows, cols, wpr)) return BIC_EINVAL;
  if (rows == 0) return BIC_OK;
  timed(ctx, "bitplanes_u16", [&] {
    bic::launch_raster_planes(ctx->cur, static_cast<const uint8_t*>(gray), 2, (uint32_t)rows, (uint32_t)cols, plane0,
                              nplanes, planes, (uint32_t)wpr, (uint64_t)pitch, big_endian ? 1 : 0, ctx->gray_code);
  });
  BIC_HIP(hipGetLastError());
  return BIC_OK;
}

int bic_bitplanes_u8(bic_ctx* ctx, const uint8_t* gray, size_t pitch, size_t rows, size_t cols,
                     int nplanes, uint64_t* planes, size_t wpr) {
  return bic_bitplanes_u8_range(ctx, gray, pitch, rows, cols, 0, nplanes, planes, wpr);
}

int bic_pack_streams(bic_ctx* ctx, const uint64_t* slots, int nplanes, size_t slot_words,
                     const uint64_t* plane_bits, uint64_t* dst, uint64_t* word_off) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (!slots || !plane_bits || !dst || !word_off || nplanes < 1 || nplanes > 65535 || slot_words == 0)
    return BIC_EINVAL;
  timed(ctx, "pack", [&] { bic::launch_pack(ctx->cur, slots, nplanes, slot_words, plane_bits, dst, word_off); });
  BIC_HIP(hipGetLastError());
  return BIC_OK;
}

int bic_pbm_unpack(bic_ctx* ctx, const uint8_t* raster, size_t rows, size_t cols, uint64_t* plane, size_t wpr) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (!geom_ok(rows, cols, wpr) || (rows && (!raster || !plane))) return BIC_EINVAL;
  timed(ctx, "pbm_unpack", [&] {
    bic::launch_pbm(ctx->cur, false, raster, nullptr, nullptr, plane, (uint32_t)rows, (uint32_t)cols, (uint32_t)wpr);
  });
  BIC_HIP(hipGetLastError());
  return BIC_OK;
}

int bic_pbm_pack(bic_ctx* ctx, const uint64_t* plane, size_t rows, size_t cols, size_t wpr, uint8_t* raster) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (!geom_ok(rows, cols, wpr) || (rows && (!raster || !plane))) return BIC_EINVAL;
  timed(ctx, "pbm_pack", [&] {
    bic::launch_pbm(ctx->cur, true, nullptr, raster, plane, nullptr, (uint32_t)rows, (uint32_t)cols, (uint32_t)wpr);
  });
  BIC_HIP(hipGetLastError());
  return BIC_OK;
}

int bic_planes_to_gray(bic_ctx* ctx, const uint64_t* planes, int plane0, int nplanes, size_t rows, size_t cols,
                       size_t wpr, int sample_bytes, void* gray, size_t pitch) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((sample_bytes != 1 && sample_bytes != 2) || plane0 < 0 || nplanes < 1 || plane0 + nplanes > 8 * sample_bytes)
    return BIC_EINVAL;
  if (!geom_ok(rows, cols, wpr) || pitch < cols * (size_t)sample_bytes || (rows && (!planes || !gray)))
    return BIC_EINVAL;
  if (rows == 0) return BIC_OK;
  timed(ctx, "planes_to_gray", [&] {
    bic::launch_planes_gray(ctx->cur, planes, (uint32_t)rows, (uint32_t)cols, (uint32_t)wpr, plane0, nplanes,
                            sample_bytes, static_cast<uint8_t*>(gray), (uint64_t)pitch, ctx->gray_code);
  });
  if (sample_bytes == 1 && ctx->sample_predict)  // the z samples just stored -> the samples, in place
    timed(ctx, "sample_unpredict", [&] {
      bic::launch_sample_unpredict(ctx->cur, ctx->sample_predict, static_cast<uint8_t*>(gray), (uint64_t)pitch, 0, 1,
                                   (uint32_t)rows, (uint32_t)cols);
    });
  BIC_HIP(hipGetLastError());
  return BIC_OK;
}

int bic_bitplanes_rgb(bic_ctx* ctx, const uint8_t* rgb, size_t pitch, size_t rows, size_t cols, int plane0, int nplanes,
                      uint64_t* planes, size_t wpr) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (plane0 < 0 || nplanes < 1 || plane0 + nplanes > 8 || cols > SIZE_MAX / 4 || pitch < 3 * cols ||
      (rows && (!rgb || !planes)))
    return BIC_EINVAL;
  if (!geom_ok(rows, cols, wpr)) return BIC_EINVAL;
  if (rows == 0) return BIC_OK;
  timed(ctx, "bitplanes_rgb", [&] {
    bic::launch_raster_planes(ctx->cur, rgb, 3, (uint32_t)rows, (uint32_t)cols, plane0, nplanes, planes, (uint32_t)wpr,
                              (uint64_t)pitch, 0, ctx->gray_code, ctx->color_transform, ctx->rgb_predict);
  });
  BIC_HIP(hipGetLastError());
  return BIC_OK;
}

int bic_planes_to_rgb(bic_ctx* ctx, const uint64_t* planes, int plane0, int nplanes, size_t rows, size_t cols,
                      size_t wpr, uint8_t* rgb, size_t pitch) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (plane0 < 0 || nplanes < 1 || plane0 + nplanes > 8) return BIC_EINVAL;
  if (!geom_ok(rows, cols, wpr) || cols > SIZE_MAX / 4 || pitch < 3 * cols || (rows && (!planes || !rgb)))
    return BIC_EINVAL;
  if (rows == 0) return BIC_OK;
  timed(ctx, "planes_to_rgb", [&] {
    bic::launch_planes_gray(ctx->cur, planes, (uint32_t)rows, (uint32_t)cols, (uint32_t)wpr, plane0, nplanes, 3, rgb,
                            (uint64_t)pitch, ctx->gray_code, ctx->rgb_predict ? 0 : ctx->color_transform);
  });
  if (ctx->rgb_predict)  // the z bytes just stored -> the pixels, in place (the inverse colour transform behind the scan)
    timed(ctx, "rgb_unpredict", [&] {
      bic::launch_rgb_unpredict(ctx->cur, ctx->rgb_predict, ctx->color_transform, rgb, (uint64_t)pitch, 0, 1,
                                (uint32_t)rows, (uint32_t)cols);
    });
  BIC_HIP(hipGetLastError());
  return BIC_OK;
}

int bic_pgm_bitplanes(bic_ctx* ctx, const uint8_t* raster, size_t rows, size_t cols, int maxval, int plane0,
                      int nplanes, uint64_t* planes, size_t wpr) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (maxval < 1 || maxval > 65535 || plane0 < 0 || nplanes < 1 || plane0 + nplanes > (maxval < 256 ? 8 : 16))
    return BIC_EINVAL;
  if (!geom_ok(rows, cols, wpr) || (rows && (!raster || !planes))) return BIC_EINVAL;
  if (rows == 0) return BIC_OK;
  timed(ctx, "pgm_bitplanes", [&] {
    bic::launch_raster_planes(ctx->cur, raster, maxval < 256 ? 1 : 2, (uint32_t)rows, (uint32_t)cols, plane0, nplanes,
                              planes, (uint32_t)wpr, 0, 1, ctx->gray_code, 0, maxval < 256 ? ctx->sample_predict : 0);
  });
  BIC_HIP(hipGetLastError());
  return BIC_OK;
}

}  // extern "C"
