// bic_capi_decode.cpp -- the decoders' entry points (bic_decode.hip): streams to planes, to gray or RGB samples,
// to P4 rasters. They differ in their sink alone.
#include "bic_ctx.h"

namespace {

// The stream arguments every decoder takes, checked and put into c. BIC_OK with c.rows == 0: nothing
// to decode, the pointers (`sink` = where the entry's output goes) unchecked.
int stream_call(bic::DecodeCall& c, int coder, const uint64_t* streams, size_t slot_words, const uint64_t* word_off,
                const uint64_t* plane_bits, const uint64_t* index, int nplanes, size_t rows, size_t cols, size_t wpr,
                int predict, const uint8_t* p00, const void* sink) {
  if (coder != BIC_CODER_GOLOMB && coder != BIC_CODER_EG && coder != BIC_CODER_EG_ADAPTIVE) return BIC_EINVAL;
  if (nplanes < 1 || !geom_ok(rows, cols, wpr) || !bic::decode_supported((uint32_t)cols)) return BIC_EINVAL;
  c.rows = (uint32_t)rows;
  if (rows == 0) return BIC_OK;
  if (!streams || !plane_bits || !sink || (slot_words == 0 && !word_off)) return BIC_EINVAL;
  if (coder != BIC_CODER_EG && !index) return BIC_EINVAL;  // the two coders whose rows start from an index
  c.coder = coder == BIC_CODER_GOLOMB ? 0 : coder == BIC_CODER_EG ? 1 : 2;
  c.streams = streams;
  c.slot = slot_words;
  c.word_off = word_off;
  c.plane_bits = plane_bits;
  c.index = index;
  c.p00 = p00;
  c.cols = (uint32_t)cols;
  c.wpr = (uint32_t)wpr;
  c.nplanes = (uint32_t)nplanes;
  c.predict = predict ? 1 : 0;
  return BIC_OK;
}

int run_decode(bic_ctx* ctx, const char* name, bic::DecodeCall& c) {
  const int rc = ensure_scratch(ctx, bic::decode_scratch_bytes(c));
  if (rc) return rc;
  c.scratch = ctx->scratch;
  c.flags = ctx->flags;
  c.egnib = ctx->lut + bic::kLutEgadDec;
  timed(ctx, name, [&] { bic::launch_decode(ctx->cur, c); });
  if (c.sink == bic::DecodeCall::kGray && c.gray.sample_predict)  // the z samples just stored -> the samples, in place
    timed(ctx, "sample_unpredict", [&] {
      bic::launch_sample_unpredict(ctx->cur, c.gray.sample_predict, c.gray.gray, c.gray.pitch, c.gray.frame_stride,
                                   c.gray.nframes, c.rows, c.cols);
    });
  if (c.sink == bic::DecodeCall::kRgb && c.rgb.rgb_predict)  // the z bytes just stored -> the pixels, in place
    timed(ctx, "rgb_unpredict", [&] {
      bic::launch_rgb_unpredict(ctx->cur, c.rgb.rgb_predict, c.rgb.ct_inverse, c.rgb.rgb, c.rgb.pitch, c.rgb.frame_stride,
                                c.rgb.nframes, c.rows, c.cols);
    });
  BIC_HIP(hipGetLastError());
  return BIC_OK;
}

}  // namespace

extern "C" {

int bic_decode_planes(bic_ctx* ctx, int coder, const uint64_t* streams, size_t slot_words, const uint64_t* word_off,
                      const uint64_t* plane_bits, const uint64_t* index, int nplanes, size_t rows, size_t cols,
                      size_t wpr, int predict, const uint8_t* p00, uint64_t* planes) {
  int rc = bind(ctx);
  if (rc) return rc;
  bic::DecodeCall c{};
  if ((rc = stream_call(c, coder, streams, slot_words, word_off, plane_bits, index, nplanes, rows, cols, wpr, predict,
                        p00, planes)) || !c.rows)
    return rc;
  c.sink = bic::DecodeCall::kPlanes;
  c.planes = planes;
  return run_decode(ctx, "decode", c);
}

int bic_decode_gray(bic_ctx* ctx, int coder, const uint64_t* streams, size_t slot_words, const uint64_t* word_off,
                    const uint64_t* plane_bits, const uint64_t* index, int plane0, int nplanes, size_t rows, size_t cols,
                    int predict, const uint8_t* p00, int sample_bytes, int big_endian, void* gray, size_t pitch) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((sample_bytes != 1 && sample_bytes != 2) || plane0 < 0 || nplanes < 1 || plane0 + nplanes > 8 * sample_bytes ||
      pitch < cols * (size_t)sample_bytes)
    return BIC_EINVAL;
  bic::DecodeCall c{};
  if ((rc = stream_call(c, coder, streams, slot_words, word_off, plane_bits, index, nplanes, rows, cols,
                        (cols + 63) / 64, predict, p00, gray)) || !c.rows)
    return rc;
  c.sink = bic::DecodeCall::kGray;
  c.gray = {static_cast<uint8_t*>(gray), (uint64_t)pitch, plane0, sample_bytes, sample_bytes == 2 && big_endian ? 1 : 0,
            ctx->gray_code ? 1 : 0};
  c.gray.sample_predict = sample_bytes == 1 ? ctx->sample_predict : 0;
  return run_decode(ctx, "decode_gray", c);
}

int bic_decode_gray_frames(bic_ctx* ctx, int coder, const uint64_t* streams, size_t slot_words, const uint64_t* word_off,
                           const uint64_t* plane_bits, const uint64_t* index, int nframes, int plane0, int nplanes,
                           size_t rows, size_t cols, int predict, const uint8_t* p00, int sample_bytes, int big_endian,
                           void* gray, size_t pitch, size_t frame_stride) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((sample_bytes != 1 && sample_bytes != 2) || plane0 < 0 || nplanes < 1 || plane0 + nplanes > 8 * sample_bytes ||
      nframes < 1 || (uint64_t)nframes * (uint64_t)nplanes > 65535 || cols > SIZE_MAX / 4 ||
      pitch < cols * (size_t)sample_bytes)
    return BIC_EINVAL;
  if (nframes > 1 && pitch && (rows > SIZE_MAX / pitch || frame_stride < rows * pitch)) return BIC_EINVAL;
  bic::DecodeCall c{};
  if ((rc = stream_call(c, coder, streams, slot_words, word_off, plane_bits, index, nframes * nplanes, rows, cols,
                        (cols + 63) / 64, predict, p00, gray)) || !c.rows)
    return rc;
  c.sink = bic::DecodeCall::kGray;
  c.gray = {static_cast<uint8_t*>(gray), (uint64_t)pitch, plane0, sample_bytes, sample_bytes == 2 && big_endian ? 1 : 0,
            ctx->gray_code ? 1 : 0, (uint32_t)nframes, nframes > 1 ? (uint64_t)frame_stride : 0};
  c.gray.sample_predict = sample_bytes == 1 ? ctx->sample_predict : 0;
  return run_decode(ctx, "decode_gray_frames", c);
}

int bic_decode_rgb(bic_ctx* ctx, int coder, const uint64_t* streams, size_t slot_words, const uint64_t* word_off,
                   const uint64_t* plane_bits, const uint64_t* index, int plane0, int nplanes, size_t rows, size_t cols,
                   int predict, const uint8_t* p00, uint8_t* rgb, size_t pitch) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (plane0 < 0 || nplanes < 1 || plane0 + nplanes > 8 || cols > SIZE_MAX / 4 || pitch < 3 * cols) return BIC_EINVAL;
  bic::DecodeCall c{};
  if ((rc = stream_call(c, coder, streams, slot_words, word_off, plane_bits, index, 3 * nplanes, rows, cols,
                        (cols + 63) / 64, predict, p00, rgb)) || !c.rows)
    return rc;
  c.sink = bic::DecodeCall::kRgb;
  // (BIC_OPT_RGB_PREDICT: the sink stores the z bytes, the inverse colour transform follows the scan)
  c.rgb = {rgb, (uint64_t)pitch, plane0, ctx->gray_code ? 1 : 0, ctx->rgb_predict ? 0 : ctx->color_transform};
  c.rgb.rgb_predict = ctx->rgb_predict;
  c.rgb.ct_inverse = ctx->color_transform;
  return run_decode(ctx, "decode_rgb", c);
}

int bic_decode_rgb_frames(bic_ctx* ctx, int coder, const uint64_t* streams, size_t slot_words, const uint64_t* word_off,
                          const uint64_t* plane_bits, const uint64_t* index, int nframes, int plane0, int nplanes,
                          size_t rows, size_t cols, int predict, const uint8_t* p00, uint8_t* rgb, size_t pitch,
                          size_t frame_stride) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (plane0 < 0 || nplanes < 1 || plane0 + nplanes > 8 || nframes < 1 ||
      (uint64_t)nframes * 3u * (uint64_t)nplanes > 65535 || cols > SIZE_MAX / 4 || pitch < 3 * cols)
    return BIC_EINVAL;
  if (nframes > 1 && pitch && (rows > SIZE_MAX / pitch || frame_stride < rows * pitch)) return BIC_EINVAL;
  bic::DecodeCall c{};
  if ((rc = stream_call(c, coder, streams, slot_words, word_off, plane_bits, index, nframes * 3 * nplanes, rows, cols,
                        (cols + 63) / 64, predict, p00, rgb)) || !c.rows)
    return rc;
  c.sink = bic::DecodeCall::kRgb;
  c.rgb = {rgb, (uint64_t)pitch, plane0, ctx->gray_code ? 1 : 0, ctx->rgb_predict ? 0 : ctx->color_transform,
           (uint32_t)nframes, nframes > 1 ? (uint64_t)frame_stride : 0};
  c.rgb.rgb_predict = ctx->rgb_predict;
  c.rgb.ct_inverse = ctx->color_transform;
  return run_decode(ctx, "decode_rgb_frames", c);
}

int bic_decode_pbm(bic_ctx* ctx, int coder, const uint64_t* streams, size_t slot_words, const uint64_t* word_off,
                   const uint64_t* plane_bits, const uint64_t* index, int nframes, size_t rows, size_t cols, int predict,
                   const uint8_t* p00, uint8_t* raster, size_t frame_stride) {
  int rc = bind(ctx);
  if (rc) return rc;
  bic::DecodeCall c{};
  if ((rc = stream_call(c, coder, streams, slot_words, word_off, plane_bits, index, nframes, rows, cols,
                        (cols + 63) / 64, predict, p00, raster)))
    return rc;
  const size_t frame_bytes = rows * ((cols + 7) / 8);
  if (nframes == 1) frame_stride = frame_bytes;  // (one frame: the stride is not read)
  else if (frame_stride < frame_bytes) return BIC_EINVAL;
  if (!c.rows) return BIC_OK;
  c.sink = bic::DecodeCall::kPbm;
  c.pbm = {raster, (uint64_t)frame_stride};
  return run_decode(ctx, "decode_pbm", c);
}

}  // extern "C"
