// bic_capi.cpp -- the C ABI of include/bic.h: argument validation (the reference's asserts
// become BIC_EINVAL), the per-device context (bic_ctx.h: stream, scratch arena, deferred-error flags)
// and the launch sequences, one file per family: bic_capi_rows.cpp (the row encoders),
// bic_capi_decode.cpp, bic_capi_tiles.cpp (samples, tiles, match), bic_capi_raster.cpp,
// bic_capi_algebra.cpp (GF(2), dictionary learning). This file: the context itself, its options and
// profiling, and the entries that need no device. Compiled with hipcc for gfx950; no CPU fallback
// exists: without a gfx950 device every entry point fails with BIC_ENODEV.
#include "bic_ctx.h"

#include <cctype>
#include <cmath>
#include <map>
#include <new>

#ifdef BIC_STAMPS
namespace bic {
int read_stamps(uint64_t* host, size_t n);
int read_match_stamps(uint64_t* host, size_t n);
}
#endif

namespace {

// the context's stream, byte tables and error flags
int ctx_init(bic_ctx* ctx) {
  if (hipStreamCreateWithFlags(&ctx->own, hipStreamNonBlocking) != hipSuccess) return BIC_EDEVICE;
  ctx->cur = ctx->own;
  uint64_t host_lut[bic::kLutWords];
  bic::build_byte_lut(host_lut);
  bic::egad_build_nib(host_lut + bic::kLutEgadNib);
  bic::egad_build_dec_nib(host_lut + bic::kLutEgadDec);
  if (hipMalloc(&ctx->lut, sizeof(host_lut)) != hipSuccess ||
      hipMemcpy(ctx->lut, host_lut, sizeof(host_lut), hipMemcpyHostToDevice) != hipSuccess)
    return BIC_ENOMEM;
  if (hipMalloc(&ctx->flags, 4 * sizeof(uint32_t)) != hipSuccess ||
      hipMemset(ctx->flags, 0, 4 * sizeof(uint32_t)) != hipSuccess)
    return BIC_ENOMEM;
  return BIC_OK;
}

// whatever the context holds, and the context
void ctx_release(bic_ctx* ctx) {
  for (auto& r : ctx->recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
  for (auto e : ctx->pool) (void)hipEventDestroy(e);
  if (ctx->scratch) (void)hipFree(ctx->scratch);
  if (ctx->flags) (void)hipFree(ctx->flags);
  ctx->enuml.release();
  if (ctx->lut) (void)hipFree(ctx->lut);
  if (ctx->rbuf) (void)hipFree(ctx->rbuf);
  ctx->lentab.release();
  if (ctx->own) (void)hipStreamDestroy(ctx->own);
  if (ctx->aux) (void)hipStreamDestroy(ctx->aux);
  if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
  if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
  delete ctx;
}

// pnm.cpp:5-18 skip_comments on a byte buffer: whitespace, then a '#' line (fgets into a 100-byte
// buffer: at most 99 bytes, through the newline) and again
void pnm_skip_comments(const uint8_t* b, size_t n, size_t& i) {
  for (;;) {
    while (i < n && std::isspace(b[i])) ++i;
    if (i >= n || b[i] != '#') return;
    ++i;  // the '#' (fgetc), then fgets' at most 99 bytes
    size_t k = 0;
    while (i < n && k < 99) {
      const uint8_t c = b[i++];
      ++k;
      if (c == '\n') break;
    }
  }
}
// fscanf("%d"): leading whitespace, an optional sign, digits
bool pnm_int(const uint8_t* b, size_t n, size_t& i, long long& v) {
  while (i < n && std::isspace(b[i])) ++i;
  bool neg = false;
  if (i < n && (b[i] == '+' || b[i] == '-')) neg = b[i++] == '-';
  if (i >= n || !std::isdigit(b[i])) return false;
  v = 0;
  while (i < n && std::isdigit(b[i])) {
    v = v * 10 + (b[i++] - '0');
    if (v > 0x7fffffffLL) return false;
  }
  if (neg) v = -v;
  return true;
}

}  // namespace

extern "C" {

const char* bic_strerror(int code) {
  switch (code) {
    case BIC_OK: return "ok";
    case BIC_EINVAL: return "invalid argument";
    case BIC_ENOMEM: return "device allocation failed";
    case BIC_EDEVICE: return "HIP runtime error";
    case BIC_ENOSPC: return "output slot too small";
    case BIC_ENODEV: return "no gfx950 device";
    case BIC_EDATA: return "malformed stream";
    default: return "unknown error";
  }
}

int bic_device_count(int* n) {
  if (!n) return BIC_EINVAL;
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
  *n = c;
  return BIC_OK;
}

int bic_ctx_create(int device, bic_ctx** out) {
  if (!out) return BIC_EINVAL;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return BIC_ENODEV;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return BIC_EDEVICE;
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return BIC_ENODEV;  // built for gfx950 only
  BIC_HIP(hipSetDevice(device));
  bic_ctx* ctx = new (std::nothrow) bic_ctx();
  if (!ctx) return BIC_ENOMEM;
  ctx->device = device;
  const int rc = ctx_init(ctx);
  if (rc) {
    ctx_release(ctx);
    return rc;
  }
  *out = ctx;
  return BIC_OK;
}

int bic_ctx_destroy(bic_ctx* ctx) {
  if (!ctx) return BIC_EINVAL;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->cur);
  ctx_release(ctx);
  return BIC_OK;
}

int bic_ctx_set_stream(bic_ctx* ctx, void* hip_stream) {
  if (!ctx) return BIC_EINVAL;
  ctx->cur = reinterpret_cast<hipStream_t>(hip_stream);  // NULL = the HIP null stream
  return BIC_OK;
}

void* bic_ctx_own_stream(bic_ctx* ctx) { return ctx ? reinterpret_cast<void*>(ctx->own) : nullptr; }

void* bic_ctx_get_stream(bic_ctx* ctx) { return ctx ? reinterpret_cast<void*>(ctx->cur) : nullptr; }

int bic_sync(bic_ctx* ctx) {
  int rc = bind(ctx);
  if (rc) return rc;
  BIC_HIP(hipStreamSynchronize(ctx->cur));
  BIC_HIP(hipGetLastError());
  uint32_t f[4] = {0, 0, 0, 0};
  BIC_HIP(hipMemcpy(f, ctx->flags, sizeof(f), hipMemcpyDeviceToHost));
  if (f[0] || f[1] || f[2] || f[3]) BIC_HIP(hipMemset(ctx->flags, 0, sizeof(f)));
  if (f[2] || f[3])
    hip_fail(hipSuccess, __FILE_NAME__, __LINE__, f[2] ? "look-back record flag" : "length disagreement flag");
  if (f[2]) return BIC_EDEVICE;  // a look-back record never arrived (should not happen)
  if (f[3]) return BIC_EDEVICE;  // the row encoder's length pass disagreed with its emission (a bug)
  if (f[1] & 2u) return BIC_EDATA;  // a decoder met a malformed stream
  if (f[1]) return BIC_EINVAL;
  if (f[0]) return BIC_ENOSPC;
  return BIC_OK;
}

int bic_reserve(bic_ctx* ctx, int nplanes, size_t rows, size_t cols) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (nplanes < 1 || !geom_ok(rows, cols, (cols + 63) / 64)) return BIC_EINVAL;
  const bic::Geom g = bic::make_geom(rows, cols, (cols + 63) / 64, nplanes);
  return ensure_scratch(ctx, bic::chunk_scratch_bytes(g));
}

int bic_malloc(bic_ctx* ctx, size_t bytes, void** dptr) {
  if (!dptr) return BIC_EINVAL;
  *dptr = nullptr;
  int rc = bind(ctx);
  if (rc) return rc;
  if (bytes == 0) return BIC_OK;
  return hipMalloc(dptr, bytes) == hipSuccess ? BIC_OK : BIC_ENOMEM;
}

int bic_free(bic_ctx* ctx, void* dptr) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (dptr) BIC_HIP(hipFree(dptr));
  return BIC_OK;
}

int bic_memcpy_h2d(bic_ctx* ctx, void* dst, const void* src, size_t bytes) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (bytes == 0) return BIC_OK;
  if (!dst || !src) return BIC_EINVAL;
  BIC_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->cur));
  BIC_HIP(hipStreamSynchronize(ctx->cur));
  return BIC_OK;
}

int bic_memcpy_d2h(bic_ctx* ctx, void* dst, const void* src, size_t bytes) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (bytes == 0) return BIC_OK;
  if (!dst || !src) return BIC_EINVAL;
  BIC_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->cur));
  BIC_HIP(hipStreamSynchronize(ctx->cur));
  return BIC_OK;
}

int bic_memset(bic_ctx* ctx, void* dst, int value, size_t bytes) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (bytes == 0) return BIC_OK;
  if (!dst) return BIC_EINVAL;
  BIC_HIP((bic::launch_fill(ctx->cur, dst, value, bytes), hipGetLastError()));
  return BIC_OK;
}

int bic_ctx_set_option(bic_ctx* ctx, int option, long value) {
  if (!ctx) return BIC_EINVAL;
  switch (option) {
    case BIC_OPT_MULTIPASS: ctx->force_multipass = value != 0; return BIC_OK;
    case BIC_OPT_TWO_PASS: ctx->two_pass = value != 0; return BIC_OK;
    case BIC_OPT_SINGLE_KERNEL: ctx->single_kernel = value != 0; return BIC_OK;
    case BIC_OPT_STAGED: ctx->force_staged = value != 0; return BIC_OK;
    case BIC_OPT_ONE_STREAM: ctx->one_stream = value != 0; return BIC_OK;
    case BIC_OPT_EG_SOURCE:
      ctx->eg_src_off = value == 0;
      ctx->eg_src_one = value == 2;
      return BIC_OK;
    case BIC_OPT_GRAY_CODE:
      if (value != 0 && value != 1) return BIC_EINVAL;  // (the setting stays as it was)
      ctx->gray_code = value == 1;
      return BIC_OK;
    case BIC_OPT_COLOR_TRANSFORM:
      if (value < BIC_CT_NONE || value > BIC_CT_SUBTRACT_GREEN_FOLDED) return BIC_EINVAL;  // (likewise)
      ctx->color_transform = (int)value;
      return BIC_OK;
    case BIC_OPT_SAMPLE_PREDICT:
      if (value < BIC_SP_NONE || value > BIC_SP_LEFT_FOLDED) return BIC_EINVAL;  // (likewise)
      ctx->sample_predict = (int)value;
      return BIC_OK;
    case BIC_OPT_RGB_PREDICT:
      if (value < BIC_SP_NONE || value > BIC_SP_LEFT_FOLDED) return BIC_EINVAL;  // (likewise)
      ctx->rgb_predict = (int)value;
      return BIC_OK;
    default: return BIC_EINVAL;
  }
}

size_t bic_encode_slot_words(size_t rows, size_t cols, int coder) {
  const unsigned long long base = (unsigned long long)rows * (cols + 1);
  if (coder == BIC_CODER_EG) return (size_t)((base + 1 + 63) / 64);
  return (size_t)((2 * base + 63) / 64 + 64);
}

int bic_rgb_p00(int color_transform, int gray_code, const uint8_t pixel[3], int plane0, int nplanes, uint8_t* p00) {
  return bic_rgb_p00_predict(color_transform, BIC_SP_NONE, gray_code, pixel, plane0, nplanes, p00);
}

int bic_rgb_p00_predict(int color_transform, int rgb_predict, int gray_code, const uint8_t pixel[3], int plane0,
                        int nplanes, uint8_t* p00) {
  if (color_transform < BIC_CT_NONE || color_transform > BIC_CT_SUBTRACT_GREEN_FOLDED || rgb_predict < BIC_SP_NONE ||
      rgb_predict > BIC_SP_LEFT_FOLDED || (gray_code != 0 && gray_code != 1) || !pixel || !p00 || plane0 < 0 ||
      nplanes < 1 || plane0 + nplanes > 8)
    return BIC_EINVAL;
  for (int c = 0; c < 3; ++c) {
    uint32_t v = pixel[c];
    if (c != 1 && color_transform != BIC_CT_NONE) {
      v = (v - pixel[1]) & 0xffu;
      if (color_transform == BIC_CT_SUBTRACT_GREEN_FOLDED) v = ((v << 1) ^ (v & 0x80u ? 0xffu : 0u)) & 0xffu;
    }
    // (no left neighbour: the transformed sample is its own difference)
    if (rgb_predict == BIC_SP_LEFT_FOLDED) v = ((v << 1) ^ (v & 0x80u ? 0xffu : 0u)) & 0xffu;
    if (gray_code) v ^= v >> 1;
    for (int k = 0; k < nplanes; ++k) p00[c * nplanes + k] = (uint8_t)((v >> (plane0 + k)) & 1u);
  }
  return BIC_OK;
}

int bic_gray_p00(int sample_predict, int gray_code, uint8_t sample, int plane0, int nplanes, uint8_t* p00) {
  if (sample_predict < BIC_SP_NONE || sample_predict > BIC_SP_LEFT_FOLDED || (gray_code != 0 && gray_code != 1) || !p00 ||
      plane0 < 0 || nplanes < 1 || plane0 + nplanes > 8)
    return BIC_EINVAL;
  uint32_t v = sample;  // (no left neighbour: the sample is its own difference)
  if (sample_predict == BIC_SP_LEFT_FOLDED) v = ((v << 1) ^ (v & 0x80u ? 0xffu : 0u)) & 0xffu;
  if (gray_code) v ^= v >> 1;
  for (int k = 0; k < nplanes; ++k) p00[k] = (uint8_t)((v >> (plane0 + k)) & 1u);
  return BIC_OK;
}

int bic_pnm_parse_header(const uint8_t* bytes, size_t n, bic_pnm_info* info) {
  if (!bytes || !info || n < 2 || bytes[0] != 'P') return BIC_EINVAL;
  size_t i = 2;
  long long w = 0, h = 0, mv = 1;
  const int type = bytes[1] - '0';
  if (type == 4) {  // pbm.cpp:4-27: " %d" then " %d " (which also eats whitespace-valued raster bytes)
    if (!pnm_int(bytes, n, i, w) || !pnm_int(bytes, n, i, h) || w <= 0 || h <= 0) return BIC_EINVAL;
    while (i < n && std::isspace(bytes[i])) ++i;
  } else if (type == 2 || type == 5 || type == 6) {  // pnm.cpp:20-42
    pnm_skip_comments(bytes, n, i);
    if (!pnm_int(bytes, n, i, w)) return BIC_EINVAL;
    pnm_skip_comments(bytes, n, i);
    if (!pnm_int(bytes, n, i, h)) return BIC_EINVAL;
    pnm_skip_comments(bytes, n, i);
    if (!pnm_int(bytes, n, i, mv)) return BIC_EINVAL;
    if (w <= 0 || h <= 0 || mv <= 0 || mv > 65535) return BIC_EINVAL;
    ++i;  // the fgetc after maxval
  } else {
    return BIC_EINVAL;
  }
  if (i > n) return BIC_EINVAL;
  info->type = type;
  info->cols = (size_t)w;
  info->rows = (size_t)h;
  info->maxval = (int)mv;
  info->data_offset = i;
  return BIC_OK;
}

// log2 C(n, r): the reference's enumL / enumerative_codelength (coding.cpp:19-22,
// compress7_test.cpp:25-28) without GSL. Exact at r in {0, n} (0) and, for power-of-two n,
// at r in {1, n-1} (log2 n -- where GSL's last-ulp rounding is unpinned, SURVEY.md §8 c);
// long-double lgamma elsewhere.
double bic_enum_codelength(unsigned n, unsigned r) {
  if (r == 0 || r >= n) return 0.0;
  const unsigned m = r * 2 > n ? n - r : r;
  if (m == 1) {
    if ((n & (n - 1)) == 0) {
      unsigned e = 0;
      while ((1u << e) < n) ++e;
      return (double)e;
    }
    return (double)std::log2((long double)n);
  }
  const long double ln = std::lgamma((long double)n + 1.0L) - std::lgamma((long double)m + 1.0L) -
                         std::lgamma((long double)(n - m) + 1.0L);
  return (double)(ln * 1.442695040888963407359924681001892137L);
}

int bic_tile_lentab(unsigned W, uint64_t* lentab) {
  if (W < 1 || W > 64 || !lentab) return BIC_EINVAL;
  const unsigned M = W * W;
  for (unsigned w = 0; w <= M; ++w)  // compress7_test.cpp:220-221: (idx_t)(1 + 1 + enumL(M, w))
    lentab[w] = (uint64_t)(2.0 + bic_enum_codelength(M, w));
  return BIC_OK;
}

int bic_prof_enable(bic_ctx* ctx, int on) {
  if (!ctx) return BIC_EINVAL;
  ctx->prof_on = on != 0;
  return BIC_OK;
}

int bic_prof_only(bic_ctx* ctx, const char* name) {
  if (!ctx) return BIC_EINVAL;
  ctx->prof_only = name ? name : "";
  return BIC_OK;
}

int bic_prof_collect(bic_ctx* ctx, char* buf, size_t cap) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (!buf || cap == 0) return BIC_EINVAL;
  BIC_HIP(hipStreamSynchronize(ctx->cur));
  std::map<std::string, std::pair<unsigned long, double>> agg;
  for (auto& r : ctx->recs) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) ms = -1.f;
    auto& e = agg[r.name];
    e.first += 1;
    e.second += ms;
    ctx->pool.push_back(r.a);
    ctx->pool.push_back(r.b);
  }
  ctx->recs.clear();
  (void)hipGetLastError();  // a failed elapsed-time query (-1 above) must not fail the next call
  std::string outs;
  for (auto& kv : agg) {
    char line[160];
    std::snprintf(line, sizeof line, "%s %lu %.6f\n", kv.first.c_str(), kv.second.first, kv.second.second);
    outs += line;
  }
  std::snprintf(buf, cap, "%s", outs.c_str());
  return outs.size() < cap ? BIC_OK : BIC_ENOSPC;
}

#ifdef BIC_STAMPS
int bic_debug_stamps(uint64_t* host, size_t n) { return bic::read_stamps(host, n); }
int bic_debug_match_stamps(uint64_t* host, size_t n) { return bic::read_match_stamps(host, n); }
#endif

}  // extern "C"
