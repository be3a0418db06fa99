// gpu.cpp -- bic::Device (include/bic_gpu.h): the reference C++ API's planes handed to the
// HIP kernels through the C ABI (bic.h). This file only moves data and bookkeeping; every
// pixel-level operation runs in the kernels.
#include "bic_gpu.h"
#include "bsvd.h"

#include <cstdio>
#include <cstdlib>
#include <iostream>

namespace bic {

namespace {
constexpr uint64_t kDomain = 0x80000000ull;  // the reference coders' 32-bit state stays exact below 2^31

bool same_shape(const binary_matrix& a, const binary_matrix& b) {
  return a.get_rows() == b.get_rows() && a.get_cols() == b.get_cols() &&
         a.get_blocks_per_row() == b.get_blocks_per_row() && (a.raw_blocks() || !a.get_rows());
}
}  // namespace

void coder_state::advance(GolombCoder& c, uint64_t n, uint64_t sum, uint64_t bits) {
  c.bitcount += (long)bits;
  if (n == 0) return;  // codeSample was never called: k keeps its value
  c.samples += (unsigned)n;
  c.accumulatedError += (unsigned)sum;
  unsigned k = 0;
  while ((c.samples << k) < c.accumulatedError) ++k;
  c.k = k;
}

void coder_state::advance(EGCoder& e, uint64_t ones, uint64_t bits) {
  e.bitcount += bits;
  if (ones) e.decBlockSize();  // every non-EOL run calls it; from a fresh coder one call is the fixpoint
}

int planes_for_maxval(int maxval) {
  int n = 0;
  for (long b = 1; b < maxval; b <<= 1) ++n;
  return n;
}

Device::Device(int ordinal) { status_ = bic_ctx_create(ordinal, &ctx_); }

Device::~Device() {
  if (!ctx_) return;
  for (Buf* b : {&in_, &out_a_, &out_b_, &small_, &aux_}) bic_free(ctx_, b->p);
  bic_ctx_destroy(ctx_);
}

int Device::ensure(Buf& b, size_t bytes) {
  if (b.cap >= bytes) return BIC_OK;
  int rc = bic_free(ctx_, b.p);
  b.p = nullptr;
  b.cap = 0;
  if (rc) return rc;
  const size_t want = bytes + bytes / 4 + 256;
  if ((rc = bic_malloc(ctx_, want, &b.p))) return rc;
  b.cap = want;
  return BIC_OK;
}

int Device::upload(const binary_matrix& M, uint64_t* dst) {
  return bic_memcpy_h2d(ctx_, dst, M.raw_blocks(), M.get_rows() * M.get_blocks_per_row() * sizeof(uint64_t));
}

int Device::download(uint64_t* src, binary_matrix& M) {
  return bic_memcpy_d2h(ctx_, M.raw_blocks(), src, M.get_rows() * M.get_blocks_per_row() * sizeof(uint64_t));
}

int Device::fetch_stream(const uint64_t* slot, uint64_t bits, Stream* s) {
  s->bits = bits;
  s->bytes.assign((bits + 7) / 8, 0);
  // slots hold big-endian words, so device bytes are already the stream's bytes
  return bic_memcpy_d2h(ctx_, s->bytes.data(), slot, s->bytes.size());
}

#define BIC_TRY(x)            \
  do {                        \
    const int rc_ = (x);      \
    if (rc_) return rc_;      \
  } while (0)

int Device::bitplanes(const pixel_t* gray, idx_t rows, idx_t cols, int nplanes, binary_matrix* planes) {
  BIC_TRY(status_);
  if (nplanes < 1 || nplanes > 32 || !planes || (!gray && rows && cols)) return BIC_EINVAL;
  for (int p = 0; p < nplanes; ++p)
    if (planes[p].get_rows() != rows || planes[p].get_cols() != cols || (rows && !planes[p].raw_blocks()))
      return BIC_EINVAL;
  if (rows == 0 || cols == 0) return BIC_OK;
  const idx_t wpr = planes[0].get_blocks_per_row();
  const size_t pixels = rows * cols, plane_words = rows * wpr;
  BIC_TRY(ensure(in_, pixels));
  BIC_TRY(ensure(out_a_, 8 * plane_words * sizeof(uint64_t)));
  std::vector<uint8_t> bytes(pixels);
  // the kernel reads one byte per pixel: byte b of every pixel feeds planes 8b .. 8b+7
  for (int b = 0; 8 * b < nplanes; ++b) {
    const int nb = nplanes - 8 * b < 8 ? nplanes - 8 * b : 8;
    for (size_t i = 0; i < pixels; ++i) bytes[i] = (uint8_t)(gray[i] >> (8 * b));
    BIC_TRY(bic_memcpy_h2d(ctx_, in_.p, bytes.data(), pixels));
    uint64_t* dev = static_cast<uint64_t*>(out_a_.p);
    BIC_TRY(bic_bitplanes_u8(ctx_, static_cast<const uint8_t*>(in_.p), cols, rows, cols, nb, dev, wpr));
    BIC_TRY(bic_sync(ctx_));
    for (int q = 0; q < nb; ++q) BIC_TRY(download(dev + q * plane_words, planes[8 * b + q]));
  }
  return BIC_OK;
}

int Device::med(const binary_matrix& P, binary_matrix& R, idx_t* weight) {
  BIC_TRY(status_);
  if (!same_shape(P, R)) return BIC_EINVAL;
  const idx_t rows = P.get_rows(), cols = P.get_cols(), wpr = P.get_blocks_per_row();
  if (weight) *weight = 0;
  if (rows == 0 || cols == 0) return BIC_OK;
  const size_t words = rows * wpr;
  BIC_TRY(ensure(in_, words * 8));
  BIC_TRY(ensure(out_a_, words * 8));
  BIC_TRY(ensure(small_, 64));
  uint64_t* d_in = static_cast<uint64_t*>(in_.p);
  uint64_t* d_out = static_cast<uint64_t*>(out_a_.p);
  uint64_t* d_w = weight ? static_cast<uint64_t*>(small_.p) : nullptr;
  // one copy in, the kernel, one copy out: the copy back waits for the kernel (same stream) and
  // reports its errors, so a small call (compress7_test.cpp:205-206 calls med per tile) pays two
  // host round trips and no flag read (med raises none)
  BIC_TRY(upload(P, d_in));
  BIC_TRY(bic_med_residual(ctx_, d_in, 1, rows, cols, wpr, 1, d_out, d_w));
  // the reference writes neither R(0,0) nor R's pad bits (pred.cpp:5-13): keep R's
  const bool r00 = R.get(0, 0);
  std::vector<uint64_t> old_tail(rows);
  const idx_t used = cols % 64;
  const uint64_t pad = used ? ~(~0ull << (64 - used)) : 0;
  block_t* r = R.raw_blocks();
  for (idx_t i = 0; i < rows; ++i) old_tail[i] = r[i * wpr + wpr - 1] & pad;
  BIC_TRY(download(d_out, R));
  for (idx_t i = 0; i < rows; ++i) r[i * wpr + wpr - 1] = (r[i * wpr + wpr - 1] & ~pad) | old_tail[i];
  R.set(0, 0, r00);
  if (weight) {
    uint64_t w = 0;
    BIC_TRY(bic_memcpy_d2h(ctx_, &w, d_w, 8));
    *weight = w;
  }
  return BIC_OK;
}

int Device::encode(const binary_matrix* planes, int nplanes, bool predict, GolombCoder* golomb,
                   std::vector<Stream>* golomb_streams, EGCoder* eg, std::vector<Stream>* eg_streams) {
  BIC_TRY(status_);
  if (nplanes < 1 || !planes || (!golomb && !eg)) return BIC_EINVAL;
  for (int p = 0; p < nplanes; ++p) {
    if (!same_shape(planes[0], planes[p])) return BIC_EINVAL;
    if ((golomb && !coder_state::fresh(golomb[p])) || (eg && !coder_state::fresh(eg[p]))) return BIC_EINVAL;
  }
  const idx_t rows = planes[0].get_rows(), cols = planes[0].get_cols(), wpr = planes[0].get_blocks_per_row();
  if (golomb_streams) golomb_streams->assign(golomb ? nplanes : 0, Stream());
  if (eg_streams) eg_streams->assign(eg ? nplanes : 0, Stream());
  if (rows == 0 || cols == 0) return BIC_OK;
  const size_t plane_words = rows * wpr;
  const size_t slot_g = bic_encode_slot_words(rows, cols, BIC_CODER_GOLOMB);
  const size_t slot_e = bic_encode_slot_words(rows, cols, BIC_CODER_EG);
  BIC_TRY(ensure(in_, nplanes * plane_words * 8));
  if (golomb) BIC_TRY(ensure(out_a_, nplanes * slot_g * 8));
  if (eg) BIC_TRY(ensure(out_b_, nplanes * slot_e * 8));
  BIC_TRY(ensure(small_, 3 * nplanes * 8));
  uint64_t* d_in = static_cast<uint64_t*>(in_.p);
  uint64_t* d_bits = static_cast<uint64_t*>(small_.p);  // [golomb bits | eg bits | residual ones]
  for (int p = 0; p < nplanes; ++p) BIC_TRY(upload(planes[p], d_in + p * plane_words));
  uint64_t* d_g = golomb ? static_cast<uint64_t*>(out_a_.p) : nullptr;
  uint64_t* d_e = eg ? static_cast<uint64_t*>(out_b_.p) : nullptr;
  BIC_TRY(bic_encode_planes2(ctx_, d_in, nplanes, rows, cols, wpr, predict ? 1 : 0, d_g, slot_g,
                             golomb ? d_bits : nullptr, d_e, slot_e, eg ? d_bits + nplanes : nullptr));
  BIC_TRY(bic_med_residual(ctx_, d_in, nplanes, rows, cols, wpr, predict ? 1 : 0, nullptr, d_bits + 2 * nplanes));
  BIC_TRY(bic_sync(ctx_));
  std::vector<uint64_t> h(3 * nplanes);
  BIC_TRY(bic_memcpy_d2h(ctx_, h.data(), d_bits, h.size() * 8));
  for (int p = 0; p < nplanes; ++p) {
    const uint64_t ones = h[2 * nplanes + p];
    if (golomb) {
      // samples: one per 1 plus one per row; their sum is the number of zeros
      coder_state::advance(golomb[p], ones + rows, rows * cols - ones, h[p]);
      if (golomb_streams) BIC_TRY(fetch_stream(d_g + p * slot_g, h[p], &(*golomb_streams)[p]));
    }
    if (eg) {
      coder_state::advance(eg[p], ones, h[nplanes + p]);
      if (eg_streams) BIC_TRY(fetch_stream(d_e + p * slot_e, h[nplanes + p], &(*eg_streams)[p]));
    }
  }
  return BIC_OK;
}

int Device::code_samples(GolombCoder& coder, const unsigned* samples, size_t n, Stream* stream) {
  BIC_TRY(status_);
  if (!samples && n) return BIC_EINVAL;
  uint64_t total = 0;
  for (size_t i = 0; i < n; ++i) total += samples[i];
  const uint64_t n0 = coder_state::samples(coder), a0 = coder_state::accumulated(coder);
  if (n0 + n >= kDomain || a0 + total >= kDomain) return BIC_EINVAL;
  if (stream) *stream = Stream();
  if (n == 0) return BIC_OK;
  const size_t cap = (total + 33 * n + 63) / 64 + 1;  // k + 1 <= 33 and s >> k <= s per sample
  BIC_TRY(ensure(in_, n * 4));
  BIC_TRY(ensure(out_a_, cap * 8));
  BIC_TRY(ensure(small_, 16));
  uint64_t* d_bits = static_cast<uint64_t*>(small_.p);
  BIC_TRY(bic_memcpy_h2d(ctx_, in_.p, samples, n * 4));
  BIC_TRY(bic_golomb_encode_samples(ctx_, static_cast<const uint32_t*>(in_.p), n, n0, a0, 0,
                                    static_cast<uint64_t*>(out_a_.p), cap, d_bits));
  BIC_TRY(bic_sync(ctx_));
  uint64_t h[2];
  BIC_TRY(bic_memcpy_d2h(ctx_, h, d_bits, sizeof(h)));
  coder_state::advance(coder, n, h[1], h[0]);
  if (stream) BIC_TRY(fetch_stream(static_cast<uint64_t*>(out_a_.p), h[0], stream));
  return BIC_OK;
}

int Device::tiles(const binary_matrix& I, unsigned W, TileResult* out, const uint64_t* lentab,
                  binary_matrix* resid) {
  BIC_TRY(status_);
  const idx_t rows = I.get_rows(), cols = I.get_cols(), wpr = I.get_blocks_per_row();
  if (!out || W < 1 || W > 64 || rows % W || cols % W || (resid && !same_shape(I, *resid))) return BIC_EINVAL;
  std::vector<uint64_t> table;
  if (!lentab) {
    table.resize((size_t)W * W + 1);
    BIC_TRY(bic_tile_lentab(W, table.data()));
    lentab = table.data();
  }
  const size_t nt = (rows / W) * (cols / W);
  *out = TileResult();
  if (nt == 0) return BIC_OK;
  const size_t words = rows * wpr;
  const size_t cap = (rows * cols + 33 * nt + 63) / 64 + 1;  // chosen weights sum to <= rows*cols
  BIC_TRY(ensure(in_, words * 8));
  BIC_TRY(ensure(out_a_, cap * 8));
  BIC_TRY(ensure(out_b_, resid ? words * 8 : 8));
  BIC_TRY(ensure(aux_, nt * 13 + 64));
  BIC_TRY(ensure(small_, 24));
  uint32_t* d_w = static_cast<uint32_t*>(aux_.p);
  uint8_t* d_modes = reinterpret_cast<uint8_t*>(d_w + 3 * nt);
  uint64_t* d_stats = static_cast<uint64_t*>(small_.p);
  BIC_TRY(upload(I, static_cast<uint64_t*>(in_.p)));
  BIC_TRY(bic_patch_encode(ctx_, static_cast<const uint64_t*>(in_.p), rows, cols, wpr, W, lentab, d_w, d_w + nt,
                           d_w + 2 * nt, d_modes, resid ? static_cast<uint64_t*>(out_b_.p) : nullptr,
                           static_cast<uint64_t*>(out_a_.p), cap, d_stats));
  BIC_TRY(bic_sync(ctx_));
  uint64_t st[3];
  BIC_TRY(bic_memcpy_d2h(ctx_, st, d_stats, sizeof(st)));
  out->weights.resize(nt);
  out->w_nonpred.resize(nt);
  out->w_pred.resize(nt);
  out->modes.resize(nt);
  BIC_TRY(bic_memcpy_d2h(ctx_, out->weights.data(), d_w, nt * 4));
  BIC_TRY(bic_memcpy_d2h(ctx_, out->w_nonpred.data(), d_w + nt, nt * 4));
  BIC_TRY(bic_memcpy_d2h(ctx_, out->w_pred.data(), d_w + 2 * nt, nt * 4));
  BIC_TRY(bic_memcpy_d2h(ctx_, out->modes.data(), d_modes, nt));
  out->L = st[2];
  BIC_TRY(fetch_stream(static_cast<uint64_t*>(out_a_.p), st[0], &out->stream));
  if (resid) BIC_TRY(download(static_cast<uint64_t*>(out_b_.p), *resid));
  return BIC_OK;
}

int Device::patch_search(const binary_matrix& I, unsigned W, std::vector<uint32_t>* besti,
                         std::vector<uint32_t>* bestj, std::vector<uint32_t>* bestd) {
  BIC_TRY(status_);
  if (!besti || !bestj || !bestd || W < 1 || W > 64) return BIC_EINVAL;
  const idx_t rows = I.get_rows(), cols = I.get_cols(), wpr = I.get_blocks_per_row();
  const size_t nt = ((W - 1 + rows) / W) * ((W - 1 + cols) / W);
  besti->assign(nt, 0);
  bestj->assign(nt, 0);
  bestd->assign(nt, W * W);
  if (nt == 0) return BIC_OK;
  BIC_TRY(ensure(in_, rows * wpr * 8));
  BIC_TRY(ensure(aux_, 3 * nt * 4));
  uint32_t* d = static_cast<uint32_t*>(aux_.p);
  BIC_TRY(upload(I, static_cast<uint64_t*>(in_.p)));
  BIC_TRY(bic_patch_search(ctx_, static_cast<const uint64_t*>(in_.p), rows, cols, wpr, W, d, d + nt, d + 2 * nt));
  BIC_TRY(bic_sync(ctx_));
  BIC_TRY(bic_memcpy_d2h(ctx_, besti->data(), d, nt * 4));
  BIC_TRY(bic_memcpy_d2h(ctx_, bestj->data(), d + nt, nt * 4));
  BIC_TRY(bic_memcpy_d2h(ctx_, bestd->data(), d + 2 * nt, nt * 4));
  return BIC_OK;
}

int Device::match_encode(binary_matrix& I, unsigned W, unsigned T, unsigned R, MatchResult* out,
                         GolombCoder* golomb_match, GolombCoder* golomb_nomatch, const double* enuml) {
  BIC_TRY(status_);
  if (!out || W < 1 || W > 64) return BIC_EINVAL;
  if ((golomb_match && !coder_state::fresh(*golomb_match)) || (golomb_nomatch && !coder_state::fresh(*golomb_nomatch)))
    return BIC_EINVAL;
  const idx_t rows = I.get_rows(), cols = I.get_cols(), wpr = I.get_blocks_per_row();
  if (rows % W || cols % W) return BIC_EINVAL;
  const size_t nt = (rows / W) * (cols / W), M = (size_t)W * W;
  *out = MatchResult();
  if (nt == 0) return BIC_OK;
  std::vector<double> table;
  if (!enuml) {
    table.resize(M + 1);
    for (size_t w = 0; w <= M; ++w) table[w] = bic_enum_codelength((unsigned)M, (unsigned)w);
    enuml = table.data();
  }
  const size_t cap = (rows * cols + 33 * nt + 63) / 64 + 1;  // both streams, always enough
  const size_t tile_bytes = ((4 * 4 + 1) * nt + 255) & ~(size_t)255;
  BIC_TRY(ensure(in_, rows * wpr * 8));
  BIC_TRY(ensure(out_a_, 2 * cap * 8));
  BIC_TRY(ensure(aux_, tile_bytes));
  BIC_TRY(ensure(small_, 64));
  uint64_t* d_I = static_cast<uint64_t*>(in_.p);
  uint64_t* d_s = static_cast<uint64_t*>(out_a_.p);
  uint32_t* d_t = static_cast<uint32_t*>(aux_.p);
  uint64_t* d_st = static_cast<uint64_t*>(small_.p);
  BIC_TRY(upload(I, d_I));
  BIC_TRY(bic_match_encode(ctx_, d_I, rows, cols, wpr, W, T, R, enuml, d_t, d_t + nt, d_t + 2 * nt, d_t + 3 * nt,
                           reinterpret_cast<uint8_t*>(d_t + 4 * nt), d_I, d_s, d_s + cap, cap, d_st));
  BIC_TRY(bic_sync(ctx_));
  uint64_t st[4];
  BIC_TRY(bic_memcpy_d2h(ctx_, st, d_st, sizeof(st)));
  std::vector<uint32_t>* arrs[4] = {&out->besti, &out->bestj, &out->bestd, &out->weights};
  for (int k = 0; k < 4; ++k) {
    arrs[k]->resize(nt);
    BIC_TRY(bic_memcpy_d2h(ctx_, arrs[k]->data(), d_t + k * nt, nt * 4));
  }
  out->modes.resize(nt);
  BIC_TRY(bic_memcpy_d2h(ctx_, out->modes.data(), d_t + 4 * nt, nt));
  BIC_TRY(fetch_stream(d_s, st[1], &out->stream_match));
  BIC_TRY(fetch_stream(d_s + cap, st[2], &out->stream_nomatch));
  BIC_TRY(download(d_I, I));
  out->matches = st[0];
  out->L = st[3];
  // the coders' state: samples, their sum and bits per coder
  uint64_t n[2] = {0, 0}, sum[2] = {0, 0};
  for (size_t i = 0; i < nt; ++i) {
    const int c = (out->modes[i] == 'X' || out->modes[i] == 'x') ? 0 : 1;
    n[c] += 1;
    sum[c] += out->weights[i];
  }
  if (golomb_match) coder_state::advance(*golomb_match, n[0], sum[0], st[1]);
  if (golomb_nomatch) coder_state::advance(*golomb_nomatch, n[1], sum[1], st[2]);
  return BIC_OK;
}

int Device::dict_encode(const binary_matrix& I, int variant, unsigned W, unsigned T, unsigned atom_step,
                        DictResult* out, GolombCoder* golomb_match, GolombCoder* golomb_nomatch, const double* enuml) {
  BIC_TRY(status_);
  if (!out || W < 1 || W > 64 || (variant != 2 && variant != 3) || (atom_step != 1 && atom_step != W)) return BIC_EINVAL;
  if ((golomb_match && !coder_state::fresh(*golomb_match)) || (golomb_nomatch && !coder_state::fresh(*golomb_nomatch)))
    return BIC_EINVAL;
  const idx_t rows = I.get_rows(), cols = I.get_cols(), wpr = I.get_blocks_per_row();
  const size_t nt = ((W - 1 + rows) / W) * ((W - 1 + cols) / W), M = (size_t)W * W;
  *out = DictResult();
  if (nt == 0) return BIC_OK;
  std::vector<double> table;
  if (!enuml) {
    table.resize(M + 1);
    for (size_t w = 0; w <= M; ++w) table[w] = bic_enum_codelength((unsigned)M, (unsigned)w);
    enuml = table.data();
  }
  const size_t cap = variant == 3 ? (nt * (M + 33) + 63) / 64 + 1 : 0;  // a sample <= M: always enough
  const size_t tile_bytes = ((5 * 4 + 2) * nt + 255) & ~(size_t)255;
  BIC_TRY(ensure(in_, rows * wpr * 8));
  BIC_TRY(ensure(out_a_, 2 * cap * 8 + 8));
  BIC_TRY(ensure(aux_, tile_bytes));
  BIC_TRY(ensure(small_, 64));
  uint64_t* d_I = static_cast<uint64_t*>(in_.p);
  uint64_t* d_s = static_cast<uint64_t*>(out_a_.p);
  uint32_t* d_t = static_cast<uint32_t*>(aux_.p);
  uint8_t* d_b = reinterpret_cast<uint8_t*>(d_t + 5 * nt);
  uint64_t* d_st = static_cast<uint64_t*>(small_.p);
  BIC_TRY(upload(I, d_I));
  BIC_TRY(bic_dict_encode(ctx_, variant, d_I, rows, cols, wpr, W, T, atom_step, enuml, d_t, d_t + nt, d_t + 2 * nt,
                          d_t + 3 * nt, d_b, d_b + nt, d_t + 4 * nt, cap ? d_s : nullptr, cap ? d_s + cap : nullptr,
                          cap, d_st));
  BIC_TRY(bic_sync(ctx_));
  uint64_t st[5];
  BIC_TRY(bic_memcpy_d2h(ctx_, st, d_st, sizeof(st)));
  std::vector<uint32_t>* arrs[5] = {&out->bestk, &out->bestd, &out->dsize, &out->weights, &out->dict_tiles};
  for (int k = 0; k < 5; ++k) {
    arrs[k]->resize(k == 4 ? st[4] : nt);
    BIC_TRY(bic_memcpy_d2h(ctx_, arrs[k]->data(), d_t + k * nt, arrs[k]->size() * 4));
  }
  out->modes.resize(nt);
  out->joined.resize(nt);
  BIC_TRY(bic_memcpy_d2h(ctx_, out->modes.data(), d_b, nt));
  BIC_TRY(bic_memcpy_d2h(ctx_, out->joined.data(), d_b + nt, nt));
  out->matches = st[0];
  out->L = st[3];
  if (variant != 3) return BIC_OK;
  BIC_TRY(fetch_stream(d_s, st[1], &out->stream_match));
  BIC_TRY(fetch_stream(d_s + cap, st[2], &out->stream_nomatch));
  // the coders' state: samples, their sum and bits per coder (the first tile codes no sample)
  uint64_t n[2] = {0, 0}, sum[2] = {0, 0};
  for (size_t i = 1; i < nt; ++i) {
    const int c = out->modes[i] == 'x' ? 0 : 1;
    n[c] += 1;
    sum[c] += out->weights[i];
  }
  if (golomb_match) coder_state::advance(*golomb_match, n[0], sum[0], st[1]);
  if (golomb_nomatch) coder_state::advance(*golomb_nomatch, n[1], sum[1], st[2]);
  return BIC_OK;
}

int Device::bsvd_run(int step, const binary_matrix* X, binary_matrix& E, binary_matrix& D, binary_matrix& A,
                     size_t max_iter, idx_t* result, int du, idx_t* rounds, int lm) {
  BIC_TRY(status_);
  const idx_t n = E.get_rows(), m = E.get_cols(), p = D.get_rows();
  if (D.get_cols() != m || A.get_rows() != n || A.get_cols() != p || (X && !same_shape(*X, E))) return BIC_EINVAL;
  if ((n && (!E.raw_blocks() || !A.raw_blocks())) || (p && !D.raw_blocks())) return BIC_EINVAL;
  const idx_t ew = E.get_blocks_per_row(), dw = D.get_blocks_per_row(), aw = A.get_blocks_per_row();
  BIC_TRY(ensure(out_a_, n * ew * 8 + 8));
  BIC_TRY(ensure(out_b_, p * dw * 8 + 8));
  BIC_TRY(ensure(aux_, n * aw * 8 + 8));
  BIC_TRY(ensure(small_, 64));
  if (X) BIC_TRY(ensure(in_, n * ew * 8 + 8));
  uint64_t* d_E = static_cast<uint64_t*>(out_a_.p);
  uint64_t* d_D = static_cast<uint64_t*>(out_b_.p);
  uint64_t* d_A = static_cast<uint64_t*>(aux_.p);
  uint64_t* d_ch = static_cast<uint64_t*>(small_.p);
  if (!X) BIC_TRY(upload(E, d_E));  // (learn forms E itself)
  BIC_TRY(upload(D, d_D));
  BIC_TRY(upload(A, d_A));
  uint64_t res = 0;
  const bool wide = m > 4096;  // the narrow entries' domain ends there: the wide ones give the same results
  if (step == 2) {
    uint64_t* d_X = static_cast<uint64_t*>(in_.p);
    BIC_TRY(upload(*X, d_X));
    size_t it = 0;
    if (wide || lm != BIC_BSVD_LM_TRADITIONAL)
      BIC_TRY(bic_bsvd_learn_lm(ctx_, lm, du, d_X, ew, d_E, n, m, ew, d_D, p, dw, d_A, aw, max_iter, &it));
    else
      BIC_TRY(bic_bsvd_learn_du(ctx_, du, d_X, ew, d_E, n, m, ew, d_D, p, dw, d_A, aw, max_iter, &it));
    res = it;
  } else if (step == 3) {
    size_t r = 0;
    if (wide)
      BIC_TRY(bic_bsvd_update_dictionary_wide(ctx_, BIC_BSVD_DU_PROXIMUS, d_E, n, m, ew, d_D, p, dw, d_A, aw, d_ch, &r));
    else
      BIC_TRY(bic_bsvd_update_dictionary_proximus(ctx_, d_E, n, m, ew, d_D, p, dw, d_A, aw, d_ch, &r));
    BIC_TRY(bic_memcpy_d2h(ctx_, &res, d_ch, 8));
    if (rounds) *rounds = r;
  } else {
    if (step == 0 && wide) BIC_TRY(bic_bsvd_update_coefficients_wide(ctx_, d_E, n, m, ew, d_D, p, dw, d_A, aw, d_ch));
    else if (step == 0) BIC_TRY(bic_bsvd_update_coefficients(ctx_, d_E, n, m, ew, d_D, p, dw, d_A, aw, d_ch));
    else if (wide)
      BIC_TRY(bic_bsvd_update_dictionary_wide(ctx_, BIC_BSVD_DU_STEEPEST, d_E, n, m, ew, d_D, p, dw, d_A, aw, d_ch,
                                              nullptr));
    else BIC_TRY(bic_bsvd_update_dictionary(ctx_, d_E, n, m, ew, d_D, p, dw, d_A, aw, d_ch));
    BIC_TRY(bic_memcpy_d2h(ctx_, &res, d_ch, 8));  // (waits for the step)
  }
  BIC_TRY(download(d_E, E));
  if (step != 0) BIC_TRY(download(d_D, D));
  if (step != 1) BIC_TRY(download(d_A, A));  // (step 3 changes all three)
  if (result) *result = res;
  return BIC_OK;
}

int Device::bsvd_update_coefficients(binary_matrix& E, const binary_matrix& D, binary_matrix& A, idx_t* changed) {
  return bsvd_run(0, nullptr, E, const_cast<binary_matrix&>(D), A, 0, changed);  // (step 0 only reads D)
}

int Device::bsvd_update_dictionary(binary_matrix& E, binary_matrix& D, const binary_matrix& A, idx_t* changed) {
  return bsvd_run(1, nullptr, E, D, const_cast<binary_matrix&>(A), 0, changed);  // (step 1 only reads A)
}

int Device::bsvd_learn(binary_matrix& X, binary_matrix& E, binary_matrix& D, binary_matrix& A, size_t max_iter,
                       idx_t* iters) {
  return bsvd_run(2, &X, E, D, A, max_iter, iters);
}

int Device::bsvd_learn(binary_matrix& X, binary_matrix& E, binary_matrix& D, binary_matrix& A, int du, size_t max_iter,
                       idx_t* iters) {
  return bsvd_run(2, &X, E, D, A, max_iter, iters, du);
}

int Device::bsvd_learn(int lm, int du, binary_matrix& X, binary_matrix& E, binary_matrix& D, binary_matrix& A,
                       size_t max_iter, idx_t* iters) {
  return bsvd_run(2, &X, E, D, A, max_iter, iters, du, nullptr, lm);
}

int Device::bsvd_update_dictionary_proximus(binary_matrix& E, binary_matrix& D, binary_matrix& A, idx_t* changed,
                                            idx_t* rounds) {
  return bsvd_run(3, nullptr, E, D, A, 0, changed, BIC_BSVD_DU_PROXIMUS, rounds);
}

int Device::bsvd_initialize(int mi, const binary_matrix& E, binary_matrix& D, binary_matrix& A, uint64_t* state) {
  BIC_TRY(status_);
  const idx_t n = E.get_rows(), m = E.get_cols(), p = D.get_rows();
  if (D.get_cols() != m || A.get_rows() != n || A.get_cols() != p) return BIC_EINVAL;
  if (!n || !p || !E.raw_blocks() || !A.raw_blocks() || !D.raw_blocks()) return BIC_EINVAL;
  const idx_t ew = E.get_blocks_per_row(), dw = D.get_blocks_per_row(), aw = A.get_blocks_per_row();
  BIC_TRY(ensure(out_a_, n * ew * 8 + 8));
  BIC_TRY(ensure(out_b_, p * dw * 8 + 8));
  BIC_TRY(ensure(aux_, n * aw * 8 + 8));
  uint64_t* d_E = static_cast<uint64_t*>(out_a_.p);
  uint64_t* d_D = static_cast<uint64_t*>(out_b_.p);
  uint64_t* d_A = static_cast<uint64_t*>(aux_.p);
  BIC_TRY(upload(E, d_E));
  if (dw > (m + 63) / 64) BIC_TRY(upload(D, d_D));  // (words past a row's own are not written: they come back as sent)
  if (aw > (p + 63) / 64) BIC_TRY(upload(A, d_A));
  BIC_TRY(bic_bsvd_initialize(ctx_, mi, d_E, n, m, ew, d_D, p, dw, d_A, aw, state));
  BIC_TRY(download(d_D, D));  // (waits for the work)
  BIC_TRY(download(d_A, A));
  return BIC_OK;
}

int Device::bsvd_model_codelength(const binary_matrix& E, const binary_matrix& D, const binary_matrix& A,
                                  uint64_t* length) {
  BIC_TRY(status_);
  const idx_t n = E.get_rows(), m = E.get_cols(), p = D.get_rows();
  if (!length || !n || !m || !E.raw_blocks()) return BIC_EINVAL;
  if (p && (D.get_cols() != m || A.get_rows() != n || A.get_cols() != p || !D.raw_blocks() || !A.raw_blocks()))
    return BIC_EINVAL;
  const idx_t ew = E.get_blocks_per_row(), dw = p ? D.get_blocks_per_row() : 0, aw = p ? A.get_blocks_per_row() : 0;
  BIC_TRY(ensure(out_a_, n * ew * 8 + 8));
  BIC_TRY(ensure(out_b_, p * dw * 8 + 8));
  BIC_TRY(ensure(aux_, n * aw * 8 + 8));
  uint64_t* d_E = static_cast<uint64_t*>(out_a_.p);
  uint64_t* d_D = static_cast<uint64_t*>(out_b_.p);
  uint64_t* d_A = static_cast<uint64_t*>(aux_.p);
  BIC_TRY(upload(E, d_E));
  if (p) {
    BIC_TRY(upload(D, d_D));
    BIC_TRY(upload(A, d_A));
  }
  return bic_bsvd_model_codelength(ctx_, d_E, n, m, ew, p ? d_D : nullptr, p, dw, p ? d_A : nullptr, aw, length);
}

int Device::bsvd_learn_mdl(int search, int lmi, int du, int mi, binary_matrix& X, binary_matrix& E, binary_matrix& D,
                           binary_matrix& A, uint64_t* state, MdlResult* out, size_t p_cap) {
  BIC_TRY(status_);
  const idx_t n = E.get_rows(), m = E.get_cols(), p = D.get_rows();
  if (!out || D.get_cols() != m || A.get_rows() != n || A.get_cols() != p || !same_shape(X, E)) return BIC_EINVAL;
  if (!n || !m || !p || !E.raw_blocks() || !A.raw_blocks() || !D.raw_blocks()) return BIC_EINVAL;
  if (search != BIC_BSVD_MDL_FORWARD) p_cap = p;  // only the forward search grows the model
  else if (!p_cap) p_cap = 4096;
  if (p > p_cap || p_cap > 4096) return BIC_EINVAL;
  const idx_t ew = E.get_blocks_per_row(), dw = D.get_blocks_per_row(), aw = A.get_blocks_per_row();
  const idx_t cw = (p_cap + 63) / 64;  // A's pitch on the device
  BIC_TRY(ensure(in_, n * ew * 8 + 8));
  BIC_TRY(ensure(out_a_, n * ew * 8 + 8));
  BIC_TRY(ensure(out_b_, p_cap * dw * 8 + 8));
  BIC_TRY(ensure(aux_, n * cw * 8 + 8));
  uint64_t* d_X = static_cast<uint64_t*>(in_.p);
  uint64_t* d_E = static_cast<uint64_t*>(out_a_.p);
  uint64_t* d_D = static_cast<uint64_t*>(out_b_.p);
  uint64_t* d_A = static_cast<uint64_t*>(aux_.p);
  BIC_TRY(upload(X, d_X));
  BIC_TRY(upload(E, d_E));  // (the full search may leave it as it is)
  BIC_TRY(upload(D, d_D));
  std::vector<uint64_t> wide(n * cw, 0);
  for (idx_t i = 0; i < n; ++i) std::memcpy(&wide[i * cw], A.raw_blocks() + i * aw, aw * 8);
  BIC_TRY(bic_memcpy_h2d(ctx_, d_A, wide.data(), wide.size() * 8));
  size_t atoms = 0, passes = 0;
  uint64_t len = 0;
  out->trace.assign(p_cap + 16, bic_bsvd_mdl_step{});  // (a search runs at most p_cap passes)
  const int rc = bic_bsvd_learn_mdl(ctx_, search, lmi, du, mi, d_X, ew, d_E, n, m, ew, d_D, p, p_cap, dw, d_A, cw, state,
                                    &atoms, &len, out->trace.data(), out->trace.size(), &passes);
  out->trace.resize(std::min(passes, out->trace.size()));
  if (rc != BIC_OK && rc != BIC_ENOSPC) return rc;
  out->atoms = atoms;
  out->length = len;
  if (search == BIC_BSVD_MDL_FULL && atoms == 0) return rc;  // nothing was taken: E, D and A stay
  BIC_TRY(download(d_E, E));
  D.destroy();
  A.destroy();
  if (atoms) {
    D.allocate(atoms, m);
    A.allocate(n, atoms);
    BIC_TRY(download(d_D, D));
    BIC_TRY(bic_memcpy_d2h(ctx_, wide.data(), d_A, wide.size() * 8));
    const idx_t rw = A.get_blocks_per_row();
    for (idx_t i = 0; i < n; ++i) std::memcpy(A.raw_blocks() + i * rw, &wide[i * cw], rw * 8);
  }
  return rc;
}

namespace {
// M as rows x cols, its storage kept where it already has that shape
void reshape(binary_matrix& M, idx_t rows, idx_t cols) {
  if (M.raw_blocks() && M.get_rows() == rows && M.get_cols() == cols) return;
  M.destroy();
  M.allocate(rows, cols);
}
}  // namespace

int Device::patches(const binary_matrix& I, unsigned W, binary_matrix& X) {
  BIC_TRY(status_);
  const idx_t rows = I.get_rows(), cols = I.get_cols(), wpr = I.get_blocks_per_row();
  if (!rows || !cols || !I.raw_blocks() || W < 1 || W > 1024) return BIC_EINVAL;
  const idx_t n = ((W - 1 + rows) / W) * ((W - 1 + cols) / W), m = (idx_t)W * W;
  reshape(X, n, m);
  const idx_t xw = X.get_blocks_per_row();
  BIC_TRY(ensure(in_, rows * wpr * 8));
  BIC_TRY(ensure(out_a_, n * xw * 8));
  uint64_t* d_I = static_cast<uint64_t*>(in_.p);
  uint64_t* d_X = static_cast<uint64_t*>(out_a_.p);
  BIC_TRY(upload(I, d_I));
  BIC_TRY(bic_patches_gather(ctx_, d_I, rows, cols, wpr, W, d_X, xw));
  return download(d_X, X);  // (waits for the work)
}

int Device::unpatch(const binary_matrix& X, unsigned W, binary_matrix& I) {
  BIC_TRY(status_);
  const idx_t rows = I.get_rows(), cols = I.get_cols(), wpr = I.get_blocks_per_row();
  if (!rows || !cols || !I.raw_blocks() || !X.raw_blocks() || W < 1 || W > 1024) return BIC_EINVAL;
  const idx_t n = ((W - 1 + rows) / W) * ((W - 1 + cols) / W), xw = X.get_blocks_per_row();
  if (X.get_rows() != n || X.get_cols() != (idx_t)W * W) return BIC_EINVAL;
  BIC_TRY(ensure(in_, n * xw * 8));
  BIC_TRY(ensure(out_a_, rows * wpr * 8));
  uint64_t* d_X = static_cast<uint64_t*>(in_.p);
  uint64_t* d_I = static_cast<uint64_t*>(out_a_.p);
  BIC_TRY(upload(X, d_X));
  BIC_TRY(bic_patches_scatter(ctx_, d_X, xw, W, d_I, rows, cols, wpr));
  return download(d_I, I);
}

int Device::mosaic(const binary_matrix& D, binary_matrix& image) {
  BIC_TRY(status_);
  const idx_t n = D.get_rows(), m = D.get_cols(), dw = D.get_blocks_per_row();
  size_t irows = 0, icols = 0;
  if (!D.raw_blocks()) return BIC_EINVAL;
  BIC_TRY(bic_mosaic_dims(n, m, &irows, &icols));
  reshape(image, irows, icols);
  const idx_t iw = image.get_blocks_per_row();
  BIC_TRY(ensure(in_, n * dw * 8));
  BIC_TRY(ensure(out_a_, irows * iw * 8));
  uint64_t* d_D = static_cast<uint64_t*>(in_.p);
  uint64_t* d_img = static_cast<uint64_t*>(out_a_.p);
  BIC_TRY(upload(D, d_D));
  BIC_TRY(bic_mosaic(ctx_, d_D, n, m, dw, d_img, iw));
  return download(d_img, image);
}

int Device::bsvd_learn_image(int mi, int lm, int du, const binary_matrix& I, unsigned W, idx_t p, binary_matrix& X,
                             binary_matrix& E, binary_matrix& D, binary_matrix& A, uint64_t* state, size_t max_iter,
                             idx_t* iters, binary_matrix* residual) {
  BIC_TRY(status_);
  const idx_t rows = I.get_rows(), cols = I.get_cols(), wpr = I.get_blocks_per_row();
  if (!rows || !cols || !I.raw_blocks() || W < 1 || W > 64 || p < 1 || p > 4096) return BIC_EINVAL;
  const idx_t n = ((W - 1 + rows) / W) * ((W - 1 + cols) / W), m = (idx_t)W * W;
  reshape(X, n, m);
  reshape(E, n, m);
  reshape(D, p, m);
  reshape(A, n, p);
  if (residual) reshape(*residual, rows, cols);
  const idx_t xw = X.get_blocks_per_row(), aw = A.get_blocks_per_row();
  // the plane and, behind it, the residual image share one buffer
  BIC_TRY(ensure(in_, 2 * rows * wpr * 8));
  BIC_TRY(ensure(small_, n * xw * 8));
  BIC_TRY(ensure(out_a_, n * xw * 8));
  BIC_TRY(ensure(out_b_, p * xw * 8));
  BIC_TRY(ensure(aux_, n * aw * 8));
  uint64_t* d_I = static_cast<uint64_t*>(in_.p);
  uint64_t* d_R = d_I + rows * wpr;
  uint64_t* d_X = static_cast<uint64_t*>(small_.p);
  uint64_t* d_E = static_cast<uint64_t*>(out_a_.p);
  uint64_t* d_D = static_cast<uint64_t*>(out_b_.p);
  uint64_t* d_A = static_cast<uint64_t*>(aux_.p);
  BIC_TRY(upload(I, d_I));
  size_t it = 0;
  BIC_TRY(bic_bsvd_learn_image(ctx_, mi, lm, du, d_I, rows, cols, wpr, W, d_X, xw, d_E, xw, d_D, p, xw, d_A, aw, state,
                               max_iter, &it, residual ? d_R : nullptr, wpr));
  BIC_TRY(download(d_X, X));
  BIC_TRY(download(d_E, E));
  BIC_TRY(download(d_D, D));
  BIC_TRY(download(d_A, A));
  if (residual) BIC_TRY(download(d_R, *residual));
  if (iters) *iters = it;
  return BIC_OK;
}

Device& default_device() {
  static Device* dev = new Device(0);
  if (dev->status() != BIC_OK) {
    std::fprintf(stderr, "bic: no usable gfx950 device for the GPU hot path: %s\n", bic_strerror(dev->status()));
    std::abort();
  }
  return *dev;
}

}  // namespace bic

// ---- include/bsvd.h on the default device --------------------------------------------------------
namespace {
idx_t bsvd_or_abort(const char* what, int rc, idx_t value) {
  if (rc != BIC_OK) {
    std::fprintf(stderr, "%s: %s\n", what, bic_strerror(rc));
    std::abort();
  }
  return value;
}
}  // namespace

// the reference's process-wide generator (get_rng, bsvd.cpp:8-15): seeded from random_seed at the first draw
long random_seed = 34503498;
mi_algorithm_t initialize_model = initialize_model_neighbor;
cu_algorithm_t update_coefficients = update_coefficients_omp;
// (the reference initialises this one with itself, i.e. null, and relies on learn_model_setup)
du_algorithm_t update_dictionary = update_dictionary_steepest;

namespace {
// (seeded by the first rule that draws; the MDL searches share it)
uint64_t* bsvd_rng_state(int mi) {
  static uint64_t state = 0;
  static bool seeded = false;
  if (mi != BIC_BSVD_MI_PARTITION && !seeded) {
    bic_bsvd_rng_seed((uint64_t)random_seed, &state);
    seeded = true;
  }
  return &state;
}

void bsvd_initialize_or_abort(const char* what, int mi, const binary_matrix& E, binary_matrix& D, binary_matrix& A) {
  bsvd_or_abort(what, bic::default_device().bsvd_initialize(mi, E, D, A, bsvd_rng_state(mi)), 0);
}
}  // namespace

void initialize_model_neighbor(const binary_matrix& E, binary_matrix& D, binary_matrix& A) {
  bsvd_initialize_or_abort("initialize_model_neighbor", BIC_BSVD_MI_NEIGHBOR, E, D, A);
}

void initialize_model_partition(const binary_matrix& E, binary_matrix& D, binary_matrix& A) {
  bsvd_initialize_or_abort("initialize_model_partition", BIC_BSVD_MI_PARTITION, E, D, A);
}

void initialize_model_random_centroids(const binary_matrix& E, binary_matrix& D, binary_matrix& A) {
  bsvd_initialize_or_abort("initialize_model_random_centroids", BIC_BSVD_MI_CENTROIDS, E, D, A);
}

void initialize_model_random_centroids_xor(const binary_matrix& E, binary_matrix& D, binary_matrix& A) {
  bsvd_initialize_or_abort("initialize_model_random_centroids_xor", BIC_BSVD_MI_CENTROIDS_XOR, E, D, A);
}

idx_t update_coefficients_basic(binary_matrix& E, const binary_matrix& D, binary_matrix& A) {
  idx_t changed = 0;
  const int rc = bic::default_device().bsvd_update_coefficients(E, D, A, &changed);
  return bsvd_or_abort("update_coefficients_basic", rc, changed);
}

idx_t update_coefficients_omp(binary_matrix& E, const binary_matrix& D, binary_matrix& A) {
  idx_t changed = 0;
  const int rc = bic::default_device().bsvd_update_coefficients(E, D, A, &changed);
  return bsvd_or_abort("update_coefficients_omp", rc, changed);
}

idx_t update_dictionary_steepest(binary_matrix& E, binary_matrix& D, binary_matrix& A) {
  idx_t changed = 0;
  const int rc = bic::default_device().bsvd_update_dictionary(E, D, A, &changed);
  return bsvd_or_abort("update_dictionary_steepest", rc, changed);
}

idx_t update_dictionary_proximus(binary_matrix& E, binary_matrix& D, binary_matrix& A) {
  idx_t changed = 0;
  const int rc = bic::default_device().bsvd_update_dictionary_proximus(E, D, A, &changed);
  return bsvd_or_abort("update_dictionary_proximus", rc, changed);
}

idx_t update_dictionary_proximus_omp(binary_matrix& E, binary_matrix& D, binary_matrix& A) {
  idx_t changed = 0;
  const int rc = bic::default_device().bsvd_update_dictionary_proximus(E, D, A, &changed);
  return bsvd_or_abort("update_dictionary_proximus_omp", rc, changed);
}

namespace {
// the device rule behind the global update_dictionary: one of the four dictionary functions of bsvd.h
int bsvd_rule_or_abort(const char* what) {
  if (update_dictionary == update_dictionary_steepest) return BIC_BSVD_DU_STEEPEST;
  if (update_dictionary == update_dictionary_proximus || update_dictionary == update_dictionary_proximus_omp)
    return BIC_BSVD_DU_PROXIMUS;
  std::fprintf(stderr, "%s: update_dictionary is not one of this build's dictionary functions\n", what);
  std::abort();
}

idx_t bsvd_learn_or_abort(const char* what, int lm, binary_matrix& X, binary_matrix& E, binary_matrix& D,
                          binary_matrix& A) {
  idx_t iters = 0;
  const int du = bsvd_rule_or_abort(what);
  // (the traditional loop with the steepest rule stays the call it has always been)
  const int rc = (lm == BIC_BSVD_LM_TRADITIONAL && du == BIC_BSVD_DU_STEEPEST)
                     ? bic::default_device().bsvd_learn(X, E, D, A, 0, &iters)
                     : bic::default_device().bsvd_learn(lm, du, X, E, D, A, 0, &iters);
  return bsvd_or_abort(what, rc, iters);
}
}  // namespace

idx_t learn_model_traditional(binary_matrix& X, binary_matrix& E, binary_matrix& D, binary_matrix& A) {
  return bsvd_learn_or_abort("learn_model_traditional", BIC_BSVD_LM_TRADITIONAL, X, E, D, A);
}

idx_t learn_model_alter1(binary_matrix& X, binary_matrix& E, binary_matrix& D, binary_matrix& A) {
  return bsvd_learn_or_abort("learn_model_alter1", BIC_BSVD_LM_ALTER1, X, E, D, A);
}

idx_t learn_model_alter2(binary_matrix& X, binary_matrix& E, binary_matrix& D, binary_matrix& A) {
  return bsvd_learn_or_abort("learn_model_alter2", BIC_BSVD_LM_ALTER2, X, E, D, A);
}

idx_t learn_model_alter3(binary_matrix& X, binary_matrix& E, binary_matrix& D, binary_matrix& A) {
  return bsvd_learn_or_abort("learn_model_alter3", BIC_BSVD_LM_ALTER3, X, E, D, A);
}

// ---- the MDL model order (bsvd.cpp:1438-1717) ------------------------------------------------------
ml_algorithm_t learn_model = learn_model_traditional;
ml_algorithm_t learn_model_inner = learn_model_traditional;

const char* mi_algorithm_names[] = {"Neighbor initialization", "Partition initialization",
                                    "Random centroids initialization",
                                    "Random centroids (in mod-2 algebra) initialization",
                                    "Graph growing initialization", 0};
const char* cu_algorithm_names[] = {"OpenMP basic coefficients update", "Basic coefficients update",
                                    "Fast coefficients update (broken!)", 0};
const char* du_algorithm_names[] = {"Steepest descent (a la MOD)  dictionary update", "Proximus-like dictionary update",
                                    "Steepest descent (a la MOD)  dictionary update (OMP)",
                                    "Proximus-like dictionary update (OMP)", 0};
const char* lm_algorithm_names[] = {
    "Model learning by traditional alternate descent",
    "Role-switching learning 1: at each iteration, the role of A and D are switched",
    "Role-switched learning 2: after convergence, the role of A and D are switched and traditional model is applied "
    "again",
    "Role switched learning 3: like RS1 but only update_dictionary is applied (for use with Proximus",
    "MDL/forward selection",
    "MDO/backward selection",
    "MDL/full search",
    0};

namespace {
const mi_algorithm_t kInitialisers[] = {initialize_model_neighbor, initialize_model_partition,
                                        initialize_model_random_centroids, initialize_model_random_centroids_xor};
const ml_algorithm_t kLearners[] = {learn_model_traditional,           learn_model_alter1,
                                    learn_model_alter2,                learn_model_alter3,
                                    learn_model_mdl_forward_selection, learn_model_mdl_backward_selection,
                                    learn_model_mdl_full_search};

void missing_piece(const char* which) {
  std::cerr << which << " is not part of this build" << std::endl;
  std::exit(-1);
}

void print_pass(const bic_bsvd_mdl_step& r) {
  std::cout << "currK=" << r.K << " currL=" << r.currL << " bestK=" << r.bestK << " bestL=" << r.bestL
            << " stuck=" << r.stuck << " dif=" << r.dif << " dev=" << r.dev << std::endl;
}

// one search on the default device with what the globals say, then the reference's stdout lines from the trace
idx_t bsvd_mdl_or_abort(const char* what, int search, binary_matrix& X, binary_matrix& E, binary_matrix& D,
                        binary_matrix& A) {
  int lmi = -1, mi = -1;
  for (int i = 0; i < 4; ++i) {
    if (learn_model_inner == kLearners[i]) lmi = i;
    if (initialize_model == kInitialisers[i]) mi = i;
  }
  if (lmi < 0) {
    std::fprintf(stderr, "%s: learn_model_inner is not one of this build's four learners\n", what);
    std::abort();
  }
  if (mi < 0 && search != BIC_BSVD_MDL_BACKWARD) {
    std::fprintf(stderr, "%s: initialize_model is not one of this build's initialisers\n", what);
    std::abort();
  }
  if (mi < 0) mi = BIC_BSVD_MI_PARTITION;  // (the backward search draws nothing)
  const int du = bsvd_rule_or_abort(what);
  bic::Device::MdlResult r;
  const bool draws = search != BIC_BSVD_MDL_BACKWARD && mi != BIC_BSVD_MI_PARTITION;
  const int rc = bic::default_device().bsvd_learn_mdl(search, lmi, du, mi, X, E, D, A,
                                                      draws ? bsvd_rng_state(mi) : nullptr, &r);
  if (search == BIC_BSVD_MDL_FULL) {
    for (const bic_bsvd_mdl_step& s : r.trace) {
      std::cout << "K=" << s.K;
      for (int i = 0; i < 10; ++i) {
        random_seed = (random_seed * 31) % 17;  // :1686 (changes no draw: the generator is seeded once)
        std::cout << " " << s.lens[i];
      }
      std::cout << " " << s.currL << std::endl;
    }
    if (rc == BIC_OK) std::cout << "bestL=" << r.length << " bestk=" << r.atoms << std::endl;
  } else {
    for (const bic_bsvd_mdl_step& s : r.trace) print_pass(s);
    if (rc == BIC_OK && search == BIC_BSVD_MDL_BACKWARD && r.atoms == 0) {
      std::cout << "Resulted in empty model!" << std::endl;
    } else if (rc == BIC_OK && !r.trace.empty()) {
      // the last pass was rejected unless it made the model of K - 1 (forward: K + 1) atoms the best
      const bic_bsvd_mdl_step& last = r.trace.back();
      const uint64_t made = search == BIC_BSVD_MDL_FORWARD ? last.K + 1 : last.K - 1;
      if (last.stuck == 9 && r.atoms != made) std::cout << "No further improvement." << std::endl;
    }
  }
  return bsvd_or_abort(what, rc, r.length);
}
}  // namespace

idx_t model_codelength(const binary_matrix& E, const binary_matrix& D, const binary_matrix& A) {
  uint64_t len = 0;
  const int rc = bic::default_device().bsvd_model_codelength(E, D, A, &len);
  return bsvd_or_abort("model_codelength", rc, len);
}

idx_t learn_model_mdl_forward_selection(binary_matrix& X, binary_matrix& E, binary_matrix& D, binary_matrix& A) {
  return bsvd_mdl_or_abort("learn_model_mdl_forward_selection", BIC_BSVD_MDL_FORWARD, X, E, D, A);
}

idx_t learn_model_mdl_backward_selection(binary_matrix& X, binary_matrix& E, binary_matrix& D, binary_matrix& A) {
  return bsvd_mdl_or_abort("learn_model_mdl_backward_selection", BIC_BSVD_MDL_BACKWARD, X, E, D, A);
}

idx_t learn_model_mdl_full_search(binary_matrix& X, binary_matrix& E, binary_matrix& D, binary_matrix& A) {
  return bsvd_mdl_or_abort("learn_model_mdl_full_search", BIC_BSVD_MDL_FULL, X, E, D, A);
}

void learn_model_setup(int mi_algo, int cu_algo, int du_algo, int lm_algo, int lmi_algo) {
  // (bsvd.cpp:80-84: only the upper bounds are checked there; a negative index is refused here as well)
  if (mi_algo < 0 || mi_algo > 4) { std::cerr << "Invalid model initialization algorithm (0-" << 4 << ')' << std::endl; std::exit(-1); }
  if (cu_algo < 0 || cu_algo > 2) { std::cerr << "Invalid coefficients update algorithm (0-" << 2 << ')' << std::endl; std::exit(-1); }
  if (du_algo < 0 || du_algo > 3) { std::cerr << "Invalid dictionary update algorithm (0-" << 3 << ')' << std::endl; std::exit(-1); }
  if (lm_algo < 0 || lm_algo > 6) { std::cerr << "Invalid model learning algorithm (0-" << 6 << ')' << std::endl; std::exit(-1); }
  if (lmi_algo < 0 || lmi_algo > 3) { std::cerr << "Invalid inner model learning algorithm (0-" << 3 << ')' << std::endl; std::exit(-1); }
  if (mi_algo == 4) missing_piece("initialize_model_graph_grow (model initialization algorithm 4)");
  if (cu_algo == 2) missing_piece("update_coefficients_fast (coefficients update algorithm 2)");
  if (du_algo == 2) missing_piece("update_dictionary_steepest_omp (dictionary update algorithm 2)");
  const du_algorithm_t rules[] = {update_dictionary_steepest, update_dictionary_proximus, nullptr,
                                  update_dictionary_proximus_omp};
  initialize_model = kInitialisers[mi_algo];
  std::cout << "Using " << mi_algorithm_names[mi_algo] << std::endl;
  update_coefficients = cu_algo == 0 ? update_coefficients_omp : update_coefficients_basic;
  std::cout << "Using " << cu_algorithm_names[cu_algo] << std::endl;
  update_dictionary = rules[du_algo];
  std::cout << "Using " << du_algorithm_names[du_algo] << std::endl;
  learn_model = kLearners[lm_algo];
  std::cout << "Using " << lm_algorithm_names[lm_algo] << " for outer learning loop." << std::endl;
  learn_model_inner = kLearners[lmi_algo];
  std::cout << "Using " << lm_algorithm_names[lmi_algo] << " for inner learning." << std::endl;
}
