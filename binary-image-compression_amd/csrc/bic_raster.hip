// bic_raster.hip -- SURVEY.md §8 f3: PBM / PGM rasters on the device, read straight out of a file's
// bytes (any alignment: a raster starts after a header of any length), so a whole file -> streams
// path runs on the GPU with only the header parsed on the host (bic_pnm_parse_header).
//
//  * pbm.cpp:29-77 (read_pbm_data / write_pbm): P4 rows of ceil(cols / 8) bytes, MSB = leftmost
//    pixel, rows byte-aligned -- plane word w of row i is the big-endian value of the row's bytes
//    8w .. 8w + 7 (bytes past the row's end and pad bits 0).
//  * pnm.cpp:54-89 (read_pgm_p5_data) + bitplane_tool.cpp:24-30: P5 samples of 1 byte (maxval
//    < 256) or 2 bytes big-endian ((hi << 8) + lo, pnm.cpp:71-74), row-major, no row padding;
//    plane b = bit b of each sample.
// Each lane assembles its bytes from aligned 8-byte loads shifted by the raster's misalignment
// (neighbouring lanes share the loads' cache lines: 64 lanes read one contiguous span), and never
// touches an aligned word that holds no raster byte (no read past the buffer's last page).
#include "bic_device.h"

namespace bic {

// 8 raster bytes starting at byte p (little-endian u64: byte p in bits 0-7), p < end; words past
// end read as 0
__device__ __forceinline__ uint64_t bytes8(const uint8_t* base, uint64_t p, uint64_t end) {
  const uint64_t a = p >> 3, last = (end - 1) >> 3;
  const uint32_t s = (uint32_t)(p & 7);
  const uint64_t* W = reinterpret_cast<const uint64_t*>(base);
  const uint64_t lo = a <= last ? W[a] : 0ull;
  if (!s) return lo;
  const uint64_t hi = a + 1 <= last ? W[a + 1] : 0ull;
  return (lo >> (8 * s)) | (hi << (64 - 8 * s));
}

// P4 raster -> plane. Thread per plane word. `base` is the raster's 8-aligned floor (off = the
// raster's byte offset in it), so every load is aligned.
__global__ __launch_bounds__(256) void k_pbm_unpack2(const uint8_t* __restrict__ base, uint32_t off, uint32_t rows,
                                                     uint32_t cols, uint32_t wpr, uint64_t* __restrict__ plane) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint32_t used = (cols + 63) / 64, nb = (cols + 7) / 8;
  if (i >= (uint64_t)rows * wpr) return;
  const uint32_t row = (uint32_t)(i / wpr), w = (uint32_t)(i % wpr);
  uint64_t v = 0;
  if (w < used) {
    const uint64_t end = off + (uint64_t)rows * nb;
    v = bswap64(bytes8(base, off + (uint64_t)row * nb + 8ull * w, end));  // byte 0 = MSB
    const uint32_t valid = min(64u, cols - 64 * w);                         // pixels of this word
    if (valid < 64) v &= ~(~0ull >> valid);
  }
  plane[i] = v;
}

// plane -> P4 raster (8-aligned raster, rows a multiple of 8 bytes: one 8-byte store per word);
// otherwise byte stores.
__global__ __launch_bounds__(256) void k_pbm_pack2(const uint64_t* __restrict__ plane, uint32_t rows, uint32_t cols,
                                                   uint32_t wpr, uint8_t* __restrict__ raster, int vec) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint32_t used = (cols + 63) / 64, nb = (cols + 7) / 8;
  if (i >= (uint64_t)rows * used) return;
  const uint32_t row = (uint32_t)(i / used), w = (uint32_t)(i % used);
  uint64_t v = plane[(uint64_t)row * wpr + w];
  if (w == used - 1 && (cols & 63)) v &= ~(~0ull >> (cols & 63));
  if (vec) {
    reinterpret_cast<uint64_t*>(raster)[((uint64_t)row * nb >> 3) + w] = bswap64(v);
    return;
  }
  uint8_t* dst = raster + (uint64_t)row * nb + 8ull * w;
#pragma unroll
  for (int b = 0; b < 8; ++b)
    if (8 * w + b < nb) dst[b] = (uint8_t)(v >> (56 - 8 * b));
}

// P5 samples (BPP = 1 or 2 bytes) -> planes plane0 .. plane0 + nplanes - 1. Lane = output word w
// of a row (64 samples); 16 (BPP 1) or 32 (BPP 2) aligned loads, the 8 x 8 bit transposes of
// k_bitplanes_u8 per byte column.
// Rows of `pitch` bytes (a P5 raster: cols * BPP); selL / selH: the v_perm_b32 selectors of a two-byte
// sample's low and high bytes (wave-uniform: big-endian or the host's order).
// GC (BIC_OPT_GRAY_CODE): the planes of G(v) = v ^ (v >> 1) on the whole sample -- bit 7 of the low byte
// takes bit 0 of the high byte in.
// BPP 3 (bic_bitplanes_rgb): interleaved R G B pixels of one-byte samples (P6, pnm.cpp:194-239); the wave
// takes channel blockIdx.y -- 24 loads, two v_perm_b32 per four pixels (rgb_pick4) -- and writes planes
// plane0 .. of it as output planes channel * nplanes ..
// CT (BIC_OPT_COLOR_TRANSFORM, BPP 3): channels 0 and 2 also pick the green bytes and go through ct_forward4
// before G (1: subtract green, 2: folded; an instantiation each).
// SP (BIC_OPT_SAMPLE_PREDICT, BPP 1): every sample minus the one on its left (2: folded) before G, as in
// k_bitplanes_u8; the left of the word's first sample is one more byte load, 0 at column 0. With BPP 3
// (BIC_OPT_RGB_PREDICT) the same on the wave's channel after CT: the left pixel lies three bytes back.
template <int BPP, bool GC, int CT = 0, int SP = 0>
__global__ __launch_bounds__(256) void k_raster_planes(const uint8_t* __restrict__ base, uint32_t off, uint32_t rows,
                                                       uint32_t cols, int plane0, int nplanes,
                                                       uint64_t* __restrict__ planes, uint32_t wpr, uint64_t pitch,
                                                       uint32_t selL, uint32_t selH) {
  const uint32_t groups = (cols + 4095) / 4096;  // 64-word groups per row
  const uint64_t gw = (uint64_t)blockIdx.x * 4 + wave_id();
  if (gw >= (uint64_t)rows * groups) return;
  const uint32_t row = (uint32_t)(gw / groups), w = (uint32_t)(gw % groups) * 64 + lane_id();
  const uint32_t used = (cols + 63) / 64;
  if (w >= used) return;
  const uint64_t end = off + (uint64_t)(rows - 1) * pitch + (uint64_t)cols * BPP;
  const uint64_t p0 = off + (uint64_t)row * pitch + 64ull * w * BPP;
  uint64_t lo8[8], hi8[8];  // per group of 8 samples: the low / high bytes, little-endian
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    if constexpr (BPP == 1) {
      lo8[g] = bytes8(base, p0 + 8 * g, end);
      hi8[g] = 0;
    } else if constexpr (BPP == 3) {
      const uint64_t a = bytes8(base, p0 + 24 * g, end), b = bytes8(base, p0 + 24 * g + 8, end),
                     c = bytes8(base, p0 + 24 * g + 16, end);
      const uint32_t s1 = rgb_sel1(blockIdx.y), s2 = rgb_sel2(blockIdx.y);
      if constexpr (CT != 0) {
        uint32_t x0 = rgb_pick4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, s1, s2),
                 x1 = rgb_pick4((uint32_t)(b >> 32), (uint32_t)c, (uint32_t)(c >> 32), s1, s2);
        if (blockIdx.y != 1) {
          x0 = ct_forward4<CT>(x0, rgb_pick4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, rgb_sel1(1), rgb_sel2(1)));
          x1 = ct_forward4<CT>(x1, rgb_pick4((uint32_t)(b >> 32), (uint32_t)c, (uint32_t)(c >> 32), rgb_sel1(1),
                                             rgb_sel2(1)));
        }
        lo8[g] = ((uint64_t)x1 << 32) | x0;
      } else {
        lo8[g] = ((uint64_t)rgb_pick4((uint32_t)(b >> 32), (uint32_t)c, (uint32_t)(c >> 32), s1, s2) << 32) |
                 rgb_pick4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, s1, s2);
      }
      hi8[g] = 0;
    } else {
      const uint64_t a = bytes8(base, p0 + 16 * g, end), b = bytes8(base, p0 + 16 * g + 8, end);
      // sample = (byte 2k << 8) + byte 2k+1 (pnm.cpp:73): odd bytes are the low ones
      // (selL = 0x07050301, selH = 0x06040200; the host's little-endian order swaps them)
      lo8[g] = ((uint64_t)__builtin_amdgcn_perm((uint32_t)(b >> 32), (uint32_t)b, selL) << 32) |
               __builtin_amdgcn_perm((uint32_t)(a >> 32), (uint32_t)a, selL);
      hi8[g] = ((uint64_t)__builtin_amdgcn_perm((uint32_t)(b >> 32), (uint32_t)b, selH) << 32) |
               __builtin_amdgcn_perm((uint32_t)(a >> 32), (uint32_t)a, selH);
    }
  }
  if constexpr (SP != 0) {
    static_assert(BPP == 1 || BPP == 3 || SP == 0, "sample prediction: one-byte samples only");
    uint32_t prev = 0;
    if constexpr (BPP == 3) {  // the pixel left of the word: the same channel of it, T_ct'ed with its own green
      if (w) {
        prev = (uint32_t)base[p0 - 3 + blockIdx.y];
        if constexpr (CT != 0)
          if (blockIdx.y != 1) prev = ct_forward4<CT>(prev, (uint32_t)base[p0 - 2]) & 0xffu;
        prev <<= 24;
      }
    } else {
      prev = w ? (uint32_t)base[p0 - 1] << 24 : 0u;
    }
#pragma unroll
    for (int g = 0; g < 8; ++g) {  // (samples past the row's end: `mask` below)
      const uint32_t lo = (uint32_t)lo8[g], hi = (uint32_t)(lo8[g] >> 32);
      lo8[g] = ((uint64_t)sp_forward4<SP>(hi, lo) << 32) | sp_forward4<SP>(lo, prev);
      prev = hi;
    }
  }
  if constexpr (GC) {
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      lo8[g] ^= ((lo8[g] >> 1) & 0x7f7f7f7f7f7f7f7full) ^ ((hi8[g] & 0x0101010101010101ull) << 7);
      hi8[g] ^= (hi8[g] >> 1) & 0x7f7f7f7f7f7f7f7full;
    }
  }
  const uint32_t valid = min(64u, cols - 64 * w);
  const uint64_t mask = valid < 64 ? ~(~0ull >> valid) : ~0ull;  // samples past the row's end
  uint64_t TL[8], TH[8];
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    TL[g] = transpose8x8_r(bswap64(lo8[g]));  // byte b = plane b's 8 bits of the group
    TH[g] = BPP == 2 ? transpose8x8_r(bswap64(hi8[g])) : 0;
  }
  const uint64_t plane_words = (uint64_t)rows * wpr;
  if constexpr (BPP == 3) planes += (uint64_t)blockIdx.y * nplanes * plane_words;  // the channel's planes
  uint64_t* dst = planes + (uint64_t)row * wpr + w;
  for (int b = 0; b < nplanes; ++b) {
    const int sb = b + plane0;
    uint64_t v = 0;
#pragma unroll
    for (int g = 0; g < 8; ++g) v |= (((sb < 8 ? TL[g] : TH[g]) >> (8 * (sb & 7))) & 0xffull) << (56 - 8 * g);
    dst[b * plane_words] = v & mask;
  }
  if (w == used - 1)
    for (int b = 0; b < nplanes; ++b)
      for (uint32_t q = used; q < wpr; ++q) planes[b * plane_words + (uint64_t)row * wpr + q] = 0;  // pad words
}

// planes plane0 .. plane0 + nplanes - 1 -> gray samples (plane2pgm_tool.cpp:33-52: sample |= mask
// for every set bit of plane b, mask = 1 << b; bits no plane covers are 0). Lane = word w of a row
// (64 samples): byte (plane0 + b) & 7 of each group's 8x8 block holds plane b's byte, the 8x8 bit
// transpose (an involution) turns it back into 8 samples' bytes. BPS 1: one byte per sample; BPS 2:
// two bytes big-endian (the P5 layout write_p5_data uses for maxval >= 256, pnm.cpp:111-124).
// 16-byte stores when the row's bytes are 16-byte aligned (VEC), byte stores otherwise.
// GC (BIC_OPT_GRAY_CODE): the planes are G's; sample bit b = XOR of the planes k >= b (bits no plane
// covers count as 0), a suffix XOR over the blocks' bytes, then masked to the bits the planes cover.
// BPS 3 (bic_planes_to_rgb): planes c * nplanes + b are channel c's (plane0 + b); the three channels' bytes
// of a group of 8 pixels are interleaved R G B with v_perm_b32 (rgb_interleave4), 192 bytes per lane.
// CT (BIC_OPT_COLOR_TRANSFORM, BPS 3): the assembled R' and B' (after ungray_blocks and its mask) go through
// ct_inverse4 with the assembled G before the interleave; all eight bits of the result are written.
template <int BPS, bool VEC, bool GC, int CT = 0>
__global__ __launch_bounds__(256) void k_planes_gray(const uint64_t* __restrict__ planes, uint32_t rows, uint32_t cols,
                                                     uint32_t wpr, int plane0, int nplanes, uint8_t* __restrict__ gray,
                                                     uint64_t pitch) {
  const uint32_t groups = (cols + 4095) / 4096;
  const uint64_t gw = (uint64_t)blockIdx.x * 4 + wave_id();
  if (gw >= (uint64_t)rows * groups) return;
  const uint32_t row = (uint32_t)(gw / groups), w = (uint32_t)(gw % groups) * 64 + lane_id();
  const uint32_t used = (cols + 63) / 64;
  if (w >= used) return;
  const uint64_t plane_words = (uint64_t)rows * wpr;
  const uint64_t* src = planes + (uint64_t)row * wpr + w;
  if constexpr (BPS == 3) {
    uint8_t* dst = gray + (uint64_t)row * pitch + (uint64_t)w * 192;
    const uint32_t valid = min(64u, cols - 64 * w);
    uint64_t ch[3][8];  // per channel and group: the 8 pixels' bytes, little-endian
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      uint64_t TL[8], TH[8];
#pragma unroll
      for (int g = 0; g < 8; ++g) TL[g] = TH[g] = 0;
      for (int b = 0; b < nplanes; ++b) {
        const uint64_t v = src[(uint64_t)(c * nplanes + b) * plane_words];
#pragma unroll
        for (int g = 0; g < 8; ++g) TL[g] |= ((v >> (56 - 8 * g)) & 0xffull) << (8 * (b + plane0));
      }
      if constexpr (GC) ungray_blocks<1, 8>(TL, TH, ((1u << nplanes) - 1u) << plane0);
#pragma unroll
      for (int g = 0; g < 8; ++g) ch[c][g] = bswap64(transpose8x8_r(TL[g]));
    }
    uint32_t out[48];  // the 64 pixels' bytes in file order
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      if constexpr (CT != 0) {
#pragma unroll
        for (int c = 0; c < 3; c += 2)
          ch[c][g] = ((uint64_t)ct_inverse4<CT>((uint32_t)(ch[c][g] >> 32), (uint32_t)(ch[1][g] >> 32)) << 32) |
                     ct_inverse4<CT>((uint32_t)ch[c][g], (uint32_t)ch[1][g]);
      }
      rgb_interleave4((uint32_t)ch[0][g], (uint32_t)ch[1][g], (uint32_t)ch[2][g], out[6 * g], out[6 * g + 1],
                      out[6 * g + 2]);
      rgb_interleave4((uint32_t)(ch[0][g] >> 32), (uint32_t)(ch[1][g] >> 32), (uint32_t)(ch[2][g] >> 32),
                      out[6 * g + 3], out[6 * g + 4], out[6 * g + 5]);
    }
    if (VEC && valid == 64) {
#pragma unroll
      for (int q = 0; q < 12; ++q)
        reinterpret_cast<uint4*>(dst)[q] = make_uint4(out[4 * q], out[4 * q + 1], out[4 * q + 2], out[4 * q + 3]);
      return;
    }
#pragma unroll
    for (int i = 0; i < 192; ++i)
      if ((uint32_t)i < valid * 3) dst[i] = (uint8_t)(out[i >> 2] >> (8 * (i & 3)));
    return;
  }
  uint64_t TL[8], TH[8];
#pragma unroll
  for (int g = 0; g < 8; ++g) TL[g] = TH[g] = 0;
  for (int b = 0; b < nplanes; ++b) {
    const uint64_t v = src[b * plane_words];
    const int sb = b + plane0;
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      const uint64_t byte = ((v >> (56 - 8 * g)) & 0xffull) << (8 * (sb & 7));
      if (sb < 8) TL[g] |= byte;
      else TH[g] |= byte;
    }
  }
  if constexpr (GC) {
    const uint32_t smask = ((1u << nplanes) - 1u) << plane0;
    ungray_blocks<BPS, 8>(TL, TH, smask);
  }
  uint32_t out[BPS * 16];  // the 64 samples' bytes in file order
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    const uint64_t lo = bswap64(transpose8x8_r(TL[g]));  // byte k = sample 8g + k's low byte
    if constexpr (BPS == 1) {
      out[2 * g] = (uint32_t)lo;
      out[2 * g + 1] = (uint32_t)(lo >> 32);
    } else {
      const uint64_t hi = bswap64(transpose8x8_r(TH[g]));
      // big-endian samples: hi0 lo0 hi1 lo1 ...
      const uint32_t l0 = (uint32_t)lo, l1 = (uint32_t)(lo >> 32), h0 = (uint32_t)hi, h1 = (uint32_t)(hi >> 32);
      out[4 * g] = __builtin_amdgcn_perm(l0, h0, 0x05010400u);
      out[4 * g + 1] = __builtin_amdgcn_perm(l0, h0, 0x07030602u);
      out[4 * g + 2] = __builtin_amdgcn_perm(l1, h1, 0x05010400u);
      out[4 * g + 3] = __builtin_amdgcn_perm(l1, h1, 0x07030602u);
    }
  }
  uint8_t* dst = gray + (uint64_t)row * pitch + (uint64_t)w * 64 * BPS;
  const uint32_t valid = min(64u, cols - 64 * w);
  if (VEC && valid == 64) {
#pragma unroll
    for (int q = 0; q < BPS * 4; ++q)
      reinterpret_cast<uint4*>(dst)[q] = make_uint4(out[4 * q], out[4 * q + 1], out[4 * q + 2], out[4 * q + 3]);
    return;
  }
  for (uint32_t i = 0; i < valid * BPS; ++i) dst[i] = (uint8_t)(out[i >> 2] >> (8 * (i & 3)));
}

void launch_planes_gray(hipStream_t s, const uint64_t* planes, uint32_t rows, uint32_t cols, uint32_t wpr, int plane0,
                        int nplanes, int bps, uint8_t* gray, uint64_t pitch, bool gray_code, int color_transform) {
  const uint64_t waves = (uint64_t)rows * ((cols + 4095) / 4096);
  const uint32_t grid = (uint32_t)((waves + 3) / 4);
  if (!grid) return;
  const bool vec = reinterpret_cast<uintptr_t>(gray) % 16 == 0 && pitch % 16 == 0;
#define BIC_PGG(B, V, G) k_planes_gray<B, V, G><<<grid, 256, 0, s>>>(planes, rows, cols, wpr, plane0, nplanes, gray, pitch)
#define BIC_PG(B, V)                        \
  do {                                      \
    if (gray_code) BIC_PGG(B, V, true);     \
    else BIC_PGG(B, V, false);              \
  } while (0)
#define BIC_PGC(V, G, C) \
  k_planes_gray<3, V, G, C><<<grid, 256, 0, s>>>(planes, rows, cols, wpr, plane0, nplanes, gray, pitch)
#define BIC_PGC2(C)                                                          \
  do {                                                                       \
    if (gray_code) { if (vec) BIC_PGC(true, true, C); else BIC_PGC(false, true, C); }   \
    else { if (vec) BIC_PGC(true, false, C); else BIC_PGC(false, false, C); }           \
  } while (0)
  if (bps == 3 && color_transform == 1) BIC_PGC2(1);
  else if (bps == 3 && color_transform == 2) BIC_PGC2(2);
  else if (bps == 1) { if (vec) BIC_PG(1, true); else BIC_PG(1, false); }
  else if (bps == 3) { if (vec) BIC_PG(3, true); else BIC_PG(3, false); }
  else { if (vec) BIC_PG(2, true); else BIC_PG(2, false); }
#undef BIC_PGC2
#undef BIC_PGC
#undef BIC_PG
#undef BIC_PGG
}

void launch_pbm(hipStream_t s, bool pack, const uint8_t* raster_in, uint8_t* raster_out, const uint64_t* plane_in,
                uint64_t* plane_out, uint32_t rows, uint32_t cols, uint32_t wpr) {
  if (!pack) {
    const uint64_t n = (uint64_t)rows * wpr;
    const uintptr_t r = reinterpret_cast<uintptr_t>(raster_in);
    const uint8_t* base = reinterpret_cast<const uint8_t*>(r & ~(uintptr_t)7);
    if (n) k_pbm_unpack2<<<(uint32_t)((n + 255) / 256), 256, 0, s>>>(base, (uint32_t)(r & 7), rows, cols, wpr, plane_out);
    return;
  }
  const uint64_t n = (uint64_t)rows * ((cols + 63) / 64);
  const int vec = (reinterpret_cast<uintptr_t>(raster_out) % 8 == 0) && ((cols + 7) / 8) % 8 == 0;
  if (n) k_pbm_pack2<<<(uint32_t)((n + 255) / 256), 256, 0, s>>>(plane_in, rows, cols, wpr, raster_out, vec);
}

void launch_raster_planes(hipStream_t s, const uint8_t* raster, int bpp, uint32_t rows, uint32_t cols, int plane0,
                          int nplanes, uint64_t* planes, uint32_t wpr, uint64_t pitch, int big_endian, bool gray_code,
                          int color_transform, int sample_predict) {
  const uintptr_t r = reinterpret_cast<uintptr_t>(raster);
  if (!pitch) pitch = (uint64_t)cols * bpp;
  const uint32_t selL = big_endian ? 0x07050301u : 0x06040200u, selH = big_endian ? 0x06040200u : 0x07050301u;
  const uint8_t* base = reinterpret_cast<const uint8_t*>(r & ~(uintptr_t)7);
  const uint64_t waves = (uint64_t)rows * ((cols + 4095) / 4096);
  const uint32_t grid = (uint32_t)((waves + 3) / 4);
  if (!grid) return;
  if (bpp == 3 && sample_predict) {  // BIC_OPT_RGB_PREDICT; grid.y: the channel
#define BIC_RPP(G, C, S) \
  k_raster_planes<3, G, C, S><<<dim3(grid, 3), 256, 0, s>>>(base, (uint32_t)(r & 7), rows, cols, plane0, nplanes, planes, \
                                                            wpr, pitch, 0, 0)
#define BIC_RPP2(G, S)                               \
  do {                                               \
    if (color_transform == 1) BIC_RPP(G, 1, S);      \
    else if (color_transform == 2) BIC_RPP(G, 2, S); \
    else BIC_RPP(G, 0, S);                           \
  } while (0)
    if (sample_predict == 1) { if (gray_code) BIC_RPP2(true, 1); else BIC_RPP2(false, 1); }
    else { if (gray_code) BIC_RPP2(true, 2); else BIC_RPP2(false, 2); }
#undef BIC_RPP2
#undef BIC_RPP
    return;
  }
  if (bpp == 3 && color_transform) {  // grid.y: the channel
#define BIC_RPC(G, C) \
  k_raster_planes<3, G, C><<<dim3(grid, 3), 256, 0, s>>>(base, (uint32_t)(r & 7), rows, cols, plane0, nplanes, planes, wpr, \
                                                         pitch, 0, 0)
    if (color_transform == 1) { if (gray_code) BIC_RPC(true, 1); else BIC_RPC(false, 1); }
    else { if (gray_code) BIC_RPC(true, 2); else BIC_RPC(false, 2); }
#undef BIC_RPC
    return;
  }
  if (bpp == 3) {  // grid.y: the channel
    if (gray_code)
      k_raster_planes<3, true><<<dim3(grid, 3), 256, 0, s>>>(base, (uint32_t)(r & 7), rows, cols, plane0, nplanes, planes,
                                                             wpr, pitch, 0, 0);
    else
      k_raster_planes<3, false><<<dim3(grid, 3), 256, 0, s>>>(base, (uint32_t)(r & 7), rows, cols, plane0, nplanes, planes,
                                                              wpr, pitch, 0, 0);
    return;
  }
  if (bpp == 1 && sample_predict) {
#define BIC_RPS(G, S) \
  k_raster_planes<1, G, 0, S><<<grid, 256, 0, s>>>(base, (uint32_t)(r & 7), rows, cols, plane0, nplanes, planes, wpr, pitch, 0, 0)
    if (sample_predict == 1) { if (gray_code) BIC_RPS(true, 1); else BIC_RPS(false, 1); }
    else { if (gray_code) BIC_RPS(true, 2); else BIC_RPS(false, 2); }
#undef BIC_RPS
    return;
  }
#define BIC_RP(B, G) \
  k_raster_planes<B, G><<<grid, 256, 0, s>>>(base, (uint32_t)(r & 7), rows, cols, plane0, nplanes, planes, wpr, pitch, selL, selH)
  if (gray_code) { if (bpp == 1) BIC_RP(1, true); else BIC_RP(2, true); }
  else { if (bpp == 1) BIC_RP(1, false); else BIC_RP(2, false); }
#undef BIC_RP
}

// BIC_OPT_SAMPLE_PREDICT on the way back (one-byte samples), in place on the z samples k_planes_gray /
// k_col_apply_gray have just stored: v(j) = (v(j - 1) + d(j)) & 0xff along the row from v(-1) = 0, d = z (SP 1)
// or its unfolding (SP 2). One wave per (frame, row) walks the row in pieces of 1024 bytes, 16 per lane: the
// dwords' inclusive byte prefix sums (sp_scan4), the dwords' totals down the lane, the lanes' totals scanned
// across the wave by DPP (row_shr 1 2 4 8 inside a row of 16, row_bcast 15 and 31 across the rows), and a
// wave-uniform carry byte into the next piece. A lane whose 16 bytes lie inside the row and are 16-byte aligned
// loads and stores them as one uint4; at the row's end, or with a misaligned row, it takes bytes -- nothing
// past the row's first `cols` bytes is read or written (pitch padding and the gap between frames stay).
template <int SP>
__global__ __launch_bounds__(256) void k_sample_unpredict(uint8_t* __restrict__ gray, uint64_t pitch,
                                                          uint64_t frame_stride, uint32_t rows, uint32_t cols) {
  const uint32_t row = blockIdx.x * 4 + wave_id();
  if (row >= rows) return;  // whole wave
  const uint32_t lane = lane_id();
  uint8_t* p = gray + (uint64_t)blockIdx.y * frame_stride + (uint64_t)row * pitch;
  const bool al = reinterpret_cast<uintptr_t>(p) % 16 == 0;  // (wave-uniform)
  uint32_t carry = 0;  // the sample left of the piece
  for (uint32_t c0 = 0; c0 < cols; c0 += 1024) {
    const uint32_t j = c0 + 16 * lane;
    const bool vec = al && j + 16 <= cols;
    uint32_t x[4] = {0, 0, 0, 0};
    if (vec) {
      const uint4 t = *reinterpret_cast<const uint4*>(p + j);
      x[0] = t.x, x[1] = t.y, x[2] = t.z, x[3] = t.w;
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (j + i < cols) x[i >> 2] |= (uint32_t)p[j + i] << (8 * (i & 3));
    }
    uint32_t run = 0;  // the lane's bytes before the dword, summed
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      x[q] = sp_add4(sp_scan4<SP>(x[q]), run * 0x01010101u);
      run = x[q] >> 24;
    }
    // the lanes' totals, inclusive across the wave (mod 256: the high bits are dropped at the end)
    uint32_t t = run;
    t += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t, 0x111, 0xf, 0xf, true);
    t += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t, 0x112, 0xf, 0xf, true);
    t += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t, 0x114, 0xf, 0xf, true);
    t += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t, 0x118, 0xf, 0xf, true);
    t += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t, 0x142, 0xa, 0xf, false);  // rows 1, 3 += row 0's, 2's total
    t += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t, 0x143, 0xc, 0xf, false);  // rows 2, 3 += rows 0-1's total
    const uint32_t add = ((t - run + carry) & 0xffu) * 0x01010101u;  // what lies left of the lane's bytes
#pragma unroll
    for (int q = 0; q < 4; ++q) x[q] = sp_add4(x[q], add);
    carry = ((uint32_t)__builtin_amdgcn_readlane((int)t, 63) + carry) & 0xffu;
    if (vec) {
      *reinterpret_cast<uint4*>(p + j) = make_uint4(x[0], x[1], x[2], x[3]);
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (j + i < cols) p[j + i] = (uint8_t)(x[i >> 2] >> (8 * (i & 3)));
    }
  }
}

void launch_sample_unpredict(hipStream_t s, int sample_predict, uint8_t* gray, uint64_t pitch, uint64_t frame_stride,
                             uint32_t nframes, uint32_t rows, uint32_t cols) {
  if (!sample_predict || !rows || !cols || !nframes) return;
  const dim3 grid((rows + 3) / 4, nframes);  // (nframes <= 65535)
  if (sample_predict == 1) k_sample_unpredict<1><<<grid, 256, 0, s>>>(gray, pitch, frame_stride, rows, cols);
  else k_sample_unpredict<2><<<grid, 256, 0, s>>>(gray, pitch, frame_stride, rows, cols);
}

// BIC_OPT_RGB_PREDICT on the way back, in place on the interleaved z bytes k_planes_gray<3> / k_col_apply_rgb have
// just stored (both run as with CT 0 then: they store R' G' B' z bytes): per channel c'(j) = (c'(j - 1) + d(j)) & 0xff
// along the row from c'(-1) = 0, d = z (SP 1) or its unfolding (SP 2), then the inverse colour transform CT on
// (R', G', B'). k_sample_unpredict's shape: one wave per (frame, row), pieces of 1024 pixels, 16 pixels = 48 bytes
// per lane -- three uint4 when they lie inside the row and the row is 16-byte aligned, bytes otherwise; nothing
// past the row's first 3 * cols bytes is read or written. The 12 dwords are de-interleaved to four dwords per
// channel (rgb_pick4), scanned (sp_scan4, the totals down the lane), the three channel totals packed into one dword
// and scanned across the wave by the same DPP steps with sp_add4 in the place of + (no carry crosses a byte), the
// exclusive form by a one-lane shift; a wave-uniform packed carry goes into the next piece.
template <int SP, int CT>
__global__ __launch_bounds__(256) void k_rgb_unpredict(uint8_t* __restrict__ rgb, uint64_t pitch, uint64_t frame_stride,
                                                       uint32_t rows, uint32_t cols) {
  const uint32_t row = blockIdx.x * 4 + wave_id();
  if (row >= rows) return;  // whole wave
  const uint32_t lane = lane_id();
  uint8_t* p = rgb + (uint64_t)blockIdx.y * frame_stride + (uint64_t)row * pitch;
  const bool al = reinterpret_cast<uintptr_t>(p) % 16 == 0;  // (wave-uniform)
  const uint64_t nb = 3ull * cols;                             // the row's bytes
  uint32_t carry = 0;  // the pixel left of the piece: R' | G' << 8 | B' << 16
  for (uint32_t c0 = 0; c0 < cols; c0 += 1024) {
    const uint32_t j = c0 + 16 * lane;
    const uint64_t jb = 3ull * j;
    const bool vec = al && j + 16 <= cols;
    uint32_t x[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) x[q] = 0;
    if (vec) {
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const uint4 t = reinterpret_cast<const uint4*>(p + jb)[q];
        x[4 * q] = t.x, x[4 * q + 1] = t.y, x[4 * q + 2] = t.z, x[4 * q + 3] = t.w;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 48; ++i)
        if (jb + i < nb) x[i >> 2] |= (uint32_t)p[jb + i] << (8 * (i & 3));
    }
    uint32_t ch[3][4], tot = 0;  // per channel: the 16 pixels' bytes; the lane's three totals, packed
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      uint32_t run = 0;  // the lane's bytes of the channel before the dword, summed
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t z = rgb_pick4(x[3 * q], x[3 * q + 1], x[3 * q + 2], rgb_sel1(c), rgb_sel2(c));
        ch[c][q] = sp_add4(sp_scan4<SP>(z), run * 0x01010101u);
        run = ch[c][q] >> 24;
      }
      tot |= run << (8 * c);
    }
    // the lanes' packed totals, inclusive across the wave, byte-wise mod 256
    uint32_t t = tot;
    t = sp_add4(t, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t, 0x111, 0xf, 0xf, true));
    t = sp_add4(t, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t, 0x112, 0xf, 0xf, true));
    t = sp_add4(t, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t, 0x114, 0xf, 0xf, true));
    t = sp_add4(t, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t, 0x118, 0xf, 0xf, true));
    t = sp_add4(t, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t, 0x142, 0xa, 0xf, false));  // rows 1, 3 += row 0's, 2's
    t = sp_add4(t, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t, 0x143, 0xc, 0xf, false));  // rows 2, 3 += rows 0-1's
    // what lies left of the lane's pixels: lane - 1's inclusive totals (0 for lane 0) plus the carry
    const uint32_t left = sp_add4((uint32_t)__builtin_amdgcn_update_dpp(0, (int)t, 0x138, 0xf, 0xf, true), carry);
    carry = sp_add4((uint32_t)__builtin_amdgcn_readlane((int)t, 63), carry);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const uint32_t add = ((left >> (8 * c)) & 0xffu) * 0x01010101u;
#pragma unroll
      for (int q = 0; q < 4; ++q) ch[c][q] = sp_add4(ch[c][q], add);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if constexpr (CT != 0) {
        ch[0][q] = ct_inverse4<CT>(ch[0][q], ch[1][q]);
        ch[2][q] = ct_inverse4<CT>(ch[2][q], ch[1][q]);
      }
      rgb_interleave4(ch[0][q], ch[1][q], ch[2][q], x[3 * q], x[3 * q + 1], x[3 * q + 2]);
    }
    if (vec) {
#pragma unroll
      for (int q = 0; q < 3; ++q)
        reinterpret_cast<uint4*>(p + jb)[q] = make_uint4(x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]);
    } else {
#pragma unroll
      for (int i = 0; i < 48; ++i)
        if (jb + i < nb) p[jb + i] = (uint8_t)(x[i >> 2] >> (8 * (i & 3)));
    }
  }
}

void launch_rgb_unpredict(hipStream_t s, int rgb_predict, int color_transform, uint8_t* rgb, uint64_t pitch,
                          uint64_t frame_stride, uint32_t nframes, uint32_t rows, uint32_t cols) {
  if (!rgb_predict || !rows || !cols || !nframes) return;
  const dim3 grid((rows + 3) / 4, nframes);  // (nframes <= 65535)
#define BIC_RU(S, C) k_rgb_unpredict<S, C><<<grid, 256, 0, s>>>(rgb, pitch, frame_stride, rows, cols)
#define BIC_RU2(S)                                \
  do {                                            \
    if (color_transform == 1) BIC_RU(S, 1);       \
    else if (color_transform == 2) BIC_RU(S, 2);  \
    else BIC_RU(S, 0);                            \
  } while (0)
  if (rgb_predict == 1) BIC_RU2(1);
  else BIC_RU2(2);
#undef BIC_RU2
#undef BIC_RU
}

}  // namespace bic
