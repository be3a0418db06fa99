// bic_fused.h -- what the row encoders for rows of up to 256 words (16384 columns) share: a lane's
// codewords for one word (encode_word*), the LDS row images and their write-out, the residual rows
// read back from the EG stream (eg_src_*), the rows written straight to global memory (row_global),
// the kernels' argument block (FusedArgs, make_fused_args) and the launches' template dispatch.
// Included by bic_fused.hip (the staged encoder, the default) and bic_fused_lookback.hip.
// Semantics are those of bic_kernels.hip (GolombCoder.cpp:13-34, eg.cpp:20-37, pred.cpp:3-15); the
// difference is the schedule. Every codeword is computed ONCE: each lane turns its word into a
// register string (first codeword's binary part, its unary zeros, then <= 128 bits), or -- when the k
// bounds prove k = 0 for every codeword of the word -- copies the word's bits (a k = 0 codeword is
// exactly the run's zeros and its 1); constant k = 1..3 words go byte by byte through precomputed
// tables. Whole 64-bit words go to HBM with plain stores and the (at most two) words shared with
// neighbouring rows go to a fragment table that the fixup kernel combines (no atomics on the
// output, no pre-zeroing of the output).
#pragma once
#include "bic_device.h"
#include "bic_k1pi.h"  // the k = 1 rows' backward-parity encoder (host-compilable: tests/cpp/k1pi_check.cpp)
#include "bic_kstat.h"

#include <type_traits>

namespace bic {

#ifdef BIC_STAMPS  // diagnostic build only (make stamps): per-wave phase clocks, never in the product
// (defined here: the stamps build compiles bic_fused.hip and bic_fused_lookback.hip as one unit, so
// that the kernels of both write this one array)
__device__ unsigned long long g_stamps[1 << 22];
// BIC_KNOWN=1 (diagnostic): replay the tile prefixes recorded by the previous normal launch
// instead of looking them back, to measure what the look-back waits cost
__device__ unsigned long long g_known[2][1 << 17];
#define STAMP(slot)                                                                        \
  do {                                                                                     \
    const unsigned long long t_ = __builtin_amdgcn_s_memtime();                            \
    if (lane == 0 && (uint64_t)id * 8 + (slot) < (1u << 21)) g_stamps[(uint64_t)id * 8 + (slot)] = t_; \
  } while (0)
// k_row_walk's phases (slots 4-7 of the row: entry, residual word loaded, length walked, stored), on
// the 100 MHz clock every XCD shares (s_memrealtime), waiting for the phase's loads first
#define WSTAMP(slot)                                                                               \
  do {                                                                                             \
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                                    \
    const unsigned long long t_ = __builtin_amdgcn_s_memrealtime();                                \
    if (threadIdx.x == 0 && (uint64_t)id * 8 + (slot) < (1u << 21)) g_stamps[(uint64_t)id * 8 + (slot)] = t_; \
  } while (0)
// k_scan_rows' phases per workgroup (slots of g_stamps from 1 << 21: ONES scan, then LEN scan)
#define SSTAMP(slot)                                                                              \
  do {                                                                                            \
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                                   \
    const unsigned long long t_ = __builtin_amdgcn_s_memrealtime();                               \
    if (threadIdx.x == 0) g_stamps[(1u << 21) + (ONES ? 0u : 8192u) + blockIdx.x * 8u + (slot)] = t_; \
  } while (0)
// the class launch's phases (tools/k01_stamps.py), 4 slots per index: per k = 1 row (YSTAMP, index
// 1 << 18 + its row id; slots 0-3: entry, words assembled, image built, stored), per wave of k_emit_k01
// (index 1 << 19 + 8192 + its wave; slots 0-3: entry, k = 0 rows done, -, exit)
#define XSTAMP(idx, slot)                                                                          \
  do {                                                                                             \
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                                    \
    const unsigned long long t_ = __builtin_amdgcn_s_memrealtime();                                \
    if (lane_id() == 0 && (uint64_t)(idx) * 4 + (slot) < (1u << 22)) g_stamps[(uint64_t)(idx) * 4 + (slot)] = t_; \
  } while (0)
// (the same without draining the memory counters first: the instruction's issue time)
#define YSTAMP(idx, slot)                                                                          \
  do {                                                                                             \
    const unsigned long long t_ = __builtin_amdgcn_s_memrealtime();                                \
    if (lane_id() == 0 && (uint64_t)(idx) * 4 + (slot) < (1u << 22)) g_stamps[(uint64_t)(idx) * 4 + (slot)] = t_; \
  } while (0)
#else
#define XSTAMP(idx, slot) \
  do {                    \
  } while (0)
#define YSTAMP(idx, slot) \
  do {                    \
  } while (0)
#define STAMP(slot) \
  do {              \
  } while (0)
#define WSTAMP(slot) \
  do {               \
  } while (0)
#define SSTAMP(slot) \
  do {               \
  } while (0)
#endif

constexpr int kTileRows = 16;  // rows (= waves) per workgroup tile (C3: 666 us vs 677 at 8 rows)
constexpr int kGImg = 684;    // u32 words of Golomb row image per wave (21760 bits; with the EG image and
                              // the k = 1, 2 byte tables 4 workgroups (32 waves) fit one CU's LDS)
constexpr int kEImg = 520;    // u32 words of EG row image per wave (cols <= 16384)
constexpr int kPad = 4;       // zeroed words after an image's end (get64 reads ahead)
constexpr uint32_t kK1Table = 512u;  // the k = 1 rows' table in the u32 byte tables (k1_pi, the [pi][byte] table)
// k_emit_known's k = 1 rows (C4, C2, predict) go by encode_word_k1b, table 0 (C4 0.268 ms against 0.283
// with the backward parity's strided lanes)
constexpr uint32_t kKnownTable = 0u;

// One lane's codewords for one residual word.
struct LaneEnc {
  uint32_t head, k0, z;  // first codeword: k0-bit binary part, then z unary zeros
  uint64_t t0, t1;       // the rest (starting with the first codeword's '1'), MSB-first
  uint32_t tlen;
  uint32_t len;          // total bits
  bool lng;              // rest longer than 128 bits: placed by re-iteration
#ifdef BIC_STAMPS
  uint32_t path;         // diagnostic: 1 copy mode, 2 byte table, 3 per-codeword loop
#endif
};

__device__ __forceinline__ void tail_put(LaneEnc& e, uint64_t cw, uint32_t nb) {  // nb 1..64
  const uint32_t pos = e.tlen;
  e.tlen = pos + nb;
  if (pos + nb > 128) { e.lng = true; return; }
  const uint32_t sh = 128 - pos - nb;
  if (sh >= 64) {
    e.t0 |= cw << (sh - 64);
  } else {
    e.t1 |= cw << sh;
    if (sh + nb > 64) e.t0 |= cw >> (64 - sh);
  }
}

// Byte tables for words whose codewords all share one k in 1..3 (built on the host,
// bic_kernels.hip build_byte_lut): for a byte v != 0, the codewords that lie wholly inside the
// byte (after its first 1) as one right-aligned pattern R of lr bits, plus the byte's leading (t)
// and trailing (tz) zeros. k = 1, 2: packed u32 R | lr << 21 | t << 26 | tz << 29, staged in LDS
// by the encoder; k = 3: u64 R | lr << 32 | t << 40 | tz << 44 from global memory.
struct ByteTables {
  const uint32_t* t12;  // [2][256]
  const uint64_t* t3;   // [256]
};
__device__ __forceinline__ void tail_put_n(LaneEnc& e, uint64_t cw, uint32_t nb) {
  if (nb) tail_put(e, cw, nb);
}

// STR = false computes only e.len (the length pass of the two-pass encoder).
template <bool STR = true>
__device__ __forceinline__ LaneEnc encode_word(uint64_t x, uint32_t w, uint32_t n, int jp, uint32_t arow,
                                               bool eol, uint32_t cols, ByteTables lut) {
  LaneEnc e{};
  if (!x && !eol) return e;
  if (x && n) {
    // A never decreases and n only grows along the word, so every codeword's k lies between
    // k(n_last, A_first) and k(n_first, A_last); when the two agree, k is the same throughout.
    const uint32_t m = (uint32_t)__popcll(x);
    const uint32_t plast = w * 64 + 63 - (uint32_t)__builtin_ctzll(x);
    const uint32_t aup = arow + plast - (n + m - 1);  // >= A of the last codeword (and = A of the EOL's)
    const uint32_t afirst = arow + (uint32_t)(jp + 1) - n;
    const uint32_t khi = golomb_k(n, aup);
    const uint32_t klo = golomb_k(n + m - 1 + (eol ? 1u : 0u), afirst);
    if (khi == klo && khi == 0) {
      // k = 0: a codeword is its run's zeros and the 1 -- the word's bits verbatim
      e.z = w * 64 - (uint32_t)(jp + 1);
      e.t0 = x;
      if (!eol) {
        e.tlen = plast - w * 64 + 1;
      } else {
        const uint32_t p = cols - w * 64;  // the EOL codeword's '1'
        if (p < 64) e.t0 |= BIC_MSB >> p; else e.t1 = BIC_MSB;
        e.tlen = p + 1;
      }
      e.len = e.z + e.tlen;
#ifdef BIC_STAMPS
      e.path = 1;
#endif
      return e;
    }
    if (khi == klo && khi <= 3) {
#ifdef BIC_STAMPS
      e.path = 2;
#endif
      const uint32_t k = khi, kmask = (1u << k) - 1u;
      uint32_t c = w * 64 - (uint32_t)(jp + 1);  // zeros of the open run
      bool first = true;
      const uint32_t* T = lut.t12 + (k - 1) * 256;
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const uint32_t v = (uint32_t)(x >> (56 - 8 * b)) & 0xffu;
        if (v) {
          uint32_t R, lr, t, tz;
          if (k <= 2) {
            const uint32_t en = T[v];
            R = en & 0x1fffffu;
            lr = (en >> 21) & 31u;
            t = (en >> 26) & 7u;
            tz = en >> 29;
          } else {
            const uint64_t en = lut.t3[v];
            R = (uint32_t)en;
            lr = (uint32_t)(en >> 32) & 63u;
            t = (uint32_t)(en >> 40) & 15u;
            tz = (uint32_t)(en >> 44) & 15u;
          }
          const uint32_t sr = c + t, q = sr >> k, bin = sr & kmask;
          if constexpr (STR) {
            if (first) {
              e.head = bin;
              e.k0 = k;
              e.z = q;
              tail_put(e, (1ull << lr) | R, 1 + lr);
              first = false;
            } else {
              const uint32_t nb = k + q + 1;  // sr <= 63 here
              if (nb + lr <= 64) {
                tail_put(e, ((((uint64_t)bin << (q + 1)) | 1ull) << lr) | R, nb + lr);
              } else {
                tail_put(e, ((uint64_t)bin << (q + 1)) | 1ull, nb);
                tail_put_n(e, R, lr);
              }
            }
          }
          e.len += k + q + 1 + lr;
          c = tz;
        } else {
          c += 8;
        }
      }
      if (eol) {  // the row's trailing zeros (pad columns excluded)
        const uint32_t sr = c - (w * 64 + 64 - cols), q = sr >> k;
        if constexpr (STR) tail_put(e, ((uint64_t)(sr & kmask) << (q + 1)) | 1ull, k + q + 1);
        e.len += k + q + 1;
      }
      return e;
    }
  }
  // k changes inside the word (or n = 0, the plane's first sample): one codeword at a time, the
  // word's first one (binary part and unary zeros cut off: head, z) peeled off the loop, and
  // A = arow + jp + 1 - n carried (A' = A + s as n' = n + 1). (Byte by byte with per-byte k bounds
  // measured slower.)
#ifdef BIC_STAMPS
  e.path = 3;
#endif
  uint32_t A = arow + (uint32_t)(jp + 1) - n;
  {
    uint32_t s;
    int j;
    if (x) {
      const int cz = __builtin_clzll(x);
      x ^= BIC_MSB >> cz;
      j = (int)(w * 64) + cz;
      s = (uint32_t)(j - jp - 1);
    } else {  // (eol: the row's end-of-row codeword alone)
      j = (int)cols;
      s = cols - 1 - (uint32_t)jp;
      eol = false;
    }
    const uint32_t k = golomb_k_state(n, A);
    const uint32_t q = s >> k;
    if constexpr (STR) {
      e.head = s & ((1u << k) - 1u);
      e.k0 = k;
      e.z = q;
      tail_put(e, 1, 1);
    }
    e.len += k + q + 1;
    A += s;
    ++n;
    jp = j;
  }
  while (x) {  // (n >= 1 from here; s <= 62: k + q + 1 <= 64)
    const int cz = __builtin_clzll(x);
    x ^= BIC_MSB >> cz;
    const int j = (int)(w * 64) + cz;
    const uint32_t s = (uint32_t)(j - jp - 1);
    const uint32_t k = golomb_k(n, A), q = s >> k;
    if constexpr (STR) tail_put(e, ((uint64_t)(s & ((1u << k) - 1u)) << (q + 1)) | 1ull, k + q + 1);
    e.len += k + q + 1;
    A += s;
    ++n;
    jp = j;
  }
  if (eol) {
    const uint32_t s = cols - 1 - (uint32_t)jp;
    const uint32_t k = golomb_k(n, A), q = s >> k;
    if constexpr (STR) tail_put(e, ((uint64_t)(s & ((1u << k) - 1u)) << (q + 1)) | 1ull, k + q + 1);
    e.len += k + q + 1;
  }
  return e;
}

// OR the nb (1..64) low bits of v into the 128-bit MSB-first string (t0, t1) at bit pos
// (pos + nb <= 128 whenever v != 0), branch-free.
__device__ __forceinline__ void or128(uint64_t& t0, uint64_t& t1, uint64_t v, uint32_t pos, uint32_t nb) {
  const uint32_t end = pos + nb;
  const uint64_t p0 = end <= 64 ? v << ((64 - end) & 63) : v >> ((end - 64) & 63);
  t0 |= pos < 64 ? p0 : 0ull;
  t1 |= end > 64 ? v << ((128 - end) & 63) : 0ull;
}

// encode_word for a row whose codewords all have k = 1 (kK1Row): no k bounds, no sample count, no
// divergent paths. The first codeword (binary part in head, its q zeros in z) is cut off as in
// encode_word; the rest goes byte by byte through the k = 1 table: byte i's first 1 closes the open
// run (c zeros before the byte + t): its binary bit, q zeros, then the table's '1' + R -- one
// pattern appended to a right-aligned 128-bit accumulator (two 64-bit shifts and an or); the word's
// first byte appends '1' + R only. <= 128 bits except through long runs (then lng: placed by
// emit_word_k1).
__device__ __forceinline__ void acc_put(uint64_t& hi, uint64_t& lo, uint64_t pat, uint32_t nb) {  // nb 1..63
  hi = (hi << nb) | (lo >> (64 - nb));
  lo = (lo << nb) | pat;
}
__device__ __forceinline__ void acc_zeros(uint64_t& hi, uint64_t& lo, uint32_t nb) {  // nb <= 128
  if (nb >= 64) {
    hi = lo;
    lo = 0;
    nb -= 64;
  }
  if (nb) {
    hi = (hi << nb) | (lo >> (64 - nb));
    lo <<= nb;
  }
}
// append bin, q zeros, then pat (np bits, 1..63): total 1 + q + np bits
__device__ __forceinline__ void acc_codeword(uint64_t& hi, uint64_t& lo, uint32_t& p, uint32_t bin, uint32_t q,
                                             uint64_t pat, uint32_t np) {
  const uint32_t nb = 1 + q + np;
  if (p + nb <= 128) {
    if (nb <= 63) {
      acc_put(hi, lo, ((uint64_t)bin << (nb - 1)) | pat, nb);
    } else {
      acc_put(hi, lo, bin, 1);
      acc_zeros(hi, lo, q);
      acc_put(hi, lo, pat, np);
    }
  }
  p += nb;
}

__device__ __forceinline__ LaneEnc encode_word_k1(uint64_t x, uint32_t w, int jp, bool eol, uint32_t cols,
                                                  const uint32_t* T1) {
  LaneEnc e{};
  e.k0 = 1;
  uint32_t c = w * 64 - (uint32_t)(jp + 1);  // zeros of the open run
  if (!x) {
    if (eol) {
      const uint32_t s = cols - 1 - (uint32_t)jp;
      e.head = s & 1u;
      e.z = s >> 1;
      e.t0 = BIC_MSB;
      e.tlen = 1;
      e.len = 2 + e.z;
    }
    return e;
  }
  const uint32_t bf = (uint32_t)__builtin_clzll(x);
  const uint32_t s1 = c + bf, fb = bf >> 3;
  e.head = s1 & 1u;
  e.z = s1 >> 1;
  uint64_t hi = 0, lo = 0;
  uint32_t p = 0;
#pragma unroll
  for (uint32_t i = 0; i < 8; ++i) {
    const uint32_t v = (uint32_t)(x >> (56 - 8 * i)) & 0xffu;
    if (v) {
      const uint32_t en = T1[v];
      const uint32_t R = en & 0x1fffffu, lr = (en >> 21) & 31u, t = (en >> 26) & 7u, tz = en >> 29;
      const uint64_t pat = (1ull << lr) | R;
      if (i == fb) {
        acc_put(hi, lo, pat, lr + 1);
        p += lr + 1;
      } else {
        const uint32_t s = c + t;
        acc_codeword(hi, lo, p, s & 1u, s >> 1, pat, lr + 1);
      }
      c = tz;
    } else {
      c += 8;
    }
  }
  if (eol) {  // the row's trailing zeros (pad columns excluded)
    const uint32_t s = c - (w * 64 + 64 - cols);
    acc_codeword(hi, lo, p, s & 1u, s >> 1, 1ull, 1);
  }
  e.tlen = p;
  e.len = 1 + e.z + p;
  e.lng = p > 128;
  if (!e.lng) {  // left-align the p-bit string
    const uint32_t sh = 128 - p;
    if (sh >= 64) {
      e.t0 = lo << (sh - 64);
      e.t1 = 0;
    } else if (sh) {
      e.t0 = (hi << sh) | (lo >> (64 - sh));
      e.t1 = lo << sh;
    } else {
      e.t0 = hi;
      e.t1 = lo;
    }
  }
  return e;
}

// encode_word_k1 without branches: every byte runs the same instructions (its codeword from the k = 1
// table whether or not it holds a 1, selected in or out), so a wave never executes divergent paths.
// Inside a word a run's zeros are < 64 + 7, so a byte's pattern (bin, q zeros, '1', R) is < 64 bits;
// out-of-range shift amounts of unselected bytes are clamped.
__device__ __forceinline__ LaneEnc encode_word_k1b(uint64_t x, uint32_t w, int jp, bool eol, uint32_t cols,
                                                   const uint32_t* T1) {
  LaneEnc e{};
  e.k0 = 1;
  uint32_t c = w * 64 - (uint32_t)(jp + 1);  // zeros of the open run
  if (!x) {
    if (eol) {
      const uint32_t s = cols - 1 - (uint32_t)jp;
      e.head = s & 1u;
      e.z = s >> 1;
      e.t0 = BIC_MSB;
      e.tlen = 1;
      e.len = 2 + e.z;
    }
    return e;
  }
  const uint32_t bf = (uint32_t)__builtin_clzll(x), fb = bf >> 3;
  const uint32_t s1 = c + bf;
  e.head = s1 & 1u;
  e.z = s1 >> 1;
  uint64_t hi = 0, lo = 0;
  uint32_t p = 0;
#pragma unroll
  for (uint32_t i = 0; i < 8; ++i) {
    const uint32_t v = (uint32_t)(x >> (56 - 8 * i)) & 0xffu;
    const uint32_t en = T1[v];
    const uint32_t R = en & 0x1fffffu, lr = (en >> 21) & 31u, t = (en >> 26) & 7u, tz = en >> 29;
    const uint32_t sr = c + t;
    const uint32_t q1 = min((sr >> 1) + 1u, 62u - lr);  // the '1' after q zeros, then R
    const uint64_t tail = (1ull << lr) | R;
    const bool first = i == fb;
    const uint64_t pat = first ? tail : ((uint64_t)(sr & 1u) << (q1 + lr)) | tail;
    const uint32_t nb = first ? lr + 1 : q1 + 1 + lr;  // 1..63
    const bool act = v != 0;
    const uint64_t nhi = (hi << nb) | (lo >> (64 - nb));
    const uint64_t nlo = (lo << nb) | pat;
    hi = act ? nhi : hi;
    lo = act ? nlo : lo;
    p += act ? nb : 0u;
    c = act ? tz : c + 8;
  }
  if (eol) {  // the row's trailing zeros (pad columns excluded): bin, q zeros, '1' (< 64 bits)
    const uint32_t sr = c - (w * 64 + 64 - cols), q1 = (sr >> 1) + 1;
    const uint32_t nb = q1 + 1;
    const uint64_t pat = ((uint64_t)(sr & 1u) << q1) | 1ull;
    hi = (hi << nb) | (lo >> (64 - nb));
    lo = (lo << nb) | pat;
    p += nb;
  }
  e.tlen = p;
  e.len = 1 + e.z + p;
  e.lng = p > 128;
  if (!e.lng) {  // left-align the p-bit string
    const uint32_t sh = 128 - p;
    if (sh >= 64) {
      e.t0 = lo << (sh - 64);
      e.t1 = 0;
    } else if (sh) {
      e.t0 = (hi << sh) | (lo >> (64 - sh));
      e.t1 = lo << sh;
    } else {
      e.t0 = hi;
      e.t1 = lo;
    }
  }
  return e;
}

__device__ __forceinline__ void place128_64(uint64_t* img, uint32_t off, uint64_t A, uint64_t B, uint32_t tlen) {
  if (!tlen) return;
  const uint32_t i = off >> 6, sh = off & 63;
  uint64_t D0 = A, D1 = B, D2 = 0;
  if (sh) {
    D0 = A >> sh;
    D1 = (A << (64 - sh)) | (B >> sh);
    D2 = B << (64 - sh);
  }
  const uint32_t nw = (sh + tlen + 63) >> 6;
  lds_or64(img, i, D0);
  if (nw > 1) lds_or64(img, i + 1, D1);
  if (nw > 2) lds_or64(img, i + 2, D2);
}
struct LdsSink64 {
  uint64_t* buf;
  uint32_t idx;
  uint64_t cur;
  __device__ __forceinline__ void flush() {
    if (cur) atomicOr(reinterpret_cast<unsigned long long*>(buf + idx), (unsigned long long)cur);
    cur = 0;
  }
  __device__ __forceinline__ void orw(uint32_t i, uint64_t v) {
    if (i != idx) {
      flush();
      idx = i;
    }
    cur |= v;
  }
  __device__ __forceinline__ void put(uint32_t off, uint32_t v, uint32_t nb) {  // nb <= 32
    const uint32_t i = off >> 6, sh = off & 63;
    if (sh + nb <= 64) {
      orw(i, (uint64_t)v << (64 - sh - nb));
    } else {
      orw(i, (uint64_t)v >> (sh + nb - 64));
      orw(i + 1, (uint64_t)v << (128 - sh - nb));
    }
  }
  __device__ __forceinline__ void bit(uint32_t off) { orw(off >> 6, BIC_MSB >> (off & 63)); }
};

// emit_word for k = 1 rows (the lng fallback of encode_word_k1).
template <typename Sink, typename Off>
__device__ __forceinline__ void emit_word_k1(Sink& sk, Off off, uint64_t x, uint32_t w, int jp, bool eol, uint32_t cols) {
  for (;;) {
    int j;
    uint32_t s;
    if (x) {
      const int cz = __builtin_clzll(x);
      x ^= BIC_MSB >> cz;
      j = (int)(w * 64) + cz;
      s = (uint32_t)(j - jp - 1);
    } else if (eol) {
      j = (int)cols;
      s = cols - 1 - (uint32_t)jp;
      eol = false;
    } else {
      break;
    }
    if (s & 1u) sk.put(off, 1u, 1);
    sk.bit(off + 1 + (s >> 1));
    off += 2 + (s >> 1);
    jp = j;
  }
}

// Emit one word's codewords through a sink at bit offset `off` (fallback paths).
template <typename Sink, typename Off>
__device__ __forceinline__ void emit_word(Sink& sk, Off off, uint64_t x, uint32_t w, uint32_t n, int jp,
                                          uint32_t arow, bool eol, uint32_t cols) {
  for (;;) {
    int j;
    uint32_t s;
    if (x) {
      const int cz = __builtin_clzll(x);
      x ^= BIC_MSB >> cz;
      j = (int)(w * 64) + cz;
      s = (uint32_t)(j - jp - 1);
    } else if (eol) {
      j = (int)cols;
      s = cols - 1 - (uint32_t)jp;
      eol = false;
    } else {
      break;
    }
    const uint32_t k = golomb_k_state(n, arow + (uint32_t)(jp + 1) - n);
    if (k) {
      const uint32_t bin = s & ((1u << k) - 1u);
      if (bin) sk.put(off, bin, k);
    }
    sk.bit(off + k + (s >> k));
    off += k + (s >> k) + 1;
    ++n;
    jp = j;
  }
}

__device__ __forceinline__ void lds_or(uint32_t* img, uint32_t i, uint32_t v) {
  if (v) atomicOr(&img[i], v);
}

// OR tlen (<= 128) bits (A:B, MSB-first) into the image at bit `off`.
__device__ __forceinline__ void place128(uint32_t* img, uint32_t off, uint64_t A, uint64_t B, uint32_t tlen) {
  if (!tlen) return;
  const uint32_t i = off >> 5, sh = off & 31;
  uint64_t D0 = A, D1 = B, D2 = 0;
  if (sh) {
    D0 = A >> sh;
    D1 = (A << (64 - sh)) | (B >> sh);
    D2 = B << (64 - sh);
  }
  const uint32_t nw = (sh + tlen + 31) >> 5;
  lds_or(img, i, (uint32_t)(D0 >> 32));
  if (nw > 1) lds_or(img, i + 1, (uint32_t)D0);
  if (nw > 2) lds_or(img, i + 2, (uint32_t)(D1 >> 32));
  if (nw > 3) lds_or(img, i + 3, (uint32_t)D1);
  if (nw > 4) lds_or(img, i + 4, (uint32_t)(D2 >> 32));
}

__device__ __forceinline__ void place_small(uint32_t* img, uint32_t off, uint32_t v, uint32_t nb) {
  if (!nb || !v) return;
  const uint32_t i = off >> 5, sh = off & 31;
  if (sh + nb <= 32) {
    lds_or(img, i, v << (32 - sh - nb));
  } else {
    lds_or(img, i, v >> (sh + nb - 32));
    lds_or(img, i + 1, v << (64 - sh - nb));
  }
}

// 64 image bits starting at bit a (a may be negative: leading zeros).
__device__ __forceinline__ uint64_t raw64(const uint32_t* img, int64_t a) {
  if (a <= -64) return 0;
  const int64_t b = a < 0 ? 0 : a;
  const uint32_t i = (uint32_t)(b >> 5), sh = (uint32_t)(b & 31);
  const uint64_t hi = ((uint64_t)img[i] << 32) | img[i + 1];
  const uint64_t v = sh ? (hi << sh) | (img[i + 2] >> (32 - sh)) : hi;
  return a < 0 ? v >> (-a) : v;
}

// Same, of the image with a '0' inserted at position ins (ins < 0: no insertion).
__device__ __forceinline__ uint64_t img64(const uint32_t* img, int64_t a, int64_t ins) {
  if (ins < 0 || ins >= a + 64) return raw64(img, a);
  const uint64_t Y = raw64(img, a - 1);
  if (ins < a) return Y;
  const uint32_t q = (uint32_t)(ins - a);
  const uint64_t X = raw64(img, a);
  const uint64_t hi = q ? ~(~0ull >> q) : 0ull;
  const uint64_t lo = q == 63 ? 0ull : (~0ull >> (q + 1));
  return (X & hi) | (Y & lo);
}

// Is output word w entirely inside the row's bit range [G, G+L)?
__device__ __forceinline__ bool word_complete(uint64_t w, uint64_t G, uint64_t L) {
  return w * 64 >= G && w * 64 + 64 <= G + L;
}

// A word the row shares with a neighbouring row: into the fragment table (k_fixup combines them).
__device__ __forceinline__ void put_shared(uint64_t* out, uint64_t wi, uint64_t* frag, int which, uint64_t v) {
  (void)out;
  (void)wi;
  frag[which] = v;
}

// Write a row image of L bits to absolute bit G of out (threads tid of nt: a wave's lanes by
// default): whole words with plain stores, the
// first/last word (when shared with another row) into frag[0]/frag[1]. Output word t of the row
// holds image bits [64t - G%64, 64t - G%64 + 64): the bit shift inside the image's u32 words is
// the same for every t, so the common case (no inserted bit) is three LDS reads and a funnel
// shift per word, branch-free and independent across iterations.
__device__ __forceinline__ void write_row(const uint32_t* img, uint64_t L, uint64_t G, int64_t ins,
                                          uint64_t* out, uint64_t* frag, uint32_t tid = lane_id(), uint32_t nt = 64) {
  const uint64_t w0 = G >> 6, w1 = (G + L - 1) >> 6, nw = w1 - w0 + 1;
  if (ins >= 0) {
    for (uint64_t t = tid; t < nw; t += nt) {
      const uint64_t wb = (w0 + t) * 64;
      const uint64_t v = img64(img, (int64_t)wb - (int64_t)G, ins);
      if (word_complete(w0 + t, G, L)) out[w0 + t] = bswap64(v);
      else put_shared(out, w0 + t, frag, t == 0 ? 0 : 1, v);
    }
    return;
  }
  const uint32_t g = (uint32_t)(G & 63);
  for (uint32_t t = tid; t < (uint32_t)nw; t += nt) {
    const int32_t a = (int32_t)(64 * t) - (int32_t)g;  // first image bit of output word t
    const uint32_t b = a < 0 ? 0u : (uint32_t)a;
    const uint32_t i = b >> 5, sh = b & 31;
    const uint64_t hi = ((uint64_t)img[i] << 32) | img[i + 1];
    uint64_t v = (hi << sh) | ((uint64_t)img[i + 2] >> (32 - sh));
    if (a < 0) v >>= -a;
    if (t != 0 && t != (uint32_t)nw - 1) out[w0 + t] = bswap64(v);
    else if (word_complete(w0 + t, G, L)) out[w0 + t] = bswap64(v);
    else put_shared(out, w0 + t, frag, t == 0 ? 0 : 1, v);
  }
}

// glen[] flags of the staged encoder (set by the prefix kernels, read-only afterwards: every
// consumer masks them off, so the two emission launches never write glen)
constexpr uint64_t kK0Row = 1ull << 63;  // every codeword of the row has k = 0
constexpr uint64_t kK1Row = 1ull << 62;  // every codeword of the row has k = 1
constexpr uint64_t kLenMask = (1ull << 60) - 1;

struct FusedArgs {
  Geom g;
  const uint64_t* planes;
  const uint64_t* lut;  // byte tables (see ByteTables): [256] u64 for k = 3, then [2][256] u32
  uint32_t* counter;   // zeroed per launch
  uint64_t* ones_rec;  // zeroed per launch
  uint64_t* bits_rec;  // zeroed per launch
  uint64_t *gboff, *glen, *gfrag, *gslow;
  uint64_t *eboff, *elen, *efrag;
  uint32_t* row_o;     // two-pass / staged encoders: ones of the plane before each row
  uint32_t* sones;     // staged encoder: per (plane, row, strip) 1-counts and k statistics
  int4* krec;
  uint32_t* kpos;
  uint32_t ns;         // strips per row
  uint32_t* walk_ids;  // staged encoder: rows k_row_walk walks (count in counter[2])
  uint32_t* rest_ids;  // staged encoder: rows the REST emit launch writes (count in counter[3])
  uint32_t* slow_n;    // number of rows k_rows_global must write (zeroed per launch)
  uint64_t* slow_ids;  // their row ids
  uint64_t* out_g;
  uint64_t slot_g;
  uint64_t* bits_g;
  uint64_t* out_e;
  uint64_t slot_e;
  uint64_t* bits_e;
  uint32_t* flags;
  // packed output (CoderOut::off): per-plane totals of residual 1s (ONES scan), the
  // planes' packed start words (k_plane_bases) and EG start bits; ebase null: slot mode
  uint64_t* pones;
  uint64_t* gbase;
  uint64_t* ebase;
  uint64_t* off_g;
  uint64_t* off_e;
  uint64_t* index;  // FusedRequest::index
  // bic_encode_gray without planes (FusedRequest::eg_src): the count pass wrote the EG stream in its
  // uniform layout and the residual rows are read back from it (null: residual from planes)
  const uint64_t* esrc;
  uint64_t* efix;
  uint64_t* cls;  // FusedArena::cls (EG source: the class emission kernels' row lists, (id, offset)
                  // pairs; the class kernels store as unsigned long long, a type apart, so the compiler
                  // keeps these loads on the scalar cache: no wait on the vector memory counter)
  uint64_t* sink;     // FusedArena::sink
  uint32_t* walk_o;   // FusedArena::walk_o (the walked rows' row_o)
#ifdef BIC_STAMPS
  int known;
#endif
};

// A row's absolute Golomb bit offset: gboff holds it relative to the plane's slot start (LEN scan);
// packed output moves the plane to its packed start word gbase[plane]
__device__ __forceinline__ uint64_t gb_abs(const FusedArgs& a, uint64_t id, uint32_t plane) {
  const uint64_t G = a.gboff[id];
  return a.off_g ? G - (uint64_t)plane * a.slot_g * 64 + a.gbase[plane] * 64 : G;
}

// ---- residual rows read back from the EG stream (FusedArgs::esrc) ------------------------------
// bic_encode_gray without planes: the count pass (k_gray_strips, EGS) writes each plane's EG stream
// (eg.cpp:20-37 with the block size fixed at 1: per row ~R, then the end-of-row '1') in its uniform
// layout -- bit 0 a '1', row r at bit r (cols + 1) + 1 -- instead of storing R: that layout is the
// stream itself but for ONE bit, cleared after the emission (eg_fix_bit). Every reader of R takes
// the row from there: ~(64 stream bits at the row's offset + 64 w), a wave-uniform funnel shift.
__device__ __forceinline__ uint64_t eg_src_bit0(const Geom& g, uint32_t row) {
  return (uint64_t)row * (g.cols + 1) + 1;
}
// residual word w of a row (any lane pattern; two loads, the second one usually a cache hit)
__device__ __forceinline__ uint64_t eg_src_word(const uint64_t* eplane, const Geom& g, uint32_t row, uint32_t w) {
  if (w >= g.used) return 0;
  const uint64_t b = eg_src_bit0(g, row) + (uint64_t)w * 64;
  const uint64_t* p = eplane + (b >> 6);
  const uint32_t sh = (uint32_t)(b & 63);
  const uint64_t hi = bswap64(p[0]);
  const uint64_t x = sh ? funnel64(hi, bswap64(p[1]), 64 - sh) : hi;
  return ~x & (w == g.used - 1 ? g.trail : ~0ull);
}
// the row's words t * 64 + lane (t < WPL) as resid_row gives them: one load per word, lane l + 1's word
// through DPP (wave_shl:1), lane 63's from lane 0 of the next word group (the last: one uniform load)
// (as two halves, so that a wave can issue a row's loads one row ahead: eg_src_load, then
// eg_src_assemble when the words are needed)
template <int WPL>
__device__ __forceinline__ void eg_src_load(const uint64_t* eplane, const Geom& g, uint32_t row, uint64_t (&v)[WPL],
                                            uint64_t& last) {
  const int lane = lane_id();
  const uint64_t b = eg_src_bit0(g, row);
  const uint64_t* p = eplane + (b >> 6);
  const uint32_t nw = g.used;  // stream words used: nw (+ 1 when the row is not word-aligned)
#pragma unroll
  for (int t = 0; t < WPL; ++t) {  // (every lane loads, at a clamped index: eg_src_assemble masks)
    const uint32_t j = t * 64 + lane;
    v[t] = p[j < nw ? j : nw - 1];
  }
  last = p[(b & 63) ? nw : nw - 1];  // (uniform address; unused when the row is word-aligned)
}
template <int WPL>
__device__ __forceinline__ void eg_src_assemble(const Geom& g, uint32_t row, const uint64_t (&v)[WPL], uint64_t last,
                                                uint64_t (&r)[WPL]) {
  const int lane = lane_id();
  const uint32_t sh = (uint32_t)(eg_src_bit0(g, row) & 63);
  const uint32_t nw = g.used;
#pragma unroll
  for (int t = 0; t < WPL; ++t) {
    const uint32_t j = t * 64 + lane;
    const uint64_t hi = bswap64(v[t]);
    uint64_t nx = ((uint64_t)(uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v[t] >> 32), 0x130, 0xf, 0xf, true) << 32) |
                  (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v[t], 0x130, 0xf, 0xf, true);
    if (lane == 63) {
      if (t + 1 < WPL && (t + 1) * 64 < (int)nw)
        nx = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v[t + 1 < WPL ? t + 1 : t] >> 32), 0) << 32) |
             (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v[t + 1 < WPL ? t + 1 : t], 0);
      else
        nx = last;
    }
    // (lane j + 1's word is its clamped load when j + 1 >= nw: only its bits past the row are used)
    const uint64_t x = sh ? funnel64(hi, bswap64(nx), 64 - sh) : hi;
    r[t] = j < nw ? ~x & (j == nw - 1 ? g.trail : ~0ull) : 0;
  }
}
// the row's words t * 64 + lane (t < WPL) as resid_row gives them: one load per word, lane l + 1's word
// through DPP (wave_shl:1), lane 63's from lane 0 of the next word group (the last: one uniform load)
template <int WPL>
__device__ __forceinline__ void eg_src_row(const uint64_t* eplane, const Geom& g, uint32_t row, uint64_t (&r)[WPL]) {
  uint64_t v[WPL], last;
  eg_src_load<WPL>(eplane, g, row, v, last);
  eg_src_assemble<WPL>(g, row, v, last, r);
}

// The row's words with lane l holding words l WPL .. l WPL + WPL - 1 (consecutive: one prefix per
// lane over its own words, one wave scan per row instead of one per word group): WPL + 1 loads
// per lane, the last one lane l + 1's first (clamped: masked in the assembly)
template <int WPL>
__device__ __forceinline__ void eg_src_load_lc(const uint64_t* eplane, const Geom& g, uint32_t row,
                                               uint64_t (&v)[WPL + 1]) {
  const uint64_t b = eg_src_bit0(g, row);
  const uint64_t* p = eplane + (b >> 6);
  const uint32_t jmax = (b & 63) ? g.used : g.used - 1;
#pragma unroll
  for (int t = 0; t <= WPL; ++t) {
    const uint32_t j = (uint32_t)lane_id() * WPL + t;
    v[t] = p[j < jmax ? j : jmax];
  }
}
template <int WPL>
__device__ __forceinline__ void eg_src_assemble_lc(const Geom& g, uint32_t row, const uint64_t (&v)[WPL + 1],
                                                   uint64_t (&r)[WPL]) {
  const uint32_t sh = (uint32_t)(eg_src_bit0(g, row) & 63);
#pragma unroll
  for (int t = 0; t < WPL; ++t) {
    const uint32_t w = (uint32_t)lane_id() * WPL + t;
    const uint64_t hi = bswap64(v[t]);
    const uint64_t x = sh ? funnel64(hi, bswap64(v[t + 1]), 64 - sh) : hi;
    r[t] = w < g.used ? ~x & (w == g.used - 1 ? g.trail : ~0ull) : 0;
  }
}

// Global-memory emission for a row whose Golomb image does not fit the LDS window: codeword
// bits landing in the row's first/last output word are kept for the fragment table, the rest
// is OR'd into words this wave zeroed first.
struct FragSink {
  unsigned long long* out;
  uint64_t wh, wt;
  bool hpart, tpart;
  uint64_t acc_h, acc_t;
  uint64_t idx, cur;
  __device__ __forceinline__ void flush() {
    if (!cur) return;
    if (idx == wh && hpart) acc_h |= cur;
    else if (idx == wt && tpart) acc_t |= cur;
    else atomicOr(&out[idx], (unsigned long long)bswap64(cur));
    cur = 0;
  }
  __device__ __forceinline__ void orw(uint64_t i, uint64_t v) {
    if (i != idx) { flush(); idx = i; }
    cur |= v;
  }
  __device__ __forceinline__ void put(uint64_t off, uint32_t v, uint32_t nb) {
    const uint64_t i = off >> 6;
    const uint32_t sh = (uint32_t)(off & 63);
    if (sh + nb <= 64) {
      orw(i, (uint64_t)v << (64 - sh - nb));
    } else {
      orw(i, (uint64_t)v >> (sh + nb - 64));
      orw(i + 1, (uint64_t)v << (128 - sh - nb));
    }
  }
  __device__ __forceinline__ void bit(uint64_t off) { orw(off >> 6, BIC_MSB >> (off & 63)); }
};

// The residual word w of the row, read back from the EG image (~R, pad-masked): the image is
// written for every row, so the Golomb steps need no registers for the row.
__device__ __forceinline__ uint64_t img_resid(const uint32_t* eimg, const Geom& g, uint32_t w) {
  if (w >= g.used) return 0;
  const uint64_t v = ((uint64_t)eimg[2 * w] << 32) | eimg[2 * w + 1];
  return ~v & (w == g.used - 1 ? g.trail : ~0ull);
}

// Rows whose Golomb output exceeds the LDS window (a long dense stretch at large k): the main
// kernel records their offset and sample base and appends them to a list; k_rows_global (a small
// grid walking that list, one wave per row) recomputes each and writes it straight to global
// memory -- its inner words are zeroed and OR'd, the bits landing in its first/last (shared) word
// go to the fragment table.
// (row_global_at: the row's absolute offset G, length L and slow = its samples before + 1 given)
template <bool PREDICT>
__device__ __forceinline__ void row_global_at(const FusedArgs& a, uint64_t id, uint32_t plane, uint32_t row,
                                              uint64_t G, uint64_t L, uint64_t slow, int lane) {
  const Geom& g = a.g;
  uint64_t* frag = a.gfrag + 2 * id;
  const uint64_t wh = G >> 6, wt = (G + L - 1) >> 6;
  const bool hpart = !word_complete(wh, G, L);
  const bool tpart = !word_complete(wt, G, L);
  for (uint64_t i = wh + lane; i <= wt; i += 64)
    if (!((i == wh && hpart) || (i == wt && tpart))) a.out_g[i] = 0;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  FragSink fs{reinterpret_cast<unsigned long long*>(a.out_g), wh, wt, hpart, tpart, 0, 0, 0, 0};
  StepState st{(uint32_t)(slow - 1), -1};
  const uint32_t arow = row * (g.cols + 1);
  RowCtx rc = row_ctx(a.planes, g, plane, row, 0);
  uint64_t carry = G;
  for (uint32_t w0 = 0; w0 < g.used; w0 += 64) {
    const uint32_t w = w0 + lane;
    const uint64_t x = (!PREDICT && a.esrc) ? eg_src_word(a.esrc + (uint64_t)plane * a.slot_e, g, row, w)
                                            : resid_word<PREDICT>(rc, g, row, w);
    uint32_t n;
    int jp;
    step_prefix(x, w, st, n, jp);
    const bool eol = w == g.used - 1;
    const LaneEnc e = encode_word<false>(x, w, n, jp, arow, eol, g.cols,
                                         ByteTables{reinterpret_cast<const uint32_t*>(a.lut + 256), a.lut});
    const uint32_t inc = wave_incl_sum_u32(e.len);
    const uint64_t off = carry + inc - e.len;
    carry += lane63_u32(inc);
    emit_word(fs, off, x, w, n, jp, arow, eol, g.cols);
  }
  fs.flush();
  uint64_t h = fs.acc_h, tl = fs.acc_t;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    h |= shfl_u64(h, lane ^ d);
    tl |= shfl_u64(tl, lane ^ d);
  }
  if (lane == 0) {
    if (hpart) put_shared(a.out_g, wh, frag, 0, h | (wh == wt ? tl : 0));
    if (tpart && wt != wh) put_shared(a.out_g, wt, frag, 1, tl);
  }
}
template <bool PREDICT>
__device__ __forceinline__ void row_global(const FusedArgs& a, uint64_t id, int lane) {
  const Geom& g = a.g;
  const uint32_t plane = (uint32_t)(id / g.rows), row = (uint32_t)(id % g.rows);
  row_global_at<PREDICT>(a, id, plane, row, gb_abs(a, id, plane), a.glen[id] & kLenMask, a.gslow[id], lane);
}

// EG source: after every reader of the residual rows, the one bit per plane in which the uniform
// layout differs from the EG stream (eg_src_junctions' ONES scan found it: the first 1's bit, or the
// layout's bit past the end of a plane without 1s) is cleared. The readers are the Golomb emission
// (k_emit_k01 / k_emit_known, k_emit_rest) and the slow rows (k_rows_global, or k_emit_rest's own
// loop on the class kernels' path), so with the Golomb stream requested the clear is k_fixup's (block
// 0, launched after both); without it nothing reads the rows and k_rows_global's one block does it.
__device__ __forceinline__ void eg_fix_bit(const uint64_t* efix, uint64_t* out_e, uint64_t slot_e, uint32_t nplanes) {
  if (!efix || blockIdx.x != 0 || threadIdx.x >= nplanes) return;
  const uint64_t P = efix[threadIdx.x];
  uint64_t* w = out_e + (uint64_t)threadIdx.x * slot_e + (P >> 6);
  *w &= ~bswap64(BIC_MSB >> (P & 63));
}

// EG row from registers: row bit b (b < cols) is ~R, bit cols is the end-of-row '1'; output word
// j of the row holds row bits [64j - g, 64j - g + 64) with g = Ge % 64. Lane l forms words
// j = 64t + l from its own row word and its left neighbour's (one shuffle per step).
// INV = false: the row bits are R itself (a Golomb row whose codewords all have k = 0).
template <int WPL, bool INV = true>
__device__ __forceinline__ void eg_row_regs(const uint64_t (&rr)[WPL], const Geom& g, uint64_t Ge, uint64_t Le,
                                            uint64_t* out, uint64_t* frag) {
  const int lane = lane_id();
  const uint32_t sh = (uint32_t)(Ge & 63);
  const uint64_t w0 = Ge >> 6, nw = ((Ge + Le - 1) >> 6) - w0 + 1;
  const uint32_t eolw = g.cols >> 6;
  const uint64_t eolbit = BIC_MSB >> (g.cols & 63);
  const bool head_whole = sh == 0, tail_whole = ((Ge + Le) & 63) == 0;  // (only the first / last word can be shared)
  uint64_t carry = 0;
#pragma unroll
  for (int t = 0; t <= WPL; ++t) {
    const uint32_t j = t * 64 + lane;
    if (t * 64 >= (int)nw) break;
    uint64_t X = 0;
    if (t < WPL && j < g.used) X = INV ? ~rr[t] & (j == g.used - 1 ? g.trail : ~0ull) : rr[t];
    if (j == eolw) X |= eolbit;
    uint64_t Xl = shfl_up_u64(X, 1);
    if (lane == 0) Xl = carry;
    carry = lane63_u64(X);
    const uint64_t v = funnel64(Xl, X, sh);
    if (j < nw) {
      const uint64_t wi = w0 + j;
      if ((j != 0 || head_whole) && (j != nw - 1 || tail_whole)) out[wi] = bswap64(v);
      else put_shared(out, wi, frag, j == 0 ? 0 : 1, v);
    }
  }
}

// ---- host side: the kernels' arguments and the template dispatch --------------------------------

// The kernels' view of one call; every launch function builds it with this.
inline FusedArgs make_fused_args(const FusedCall& c) {
  const FusedArena& ar = c.ar;
  const FusedRequest& rq = c.rq;
  // the index alone (bic_row_index): the prefix kernels touch no output word, but the LEN scan checks
  // the rows against slot_g and stores the planes' totals through bits_g -- into the scratch then
  const bool index_only = !rq.g.out && rq.index;
  FusedArgs a{c.g, c.planes, c.lut, ar.counter, ar.ones_rec, ar.bits_rec, ar.gboff, ar.glen, ar.gfrag, ar.gslow,
              ar.eboff, ar.elen, ar.efrag, ar.row_o, ar.sones, ar.krec, ar.kpos, rq.counted ? rq.ns : 1u, ar.walk_ids,
              ar.rest_ids, ar.slow_n, ar.slow_ids, index_only ? rq.index : rq.g.out, rq.g.slot,
              index_only ? ar.gbase : rq.g.bits, rq.e.out, rq.e.slot, rq.e.bits, c.flags};
  a.pones = ar.pones;
  a.walk_o = ar.walk_o;
  a.gbase = ar.gbase;
  a.off_g = rq.g.out ? rq.g.off : nullptr;
  a.off_e = rq.e.out ? rq.e.off : nullptr;
  a.ebase = a.off_e ? ar.ebase : nullptr;
  a.index = a.out_g ? rq.index : nullptr;
  // EG source (bic_encode_gray without planes): the count pass wrote the EG stream, the emission is
  // Golomb's alone and reads the residual rows from it
  const bool es = c.mode == kEncStaged && rq.eg_src && a.out_e && !a.off_e && !c.predict;
  a.esrc = es ? a.out_e : nullptr;
  a.efix = es ? ar.efix : nullptr;
  a.cls = es && a.out_g && !rq.eg_src_one ? ar.cls : nullptr;
  a.sink = ar.sink;
#ifdef BIC_STAMPS
  a.known = getenv("BIC_KNOWN") && getenv("BIC_KNOWN")[0] == '1';
#endif
  return a;
}

// f(integral_constant<int, WPL>) for the row width's words per lane (w() is the constant)
template <typename F>
void with_wpl(const Geom& g, F&& f) {
  if (g.used <= 64) f(std::integral_constant<int, 1>{});
  else if (g.used <= 128) f(std::integral_constant<int, 2>{});
  else f(std::integral_constant<int, 4>{});
}
// f(WPL, PREDICT, DO_G, DO_E) as integral constants: the template arguments of a row kernel that
// writes Golomb (dg), EG (de) or both (neither: as EG alone)
template <typename F>
void with_row_kernel(const Geom& g, bool predict, bool dg, bool de, F&& f) {
  with_wpl(g, [&](auto w) {
    auto coders = [&](auto p) {
      if (dg && de) f(w, p, std::true_type{}, std::true_type{});
      else if (dg) f(w, p, std::true_type{}, std::false_type{});
      else f(w, p, std::false_type{}, std::true_type{});
    };
    if (predict) coders(std::true_type{});
    else coders(std::false_type{});
  });
}

}  // namespace bic
