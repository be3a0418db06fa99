// bic_fused.hip -- the staged row encoder for rows of up to 256 words (16384 columns), the default:
// count pass -> ONES scan -> walk of the mixed-k rows -> LEN scan -> emission (k_emit_known, or
// k_emit_k01 per row class when the rows come back from the EG stream, with k_emit_rest beside it
// for the listed rows); then the finish kernels every row encoder shares (k_rows_global, k_fixup)
// and the scratch arena's layout. The lanes' codewords, the row images and the kernels' argument
// block are bic_fused.h's; the look-back encoders (small batches, cross-checks) are
// bic_fused_lookback.hip's.
#include "bic_fused.h"

#include <algorithm>
#include <cstdio>

namespace bic {

template <bool PREDICT>
__global__ __launch_bounds__(256) void k_rows_global(FusedArgs a) {
  const int lane = lane_id();
  if (!a.out_g) eg_fix_bit(a.esrc ? a.efix : nullptr, a.out_e, a.slot_e, a.g.nplanes);
  const uint32_t nslow = *a.slow_n;
  for (uint32_t li = blockIdx.x * 4 + wave_id(); li < nslow; li += gridDim.x * 4)
    row_global<PREDICT>(a, a.slow_ids[li], lane);
}

// ==========================================================================================
// Staged encoder (default): every inter-row dependency is resolved by a kernel boundary instead of
// a decoupled look-back, so no workgroup ever waits on another (a cross-XCD look-back hop costs
// microseconds, MI355X_MICROARCH.md barrier-counter row, and a tile waiting on one holds its
// CU's waves idle). Stages: per-row residual 1-counts (k_med_rows<ROWS>) -> per-plane scan ->
// per-row Golomb lengths (word_len) -> per-plane scan of the lengths -> k_emit_known, where each
// wave walks its rows independently (persistent waves, static row order, no barriers).
// ==========================================================================================

// Golomb length of a row from its sample base O (ones of the plane before it): rows whose k
// statistics (bic_kstat.h) prove every codeword k = 0 (length cols + 1: the residual row and its
// end-of-row '1') or k = 1 (2n + (zeros - odd runs) / 2) get their length without being read;
// returns true for the others (k_row_walk walks them).
__device__ __forceinline__ bool row_class(const FusedArgs& a, uint64_t id, uint32_t row, uint32_t O, const RowK& rk) {
  const Geom& g = a.g;
  if (row == 0) return true;  // (the plane's first sample has k = 1 from the fresh state, Golomb.h:18)
  const int64_t N0 = (int64_t)O + row, A0 = (int64_t)row * g.cols - O;
  if (A0 - N0 + rk.q0 <= 0) {
    a.glen[id] = kK0Row | (g.cols + 1);
    return false;
  }
  if (A0 - 2 * N0 + rk.qh <= 0 && A0 - N0 + rk.ql > 0) {
    const uint64_t n = rk.ones + 1, zeros = g.cols - rk.ones, odd = n - rk.chg;
    a.glen[id] = kK1Row | (2 * n + (zeros - odd) / 2);
    return false;
  }
  return true;
}

// Packed output: the planes' start words in each coder's buffer (streams word-aligned, plane order:
// bic_pack_streams' layout) from the Golomb totals (LEN scan) and the EG lengths (rows (cols + 1), + 1
// when the plane holds a residual 1: eg.cpp's first-run bit), each capped at the slot size so that an
// overflowing plane (BIC_ENOSPC) cannot push a later one past the buffer. One workgroup.
__device__ __forceinline__ void plane_bases(const FusedArgs& a, uint64_t* tmp) {
  const Geom& g = a.g;
  uint64_t cg = 0, ce = 0;  // running bases (words)
  for (uint32_t q0 = 0; q0 < g.nplanes; q0 += 1024) {
    const uint32_t q = q0 + threadIdx.x;
    const bool in = q < g.nplanes;
    uint64_t gw = 0, ew = 0;
    if (in && a.off_g) gw = min((a.bits_g[q] + 63) / 64, a.slot_g);
    if (in && a.off_e) ew = min(((uint64_t)g.rows * (g.cols + 1) + (a.pones[q] ? 1 : 0) + 63) / 64, a.slot_e);
    uint64_t tg, te;
    const uint64_t pg = block_excl_scan<uint64_t>(gw, tmp, tg) + cg;
    const uint64_t pe = block_excl_scan<uint64_t>(ew, tmp, te) + ce;
    if (in && a.off_g) {
      a.off_g[q] = pg;
      a.gbase[q] = pg;
    }
    if (in && a.off_e) {
      a.off_e[q] = pe;
      a.ebase[q] = pe * 64;
    }
    cg += tg;
    ce += te;
  }
  if (threadIdx.x == 0) {
    if (a.off_g) a.off_g[g.nplanes] = cg;
    if (a.off_e) a.off_e[g.nplanes] = ce;
  }
}
// Exclusive per-plane scan of per-row values. Each kScanThreads-thread workgroup owns kScanChunk rows of a
// plane (kScanPer consecutive rows per thread) and sums the plane's earlier rows itself (coalesced,
// at most rows / kScanThreads loads per thread), so no workgroup waits on another and a plane spreads over
// rows / kScanChunk CUs. ONES: the strips' 1-counts (sones) -> row_o[], the ones before each row;
// with CLASSIFY each row is also classified (row_class) and the rows to walk are appended to
// walk_ids. Otherwise: glen[] Golomb lengths -> gboff[] absolute bit offsets in the plane's slot,
// bits_g[] the plane's total; rows past the slot's end get glen = 0 and raise the overflow flag
// (a later chunk may then sum a zeroed length: its offsets stay inside the slot, and the call
// reports BIC_ENOSPC with the stream undefined).
constexpr uint32_t kScanThreads = 512;
// (1024-row chunks: twice the workgroups of 2048, C3 prefix 51 -> 42 us; 512-row chunks, 256 workgroups for
// C3's 256 CUs: the ONES scan 12.8-14.2 -> 10.4-11.7 us)
constexpr uint32_t kScanPer = 1, kScanChunk = kScanThreads * kScanPer;
constexpr uint32_t kScanAhead = 16;  // loads in flight per thread in the ONES scan's sum of the plane's earlier rows (C3: all of them)
template <bool ONES, bool CLASSIFY>
__global__ __launch_bounds__(kScanThreads) void k_scan_rows(FusedArgs a) {
  __shared__ uint64_t tmp[17];
  const Geom& g = a.g;
  const uint32_t nb = (g.rows + kScanChunk - 1) / kScanChunk;
  const uint32_t plane = blockIdx.x / nb;
  const uint32_t b = blockIdx.x % nb;
  const uint64_t base = (uint64_t)plane * g.rows;
  auto val = [&](uint32_t r) -> uint64_t {
    if constexpr (ONES) {
      // a row's strip counts in one load for 1, 2 and 4 strips (4: C3; 16 bytes, aligned as sones is)
      const uint32_t* so = a.sones + (base + r) * a.ns;
      if (a.ns == 4) {
        const uint4 q = *reinterpret_cast<const uint4*>(so);
        return (uint64_t)q.x + q.y + q.z + q.w;
      }
      if (a.ns == 2) {
        const uint2 q = *reinterpret_cast<const uint2*>(so);
        return (uint64_t)q.x + q.y;
      }
      if (a.ns == 1) return so[0];
      uint64_t o = 0;
      for (uint32_t q = 0; q < a.ns; ++q) o += so[q];
      return o;
    } else {
      return a.glen[base + r] & kLenMask;
    }
  };
  SSTAMP(0);
  const uint32_t r0 = b * kScanChunk + threadIdx.x * kScanPer;
  uint64_t v[kScanPer], sum = 0;
#pragma unroll
  for (uint32_t i = 0; i < kScanPer; ++i) {
    v[i] = r0 + i < g.rows ? val(r0 + i) : 0;
    sum += v[i];
  }
  // (ONES + CLASSIFY: the rows' k statistics loaded now, their latency under the scans below)
  RowKRaw rks[kScanPer];
  if constexpr (ONES && CLASSIFY) {
#pragma unroll
    for (uint32_t i = 0; i < kScanPer; ++i) {
      const uint64_t id = base + (r0 + i < g.rows ? r0 + i : 0);
      rks[i] = row_kstats_load(a.krec + id * a.ns, a.kpos + id * a.ns, a.ns);
    }
  }
  SSTAMP(1);
  uint64_t before = 0;  // this thread's share of the plane's rows before the chunk
  const uint32_t lim = b * kScanChunk;
  if constexpr (ONES) {  // the records of those rows are one contiguous range
    const uint32_t* so = a.sones + base * a.ns;
    const uint64_t flat = (uint64_t)lim * a.ns;  // a multiple of 4 (lim is one of kScanChunk)
    if ((base * a.ns) % 4 == 0) {  // 16-byte loads
      // kScanAhead independent loads per trip, each at a clamped index and all issued before the first
      // is used: one wait for C3's <= 15 loads per thread
      const uint4* s4 = reinterpret_cast<const uint4*>(so);
      const uint64_t n4 = flat / 4;
      for (uint64_t i0 = threadIdx.x; i0 < n4; i0 += kScanAhead * kScanThreads) {
        uint4 q[kScanAhead];
#pragma unroll
        for (uint32_t k = 0; k < kScanAhead; ++k) {
          const uint64_t i = i0 + k * kScanThreads;
          q[k] = s4[i < n4 ? i : i0];
        }
#pragma unroll
        for (uint32_t k = 0; k < kScanAhead; ++k)
          if (i0 + k * kScanThreads < n4) before += (uint64_t)q[k].x + q[k].y + q[k].z + q[k].w;
      }
    } else {
#pragma unroll 8
      for (uint64_t i = threadIdx.x; i < flat; i += kScanThreads) before += so[i];
    }
  } else {
#pragma unroll 8
    for (uint32_t r = threadIdx.x; r < lim; r += kScanThreads) before += val(r);
  }
  SSTAMP(2);
  uint64_t tot, btot, pre;
  if constexpr (ONES) {
    // one workgroup scan of a packed pair: a plane's 1-count fits 32 bits (fused_supported), so the low
    // half -- the chunk's prefix -- never carries into the high half, whose total is `before`'s sum
    uint64_t t2;
    const uint64_t p2 = block_excl_scan<uint64_t>(sum | (before << 32), tmp, t2);
    tot = (uint32_t)t2;
    btot = t2 >> 32;
    pre = (uint32_t)p2 + btot;
  } else {  // (the lengths stay 64-bit)
    pre = block_excl_scan<uint64_t>(sum, tmp, tot);
    (void)block_excl_scan<uint64_t>(before, tmp, btot);
    pre += btot;
  }
  SSTAMP(3);
  if constexpr (ONES) {
    bool walks[kScanPer];  // classify every row of the thread first: their record loads overlap
    uint64_t p = pre;
#pragma unroll
    for (uint32_t i = 0; i < kScanPer; ++i) {
      const uint32_t r = r0 + i;
      if constexpr (CLASSIFY) walks[i] = r < g.rows && row_class(a, base + r, r, (uint32_t)p, row_kstats_combine(rks[i], g.cols));
      else walks[i] = false;
      p += v[i];
    }
#pragma unroll
    for (uint32_t i = 0; i < kScanPer; ++i) {
      const uint32_t r = r0 + i;
      const bool in = r < g.rows;
      if (in) a.row_o[base + r] = (uint32_t)pre;
      const bool walk = walks[i];
      if constexpr (CLASSIFY) {
        const uint64_t m = __ballot(walk);  // wave-aggregated append to the list of rows to walk
        if (m) {
          uint32_t wb = 0;
          const int leader = __builtin_ctzll(m);
          if (lane_id() == leader) wb = atomicAdd(a.counter + 2, (uint32_t)__popcll(m));
          wb = (uint32_t)__shfl((int)wb, leader);
          if (walk) {
            const uint32_t wi = wb + (uint32_t)__popcll(m & ((1ull << lane_id()) - 1ull));
            a.walk_ids[wi] = (uint32_t)(base + r);
            a.walk_o[wi] = (uint32_t)pre;
          }
        }
      }
      const bool first1 = in && pre == 0 && v[i] > 0;  // the row holding the plane's first 1
      if (a.esrc) {
        // EG source: the stream bit eg.cpp's first-run '0' makes differ from the uniform layout: the
        // first 1's own bit (the layout has a '1' there, the shifted ~R of the pixel before it)
        if (first1) {
          const uint32_t* so = a.sones + (base + r) * a.ns;
          const uint32_t* kp = a.kpos + (base + r) * a.ns;
          uint32_t j1 = 0;
          for (uint32_t q = 0; q < a.ns; ++q)
            if (so[q]) {
              j1 = kp[q] & 0xffffu;
              break;
            }
          a.efix[plane] = (uint64_t)r * (g.cols + 1) + j1;
        }
      } else if (first1 && !walk && a.out_e) {
        // (EG inserts a '0' after it): listed for REST here unless walked (k_row_walk's list)
        a.rest_ids[atomicAdd(a.counter + 3, 1u)] = (uint32_t)(base + r);
      }
      pre += v[i];
    }
    if (b == nb - 1 && threadIdx.x == 0) {
      const uint64_t po = btot + tot;
      a.pones[plane] = po;  // the plane's residual 1s
      if (a.esrc) {  // the EG length (eg.cpp: rows (cols + 1), + 1 for the first run's g = 1 bit)
        a.bits_e[plane] = (uint64_t)g.rows * (g.cols + 1) + (po ? 1 : 0);
        if (!po) a.efix[plane] = (uint64_t)g.rows * (g.cols + 1);  // no 1: the layout's last bit is past the end
      }
    }
  } else {
    const uint64_t cap = a.slot_g * 64;
    if (a.cls) {  // EG source: this chunk's k = 0 / k = 1 rows appended to the class lists
      static_assert(kScanPer == 1, "one row per thread");
      const uint32_t r = r0;
      const uint64_t f = r < g.rows ? a.glen[base + r] : 0;
      const bool ok = pre + v[0] <= cap && v[0] != 0;  // (an overflowing row is written by nobody)
      // a k = 1 or mixed row too long for an LDS row image is written by k_emit_rest's slow-row loop
      // (row_global; k = 0 rows are shifted copies, no image): the list is complete before the emission
      constexpr uint32_t kCapBitsRest = (kGImg - kPad) * 32;
      const bool big = v[0] > kCapBitsRest;
      const uint32_t c0 = ok && (f & kK0Row) ? 1u : 0u, c1 = ok && (f & kK1Row) && !big ? 1u : 0u;
      if (ok && !(f & kK0Row) && big) {
        a.gslow[base + r] = a.row_o[base + r] + r + 1;
        a.slow_ids[atomicAdd(a.slow_n, 1u)] = base + r;
      }
      uint32_t t0, t1;
      const uint32_t x0 = block_excl_scan<uint32_t>(c0, reinterpret_cast<uint32_t*>(tmp), t0);
      const uint32_t x1 = block_excl_scan<uint32_t>(c1, reinterpret_cast<uint32_t*>(tmp), t1);
      __shared__ uint32_t lb[2];
      if (threadIdx.x == 0) {
        lb[0] = t0 ? atomicAdd(a.counter + 4, t0) : 0u;
        lb[1] = t1 ? atomicAdd(a.counter + 5, t1) : 0u;
      }
      __syncthreads();
      const uint64_t nrows = (uint64_t)g.rows * g.nplanes;
      const uint64_t G = (uint64_t)plane * cap + pre;  // (gboff's value, written below)
      if (c0) {
        a.cls[2 * (lb[0] + x0)] = (base + r) | ((uint64_t)plane << 32);  // id, plane (the length is cols + 1)
        a.cls[2 * (lb[0] + x0) + 1] = G;
      }
      if (c1) {
        a.cls[2 * (nrows + lb[1] + x1)] = (base + r) | (v[0] << 32);
        a.cls[2 * (nrows + lb[1] + x1) + 1] = G;
      }
    }
#pragma unroll
    for (uint32_t i = 0; i < kScanPer; ++i) {
      const uint32_t r = r0 + i;
      if (r < g.rows) {
        a.gboff[base + r] = (uint64_t)plane * cap + pre;
        if (a.index) {  // the decoders' row index (bic_row_index): slot-relative offset, 1s before the row
          a.index[2 * (base + r)] = pre;
          a.index[2 * (base + r) + 1] = a.row_o[base + r];
        }
        if (pre + v[i] > cap) {
          a.glen[base + r] = 0;  // overflowed: nothing written, fixup skips
          atomicOr(&a.flags[0], 1u);
        }
      }
      pre += v[i];
    }
    if (b == nb - 1 && threadIdx.x == 0) a.bits_g[plane] = btot + tot;
  }
  SSTAMP(4);
}

// One row across a workgroup of blockDim.x / 64 (<= 4) waves, lane = word 64 v + lane of wave v:
// the lane's sample base n (samples of the plane before its word's first 1, from nbase = the
// samples before the row) and jp (the row's last 1 before its word, -1: none), from wave scans
// and the earlier waves' totals exchanged through LDS (sh: 8 words); ones = the row's 1s.
struct WideRow {
  uint32_t n;
  int jp;
  uint32_t ones;
};
__device__ __forceinline__ WideRow wide_prefix(uint64_t x, uint32_t w, uint32_t nbase, uint32_t* sh) {
  const int lane = lane_id(), v = (int)wave_id(), nw = blockDim.x >> 6;
  const uint32_t pc = (uint32_t)__popcll(x), inc = wave_incl_sum_u32(pc);
  const int mx = wave_incl_max(x ? (int)(w * 64 + 63 - __builtin_ctzll(x)) : -1);
  if (lane == 63) {
    sh[v] = inc;
    sh[8 + v] = (uint32_t)mx;
  }
  __syncthreads();
  uint32_t nb = nbase, tot = 0;
  int jb = -1;
  for (int u = 0; u < nw; ++u) {
    const uint32_t c = sh[u];
    if (u < v) {
      nb += c;
      jb = max(jb, (int)sh[8 + u]);
    }
    tot += c;
  }
  __syncthreads();  // sh is reused
  return WideRow{nb + inc - pc, max(jb, dpp_or<0x138>(-1, mx)), tot};
}

// The listed rows' Golomb lengths (codeword walk, word_len), one workgroup per row and one HALF word
// per lane (lanes 2w and 2w + 1 share residual word w, each counting the codewords whose '1' lies in
// its 32 columns), so a row's serial codeword chain is at most 32 columns long; a fixed grid strides
// over the list, whose length k_scan_rows left in counter[2]. k_emit_rest takes the rows with mixed k,
// and the row holding the plane's first 1, from this same list. (One word per lane: C3 walk 17.4 us.)
constexpr uint32_t kWalkWaves = 8192;  // the walk grid in waves (32 per CU), whatever the row width
#ifndef BIC_WALK_SPLIT
#define BIC_WALK_SPLIT 2
#endif
constexpr uint32_t kWalkSplit = BIC_WALK_SPLIT;  // lanes per residual word (1 or 2)
// residual word w of a row on its own (the word left of it loaded too): no cross-lane exchange, so
// any lane layout can call it
template <bool PREDICT>
__device__ __forceinline__ uint64_t resid_word_at(const uint64_t* planes, const Geom& g, uint32_t plane, uint32_t row,
                                                  uint32_t w) {
  if (w >= g.used) return 0;
  const uint64_t* cur = planes + (uint64_t)plane * g.plane_words + (uint64_t)row * g.wpr;
  uint64_t d = cur[w];
  if constexpr (PREDICT) {
    const uint64_t* up = cur - g.wpr;
    if (row) d ^= up[w];
    const uint64_t dl = w ? cur[w - 1] ^ (row ? up[w - 1] : 0ull) : 0ull;
    d ^= (d >> 1) | (dl << 63);
    if (row == 0 && w == 0) d &= ~BIC_MSB;  // pred.cpp never writes pP(0,0)
  }
  return w == g.used - 1 ? d & g.trail : d;
}
template <bool PREDICT>
__global__ __launch_bounds__(512) void k_row_walk(FusedArgs a) {
  __shared__ uint32_t sh[16], sl[8], sk[8];
  const Geom& g = a.g;
  const int lane = lane_id(), v = (int)wave_id(), nw = blockDim.x >> 6;
  const uint32_t w = (64 * v + lane) / kWalkSplit, h = kWalkSplit == 1 ? 1u : (uint32_t)lane & 1u;
  const uint64_t hmask = kWalkSplit == 1 ? ~0ull : (h ? 0x00000000FFFFFFFFull : 0xFFFFFFFF00000000ull);
  const uint32_t nlist = __hip_atomic_load(a.counter + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // (the list entry -- row id and its row_o, side by side -- of the workgroup's next row is loaded
  // while this row is walked)
  uint32_t nid = blockIdx.x < nlist ? a.walk_ids[blockIdx.x] : 0u, nO = blockIdx.x < nlist ? a.walk_o[blockIdx.x] : 0u;
  for (uint32_t i = blockIdx.x; i < nlist; i += gridDim.x) {
    const uint64_t id = nid;
    const uint32_t O = nO;
    if (i + gridDim.x < nlist) {
      nid = a.walk_ids[i + gridDim.x];
      nO = a.walk_o[i + gridDim.x];
    }
    WSTAMP(4);
    const uint32_t plane = (uint32_t)(id / g.rows), row = (uint32_t)(id % g.rows);
    const uint64_t x = ((!PREDICT && a.esrc) ? eg_src_word(a.esrc + (uint64_t)plane * a.slot_e, g, row, w)
                                             : resid_word_at<PREDICT>(a.planes, g, plane, row, w)) & hmask;
    WSTAMP(5);
    const WideRow p = wide_prefix(x, w, O + row, sh);
    uint32_t kor = 0;
    const bool eol = w == g.used - 1 && h == 1;
    uint32_t ll = word_len(x, w, p.n, p.jp, row * (g.cols + 1), eol, g.cols, kor);
    ll = wave_sum_u32(ll);
    WSTAMP(6);
    const uint64_t ks = __ballot(kor & ~1u), k1s = __ballot(kor & ~2u);  // some k != 0 / some k != 1
    const uint64_t kbig = __ballot(kor & ~3u);                           // some k >= 2
    if (lane == 0) {
      sl[v] = ll;
      sk[v] = (ks ? 1u : 0u) | (k1s ? 2u : 0u) | (kbig ? 4u : 0u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t L = 0, kk = 0;
      for (int u = 0; u < nw; ++u) {
        L += sl[u];
        kk |= sk[u];
      }
      // (mixed-k rows and the plane's first-1 row are k_emit_rest's: it finds them in this list by
      // glen's flags and row_o, so no row is appended here -- thousands of same-address atomics
      // would serialise this kernel)
      a.glen[id] = L | (!(kk & 1u) ? kK0Row : (!(kk & 2u) ? kK1Row : 0));
    }
    WSTAMP(7);
    __syncthreads();
  }
}

// The rows with every prefix known. EG rows, and Golomb rows whose codewords all have k = 0 (the
// residual row and its '1'), are shifted copies formed in registers; Golomb rows whose codewords
// all have k = 1 go through an LDS row image (byte tables), written with plain stores. Rows whose
// image exceeds the LDS window go to the k_rows_global list; rows with mixed k and the EG row of
// the plane's first 1 are k_emit_rest's (their per-codeword path alone costs ~50 VGPRs, which
// would halve this kernel's occupancy). The words shared with neighbouring rows go to the fragment
// tables (k_fixup). One wave per row, persistent 4-wave workgroups, no barriers after the byte
// tables are staged (XCD-remapped block order: the waves of one XCD hold consecutive rows, the
// row above is an L2 hit).
constexpr int kEmitWaves = 4;
// the class kernels' output stores (typed unsigned long long: see FusedArgs::cls)
__device__ __forceinline__ void class_store(uint64_t* dst, uint64_t v) {
  *reinterpret_cast<unsigned long long*>(dst) = v;
}
// write_row64 with a fixed number of store instructions (MAXT per lane, the idle lanes' to a.sink)
// and its stores typed unsigned long long (k_emit_k0)
template <int MAXT>
__device__ __forceinline__ void write_row64_fixed(const uint64_t* img, uint64_t L, uint64_t G, uint64_t* out,
                                                  uint64_t* frag, uint64_t* sink) {
  const int lane = lane_id();
  const uint64_t w0 = G >> 6, w1 = (G + L - 1) >> 6;
  const uint32_t nw = (uint32_t)(w1 - w0 + 1), g = (uint32_t)(G & 63);
  const bool head_whole = g == 0, tail_whole = ((G + L) & 63) == 0;
#pragma unroll
  for (int it = 0; it < MAXT; ++it) {
    const uint32_t t = it * 64 + lane;
    const bool in = t < nw;
    const uint32_t tc = in ? t : 0u;
    // (the image read as unsigned long long, the type its atomics write: ordered after them)
    const unsigned long long* im = reinterpret_cast<const unsigned long long*>(img);
    const uint64_t cur = im[tc], prev = tc ? im[tc - 1] : 0ull;
    const uint64_t v = funnel64(prev, cur, g);
    const bool whole = in && (t != 0 || head_whole) && (t != nw - 1 || tail_whole);
    uint64_t* dst = whole ? out + w0 + t : (in ? frag + (t == 0 ? 0 : 1) : sink + lane);
    class_store(dst, whole ? bswap64(v) : v);
  }
}

// One row of k_emit_known (rr: its residual words; O, Lf, Gb: its ones before, Golomb length + flags,
// absolute Golomb bit offset; Eb: its plane's EG start bit), by one wave with its LDS image gimg.
template <int WPL, bool PREDICT, bool DO_G, bool DO_E>
__device__ __forceinline__ void emit_known_row(const FusedArgs& a, uint64_t id, uint32_t plane, uint32_t row,
                                               const uint64_t (&rr)[WPL], uint32_t O, uint64_t Lf, uint64_t Gb,
                                               uint64_t Eb, uint32_t* gimg, const uint32_t* s_lut) {
  const Geom& g = a.g;
  const int lane = lane_id();
  constexpr uint32_t kCapBits = (kGImg - kPad) * 32;
  const uint64_t L = Lf & kLenMask;
  const bool k0 = (Lf & kK0Row) != 0, k1 = (Lf & kK1Row) != 0, fits = L <= kCapBits;
  const bool gk1 = DO_G && L && k1 && fits;  // Golomb row through the LDS image (k = 1 byte tables)
  if (gk1) {  // zero the Golomb image: 8-byte stores of its atomics' type (see lds_image_zero32)
    unsigned long long* z = reinterpret_cast<unsigned long long*>(gimg);
    for (int i = lane; i < kGImg / 2; i += 64) z[i] = 0ull;
  }
  bool f_here = false;  // the plane's first 1 is in this row (k_emit_rest writes its EG row)
  if (DO_E && O == 0) {
    uint32_t ones = 0;
#pragma unroll
    for (int t = 0; t < WPL; ++t) ones += (uint32_t)__popcll(rr[t]);
    f_here = wave_sum_u32(ones) > 0;
  }
  if constexpr (DO_E) {  // EG as written (eg.cpp:20-37): per row ~R then '1'; a '0' after the plane's first 1
    const uint64_t Le = (uint64_t)g.cols + 1 + (f_here ? 1 : 0);
    const uint64_t Ge_rel = (uint64_t)row * (g.cols + 1) + (O > 0 ? 1 : 0);
    const uint64_t cap = a.slot_e * 64;
    const uint64_t Ge = Eb + Ge_rel;
    if (Ge_rel + Le <= cap) {
      if (!f_here) eg_row_regs<WPL>(rr, g, Ge, Le, a.out_e, a.efrag + 2 * id);
      if (lane == 0) {
        a.eboff[id] = Ge;
        a.elen[id] = Le;
      }
    } else if (lane == 0) {
      a.eboff[id] = Ge;
      a.elen[id] = 0;
      atomicOr(&a.flags[0], 1u);
    }
    if (lane == 0 && row == g.rows - 1) a.bits_e[plane] = Ge_rel + Le;
  }
  STAMP(1);
#ifdef BIC_STAMPS
  if (lane == 0) g_stamps[id * 8 + 3] = (k0 ? 1u : 0u) | (gk1 ? 2u : 0u) | ((uint64_t)blockIdx.x << 8) |
                                        ((uint64_t)wave_id() << 40);
#endif
  if constexpr (DO_G) {
    if (k0 && L) {
      eg_row_regs<WPL, false>(rr, g, Gb, L, a.out_g, a.gfrag + 2 * id);
    } else if (gk1) {  // every codeword k = 1: branch-free byte-table words into a 64-bit LDS image
      uint64_t* img = reinterpret_cast<uint64_t*>(gimg);
      int jpc = -1;
      uint32_t loc = 0;
#pragma unroll
      for (int t = 0; t < WPL; ++t) {
        if (t * 64 >= (int)g.used) break;
        const uint32_t w = t * 64 + lane;
        const uint64_t x = rr[t];
        const int jp = step_jp(x, w, jpc);
        const bool eol = w == g.used - 1;
        const LaneEnc e = encode_word_k1b(x, w, jp, eol, g.cols, s_lut);
        const uint32_t inc = wave_incl_sum_u32(e.len);
        const uint32_t off = loc + inc - e.len;
        loc += lane63_u32(inc);
        if (!e.lng) {
          if (e.head) lds_or64(img, off >> 6, BIC_MSB >> (off & 63));
          place128_64(img, off + 1 + e.z, e.t0, e.t1, e.tlen);
        } else {
          LdsSink64 ls{img, 0, 0};
          emit_word_k1(ls, off, x, w, jp, eol, g.cols);
          ls.flush();
        }
      }
      if (lane == 0 && loc != L) atomicOr(&a.flags[3], 1u);  // word_len disagrees with the emission
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      write_row64(img, L, Gb, a.out_g, a.gfrag + 2 * id);
    }
    if (lane == 0) {
      // glen keeps its flags: k_emit_rest (on the other stream) reads them too
      const bool slow = L && !k0 && !fits;
      a.gslow[id] = slow ? O + row + 1 : 0;  // k_rows_global writes the row
      if (slow) a.slow_ids[atomicAdd(a.slow_n, 1u)] = id;
    }
  }
}

// ES: the residual rows from the EG stream the count pass wrote (FusedArgs::esrc; PREDICT false)
template <int WPL, bool PREDICT, bool DO_G, bool DO_E, bool ES = false>
__global__ __launch_bounds__(64 * kEmitWaves, 4) void k_emit_known(FusedArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kEmitWaves * kGImg];
  __shared__ uint32_t s_lut[512];
  const Geom& g = a.g;
  [[maybe_unused]] const int lane = lane_id();
  const int wave = (int)wave_id();
  uint32_t* gimg = lds + wave * kGImg;
  if (DO_G)
    for (uint32_t i = threadIdx.x; i < 512; i += blockDim.x) s_lut[i] = reinterpret_cast<const uint32_t*>(a.lut + 256)[kKnownTable + i];
  __syncthreads();  // the only workgroup barrier
  const uint64_t nrows = (uint64_t)g.rows * g.nplanes;
  // persistent waves: rows id, id + stride, ...
  const uint64_t stride = (uint64_t)gridDim.x * kEmitWaves;
  const uint64_t id0 = (uint64_t)xcd_remap(blockIdx.x, gridDim.x) * kEmitWaves +
                       (uint32_t)__builtin_amdgcn_readfirstlane(wave);  // (uniform, as the compiler sees it)
  for (uint64_t id = id0; id < nrows; id += stride) {
    const uint32_t plane = (uint32_t)(id / g.rows), row = (uint32_t)(id % g.rows);
    STAMP(0);
    uint64_t rr[WPL];
    uint32_t O;
    uint64_t Lf, Gb;
    if constexpr (ES) {
      eg_src_row<WPL>(a.esrc + (uint64_t)plane * a.slot_e, g, row, rr);
      O = a.row_o[id];
      Lf = DO_G ? a.glen[id] : 0;
      Gb = DO_G ? gb_abs(a, id, plane) : 0;
    } else {
      uint64_t cp_[WPL], cu_[WPL];
      row_load<WPL, PREDICT>(a.planes, g, plane, row, cp_, cu_);
      O = a.row_o[id];
      Lf = DO_G ? a.glen[id] : 0;
      Gb = DO_G ? gb_abs(a, id, plane) : 0;  // loaded with the row, not after the branch that uses it
      row_resid<WPL, PREDICT>(g, row, cp_, cu_, rr);
    }
    const uint64_t Eb = DO_E ? (a.ebase ? a.ebase[plane] : (uint64_t)plane * a.slot_e * 64) : 0;
    emit_known_row<WPL, PREDICT, DO_G, DO_E>(a, id, plane, row, rr, O, Lf, Gb, Eb, gimg, s_lut);
    STAMP(2);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // the next row reuses the LDS image
    __builtin_amdgcn_wave_barrier();
  }
}

// ---- EG source: one light emission kernel per row class ------------------------------------------
// With the residual rows read back from the EG stream (FusedArgs::esrc) the Golomb emission is split
// by the class the prefix kernels proved for the row (the LEN scan's lists): rows whose codewords
// all have k = 0 are shifted copies of the EG stream, inverted (k_emit_k0, no LDS), rows whose
// codewords all have k = 1 go through the byte tables and an LDS row image (k_emit_k1); mixed rows
// stay k_emit_rest's. Persistent waves, one row at a time, in the list order i, i + nw, ...
//
// Both kernels keep the memory system busy the same way: the next row's source words are loaded
// before the current row's output is stored, into the other of two word buffers (ping-pong, no
// register copies). gfx9's vmcnt counts stores with loads: a wave that loaded after storing would
// wait for its stores' acknowledgements every row. With the loads first, every load and store issued
// unconditionally (clamped indices, idle lanes storing to a.sink), the list entries read through the
// scalar cache (the kernels' stores are typed unsigned long long, apart from the entries' u64, and
// they hold no fence or workgroup barrier, so the compiler proves the entries unclobbered), the
// compiler waits for the loads alone.
__device__ __forceinline__ uint64_t rl64(uint64_t v, uint32_t l) {
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)l) << 32) |
         (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)l);
}

__device__ __forceinline__ uint64_t cls_ld(const FusedArgs& a, uint64_t i) { return a.cls[i]; }

// k = 0: the row's Golomb bits are R then the end-of-row '1' (GolombCoder.cpp:13-34 with k = 0: each
// sample's zeros and its '1'), i.e. the EG row ~R '1' (eg.cpp:20-37) with its first cols bits inverted.
// Output word t of the row (at bit Gb) holds row bits [64 t - g, 64 t - g + 64), g = Gb % 64: the
// stream bits from Bsrc + 64 t - g (Bsrc: the row in the EG slot), one funnel shift per word.
#ifndef BIC_K0_BATCH
// (8-byte lanes, pipelined batches of 3: C3 emission 162-165 -> 157-158 us; of 2: 159-162; of 4: 170-173.
// Batches of 2 keep k_emit_k01 at <= 128 VGPRs (113; batches of 3: 129), a fourth workgroup slot per CU.
// 16-byte lanes: 115 VGPRs at batches of 2, emission 167-168 us against 158-164).
// Round 6: batches of 2 with four workgroups per CU (BIC_K01_OCC 4, 113 VGPRs) --
// k_emit_k01 137 -> 132-137 us against 142-147 at batches of 3 and three per CU, same box
// (profiles/r06/ab_emission.txt gj25, gj26); the C3 step unchanged (k_emit_rest beside it takes the slack)
#define BIC_K0_BATCH 2
#endif
constexpr int kK0Batch = BIC_K0_BATCH;
// the k = 0 list's entries i0, i0 + nw, ... (one wave; i0 and nw wave-uniform)
template <int WPL, int BATCH = kK0Batch>
__device__ __forceinline__ void k0_rows(const FusedArgs& a, uint32_t i0, uint32_t nw) {
  const Geom& g = a.g;
  const int lane = lane_id();
  const uint32_t n = __hip_atomic_load(a.counter + 4, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const uint64_t L = (uint64_t)g.cols + 1;
  const uint64_t* S = a.esrc;
  if (i0 >= n) return;
  const uint32_t R = (n - i0 + nw - 1) / nw;  // the wave's rows
  struct Row {
    uint32_t id;
    uint64_t G;
    int64_t si;
    uint32_t d;
  };
  // row k of the wave (list entry i0 + k nw): where its output and its source bits are
  auto place = [&](uint32_t k) {
    const uint64_t e = i0 + (uint64_t)k * nw;
    Row r;
    const uint64_t e0 = cls_ld(a, 2 * e);
    r.id = (uint32_t)e0;
    // (the k = 0 entries carry the plane where the k = 1 ones carry the length, which is cols + 1 here:
    // no division by rows on the scalar unit)
    const uint32_t plane = (uint32_t)(e0 >> 32), row = r.id - plane * g.rows;
    const uint64_t Gs = cls_ld(a, 2 * e + 1);
    r.G = a.off_g ? Gs - (uint64_t)plane * a.slot_g * 64 + a.gbase[plane] * 64 : Gs;
    // stream bit of output word t's first bit: Bsrc - G % 64 + 64 t (>= -63: floor below)
    const int64_t s0 = (int64_t)((uint64_t)plane * a.slot_e * 64 + eg_src_bit0(g, row)) - (int64_t)(r.G & 63);
    r.si = s0 >> 6;
    r.d = (uint32_t)(s0 & 63);
    return r;
  };
  // Word groups 64 k .. 64 k + 63 of the output row. A group wholly inside the row (k >= 1 and before
  // the row's last word: C3's groups 1-3 of 5) needs no masks, clamps or fragment selects -- a uniform
  // branch on the row's scalar offsets -- and loads / stores through a scalar base plus the lane's
  // 32-bit offset: ~16 VALU per group instead of ~55 (the copies share each SIMD's VALU issue with the
  // k = 1 rows and k_emit_rest, and the younger waves wait for it: tools/k01_stamps.py)
  auto load = [&](const Row& r, uint64_t (&v)[WPL + 1]) {
    const int64_t jend = r.si + (int64_t)((r.d + (r.G & 63) + g.cols) >> 6);
    const uint64_t* sb = S + r.si;  // (r.si >= -1: only group 0 may start before the stream)
#pragma unroll
    for (int k = 0; k <= WPL; ++k) {
      if (k >= 1 && r.si + 64 * k + 63 <= jend) {
        v[k] = sb[64 * k + lane];
      } else {
        const int64_t j = r.si + 64 * k + lane;
        const int64_t jc = j > jend ? jend : j;
        v[k] = S[jc < 0 ? 0 : jc];
      }
    }
  };
  auto emit = [&](const Row& cur, uint64_t (&v)[WPL + 1]) {
    const uint32_t gs = (uint32_t)(cur.G & 63);
    const uint64_t w0 = cur.G >> 6, nwo = ((cur.G + L - 1) >> 6) - w0 + 1;  // output words (<= used + 2)
    const uint64_t eolw = (uint64_t)(g.cols + gs) >> 6, eolb = BIC_MSB >> ((g.cols + gs) & 63);
    const int64_t jend = cur.si + (int64_t)((cur.d + gs + g.cols) >> 6);
    unsigned long long* ob = reinterpret_cast<unsigned long long*>(a.out_g + w0);
#pragma unroll
    for (int k = 0; k <= WPL; ++k) {
      uint64_t nx = ((uint64_t)(uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v[k] >> 32), 0x130, 0xf, 0xf, true) << 32) |
                    (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v[k], 0x130, 0xf, 0xf, true);
      if (k < WPL) {
        const uint64_t n0 = rl64(v[k + 1 <= WPL ? k + 1 : k], 0);
        if (lane == 63) nx = n0;
      }
      if (k >= 1 && (uint64_t)(64 * k + 63) < nwo - 1) {  // interior group: a shifted, inverted copy
        const uint64_t x = ~(cur.d ? funnel64(bswap64(v[k]), bswap64(nx), 64 - cur.d) : bswap64(v[k]));
        class_store(reinterpret_cast<uint64_t*>(ob + 64 * k + lane), bswap64(x));
        continue;
      }
      const uint32_t t = 64 * k + lane;
      const int64_t j = cur.si + 64 * k + lane;
      const uint64_t vk = (j >= 0 && j <= jend) ? v[k] : 0ull;
      // (lane 63's next word: the next group's first, in range when that group is)
      const uint64_t hi = bswap64(vk);
      uint64_t x = ~(cur.d ? funnel64(hi, bswap64(nx), 64 - cur.d) : hi);
      // row bits outside [0, cols) are not the row's: before it (word 0's first gs bits) and from the
      // end-of-row '1' on
      if (t == 0) x &= ~0ull >> gs;
      if (t >= eolw) x = t == eolw ? (x & ~((eolb << 1) - 1)) | eolb : 0ull;
      const bool in = t < nwo;
      const bool whole = in && (t != 0 || gs == 0) && (t != nwo - 1 || ((cur.G + L) & 63) == 0);
      uint64_t* dst = whole ? a.out_g + w0 + t : (in ? a.gfrag + 2 * (uint64_t)cur.id + (t == 0 ? 0 : 1) : a.sink + lane);
      // (unsigned long long: a type apart from the u64 loads, so no load is taken to depend on it)
      // Only the last word group has lanes past the row (the row's 257-258 words of C3): those store
      // nothing (exec-masked, the instruction count unchanged) instead of writing the sink (emission
      // 158-161 -> 155-160 us on one box)
      if (k < WPL || in) class_store(dst, whole ? bswap64(x) : x);
    }
  };
  // rows in batches of BATCH: every row's loads issued before the first row's stores, so a wave
  // waits for its previous stores once per batch
  // software-pipelined: batch k + 1's loads issued before batch k's stores, so the wait for a batch's
  // loads never covers the previous batch's stores (vmcnt counts both, in order)
  Row ra[BATCH], rb[BATCH];
  uint64_t va[BATCH][WPL + 1], vb[BATCH][WPL + 1];
#pragma unroll
  for (int u = 0; u < BATCH; ++u) {
    ra[u] = place((uint32_t)u < R ? (uint32_t)u : 0u);
    load(ra[u], va[u]);
  }
  for (uint32_t k = 0; k < R; k += 2 * BATCH) {
#pragma unroll
    for (int u = 0; u < BATCH; ++u) {
      const uint32_t kk = k + BATCH + u;
      rb[u] = place(kk < R ? kk : k);
      load(rb[u], vb[u]);
    }
#pragma unroll
    for (int u = 0; u < BATCH; ++u)
      if (k + u < R) emit(ra[u], va[u]);
#pragma unroll
    for (int u = 0; u < BATCH; ++u) {
      const uint32_t kk = k + 2 * BATCH + u;
      ra[u] = place(kk < R ? kk : k);
      load(ra[u], va[u]);
    }
#pragma unroll
    for (int u = 0; u < BATCH; ++u)
      if (k + BATCH + u < R) emit(rb[u], vb[u]);
  }
}

// k = 1 rows: emit_known_row's byte-table path (encode_word_k1b into a 64-bit LDS row image, then
// write_row64_fixed); rows whose image exceeds the window are listed for k_rows_global.
#ifndef BIC_K1_BATCH
#define BIC_K1_BATCH 3
#endif
constexpr int kK1Batch = BIC_K1_BATCH;
// the k = 1 list's entries i0, i0 + nw, ... (one wave, with its LDS row image and the byte table): a static
// share (one ticket counter for every chunk of the ~32k k = 1 rows of C3: emission 157 -> 540 us; device-scope
// atomics on one word stall every wave and the memory channel holding it)
template <int WPL>
__device__ __forceinline__ void k1_rows(const FusedArgs& a, uint32_t i0, uint32_t nw, uint32_t* gimg,
                                        const uint32_t* s_lut) {
  const Geom& g = a.g;
  const int lane = lane_id();
  constexpr uint32_t kCapBits = (kGImg - kPad) * 32;
  const uint64_t nrows = (uint64_t)g.rows * g.nplanes;
  const uint32_t n = __hip_atomic_load(a.counter + 5, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (i0 >= n) return;
  const uint32_t R = (n - i0 + nw - 1) / nw;
  struct Row {
    uint32_t id, plane, row;
    uint64_t G, L;
  };
  auto place = [&](uint32_t k) {  // the wave's k-th row (entry i0 + k nw of the k = 1 list)
    const uint64_t e = nrows + i0 + (uint64_t)k * nw;
    Row r;
    const uint64_t e0 = cls_ld(a, 2 * e);
    r.id = (uint32_t)e0;
    r.L = e0 >> 32;
    r.plane = r.id / g.rows;
    r.row = r.id % g.rows;
    const uint64_t Gs = cls_ld(a, 2 * e + 1);
    r.G = a.off_g ? Gs - (uint64_t)r.plane * a.slot_g * 64 + a.gbase[r.plane] * 64 : Gs;
    return r;
  };
  // lane l holds the row's words l WPL .. (one wave scan per row, not per word group)
  constexpr int kV = WPL + 1;
  auto emit = [&](const Row& cur, const uint64_t (&v)[kV]) {
    if (cur.L > kCapBits) {  // (the LEN scan lists such rows as slow, never here: a length disagreement)
      if (lane == 0) atomicOr(&a.flags[3], 1u);
      return;
    }
    YSTAMP((1u << 18) + cur.id, 0);
    unsigned long long* z = reinterpret_cast<unsigned long long*>(gimg);
    for (int j = lane; j < kGImg / 2; j += 64) z[j] = 0ull;
    uint64_t rr[WPL];
    eg_src_assemble_lc<WPL>(g, cur.row, v, rr);
    YSTAMP((1u << 18) + cur.id, 1);
    uint64_t* img = reinterpret_cast<uint64_t*>(gimg);
    // the backward parity form (k1_pi): pi of each word's last column's right context (zeta) from the
    // next word holding a 1 -- in this lane, or the nearest lane to the right holding one (one ballot,
    // one bpermute); the row's first remainder bit from the first lane holding a 1
    const uint32_t tail = g.cols & 63u;  // columns of the row's last word (0: a full word)
    uint64_t xt[WPL], Zm[WPL];
    bool any = false;
    uint32_t lead = 0;
#pragma unroll
    for (int t = 0; t < WPL; ++t) {
      const uint32_t w = (uint32_t)lane * WPL + t;
      const uint64_t valid = w < g.used ? (w == g.used - 1 ? g.trail : ~0ull) : 0ull;
      xt[t] = rr[t] | ((w == g.used - 1 && tail) ? (BIC_MSB >> tail) : 0ull);  // + the end-of-row 1
      Zm[t] = ~xt[t] & valid;
    }
#pragma unroll
    for (int t = WPL - 1; t >= 0; --t)
      if (xt[t]) {
        lead = (uint32_t)__builtin_clzll(xt[t]) & 1u;
        any = true;
      }
    const uint64_t m1 = __ballot(any);
    const uint64_t nm = m1 & ~((2ull << lane) - 1ull);  // the lanes right of this one holding a 1
    const uint32_t ln = (uint32_t)__shfl((int)lead, nm ? (int)__builtin_ctzll(nm) : lane);
    const uint32_t lf = (uint32_t)__shfl((int)lead, m1 ? (int)__builtin_ctzll(m1) : 0);
    uint32_t zc = nm ? ln : 0u;  // (no 1 to the right: the end-of-row 1 follows the last word)
    uint32_t zeta[WPL];
#pragma unroll
    for (int t = WPL - 1; t >= 0; --t) {
      zeta[t] = zc;
      if (xt[t]) zc = (uint32_t)__builtin_clzll(xt[t]) & 1u;
    }
    const uint32_t* T = s_lut;
    uint64_t A[WPL], B[WPL];
    uint32_t lw[WPL], lsum = 0;
#pragma unroll
    for (int t = 0; t < WPL; ++t) {
      const uint32_t w = (uint32_t)lane * WPL + t;
      const uint64_t Pi = k1_pi(xt[t], Zm[t], zeta[t]);
      uint64_t hi = 0, lo = 0;
      uint32_t L = 0;
      if (w < g.used) {
        if (w == g.used - 1 && tail) L = k1_word_last(rr[t], Pi, tail, hi, lo);
        else L = k1_word_full(rr[t], Pi, T, hi, lo);
      }
      left128(hi, lo, L ? L : 128u, A[t], B[t]);
      lw[t] = L;
      lsum += L;
    }
    const uint32_t inc = wave_incl_sum_u32(lsum);
    uint32_t off = 1u + inc - lsum;  // (bit 0: the first run's remainder)
    const uint32_t tot = 1u + lane63_u32(inc) + (tail ? 0u : 1u);
#pragma unroll
    for (int t = 0; t < WPL; ++t) {
      place128_64(img, off, A[t], B[t], lw[t]);
      off += lw[t];
    }
    if (lane == 0) {
      if (lf && m1) lds_or64(img, 0, BIC_MSB);
      if (!tail) lds_or64(img, (tot - 1) >> 6, BIC_MSB >> ((tot - 1) & 63));  // the end-of-row '1'
      if (tot != cur.L) atomicOr(&a.flags[3], 1u);  // the closed-form length disagrees with the emission
    }
    YSTAMP((1u << 18) + cur.id, 2);
    write_row64_fixed<(kCapBits / 64 + 1 + 63) / 64>(img, cur.L, cur.G, a.out_g, a.gfrag + 2 * (uint64_t)cur.id,
                                                     a.sink);
    YSTAMP((1u << 18) + cur.id, 3);
  };
  auto load = [&](const Row& r, uint64_t (&v)[kV]) {
    eg_src_load_lc<WPL>(a.esrc + (uint64_t)r.plane * a.slot_e, g, r.row, v);
  };
  for (uint32_t k = 0; k < R; k += kK1Batch) {  // (batches as k_emit_k0)
    Row r[kK1Batch];
    uint64_t v[kK1Batch][kV];
#pragma unroll
    for (int u = 0; u < kK1Batch; ++u) {
      r[u] = place(k + u < R ? k + u : k);
      load(r[u], v[u]);
    }
#pragma unroll
    for (int u = 0; u < kK1Batch; ++u)
      if (k + u < R) emit(r[u], v[u]);
  }
}

// The rows the prefix kernels leave to this launch: Golomb rows with mixed k (per-codeword k,
// encode_word; among the walked rows, counter[2]) and the EG row holding the plane's first 1 (with
// its inserted '0'; walked, or listed by k_scan_rows in counter[3]). One workgroup per row, one word
// per lane (wide_prefix), one LDS image per workgroup.
// One row of k_emit_rest (a whole workgroup, one word per lane; `walked`: an entry of the walk list,
// skipped unless mixed-k or its plane's first-1 row -- uniform over the workgroup). Ends with a
// workgroup barrier whenever it touched the images or sh (they are reused by the next row).
template <bool PREDICT, bool DO_G, bool DO_E>
__device__ __forceinline__ void rest_row(const FusedArgs& a, uint64_t id, bool walked, uint32_t* gimg, uint32_t* eimg,
                                         const uint32_t* s_lut, uint32_t* sh, int* sf) {
  const Geom& g = a.g;
  const int lane = lane_id(), v = (int)wave_id(), nw = blockDim.x >> 6;
  const uint32_t w = 64 * v + lane;
  constexpr uint32_t kCapBits = (kGImg - kPad) * 32;
  {
    const uint32_t plane = (uint32_t)(id / g.rows), row = (uint32_t)(id % g.rows);
    const uint32_t O = a.row_o[id];
    const uint64_t Lf = DO_G ? a.glen[id] : 0;
    const uint64_t L = Lf & kLenMask;
    const bool k0 = (Lf & kK0Row) != 0, k1 = (Lf & kK1Row) != 0;
    if (walked) {  // a walked row: skip it unless mixed or the first-1 row (uniform over the workgroup)
      const uint64_t onext = row + 1 < g.rows ? a.row_o[id + 1] : a.pones[plane];
      if (!(L && !k0 && !k1) && !(DO_E && O == 0 && onext > 0)) return;
    }
    const bool gmix = DO_G && L && !k0 && !k1 && L <= kCapBits;
    uint64_t rr[1];
    if (!PREDICT && a.esrc) rr[0] = eg_src_word(a.esrc + (uint64_t)plane * a.slot_e, g, row, w);
    else resid_row<1, PREDICT>(a.planes, g, plane, row, rr, 64 * v);
    const uint64_t x = rr[0];
    const WideRow p = wide_prefix(x, w, O + row, sh);
    const bool f_here = DO_E && O == 0 && p.ones > 0;
    if (gmix) {
      uint4* z = reinterpret_cast<uint4*>(gimg);
      for (uint32_t j = threadIdx.x; j < kGImg / 4; j += blockDim.x) z[j] = make_uint4(0, 0, 0, 0);
    }
    if (f_here) {  // EG image (~R, pad-masked, EOL '1'); write_row inserts the '0' after the first 1
      const int fc = wave_min(x ? (int)(w * 64 + __builtin_clzll(x)) : INT_MAX);
      if (lane == 0) sf[v] = fc;
      if (w < g.used) {
        const uint64_t e = ~x & (w == g.used - 1 ? g.trail : ~0ull);
        eimg[2 * w] = (uint32_t)(e >> 32);
        eimg[2 * w + 1] = (uint32_t)e;
      }
      if (threadIdx.x < kPad + 1) eimg[2 * g.used + threadIdx.x] = 0;
    }
    __syncthreads();
    if (f_here) {
      if (threadIdx.x == 0) eimg[g.cols >> 5] |= 0x80000000u >> (g.cols & 31);  // EOL '1'
      __syncthreads();
      int fcol = INT_MAX;
      for (int u = 0; u < nw; ++u) fcol = min(fcol, sf[u]);
      const uint64_t Le = (uint64_t)g.cols + 2;
      const uint64_t Ge_rel = (uint64_t)row * (g.cols + 1);
      const uint64_t cap = a.slot_e * 64;
      if (Ge_rel + Le <= cap)
        write_row(eimg, Le, (a.ebase ? a.ebase[plane] : (uint64_t)plane * cap) + Ge_rel, (int64_t)fcol + 1, a.out_e,
                  a.efrag + 2 * id, threadIdx.x, blockDim.x);
    }
    if (gmix) {
      const uint32_t arow = row * (g.cols + 1);
      const bool eol = w == g.used - 1;
      const LaneEnc e = encode_word(x, w, p.n, p.jp, arow, eol, g.cols, ByteTables{s_lut, a.lut});
      const uint32_t inc = wave_incl_sum_u32(e.len);
      if (lane == 63) sh[v] = inc;
      __syncthreads();
      uint32_t wb = 0, tot = 0;
      for (int u = 0; u < nw; ++u) {
        if (u < v) wb += sh[u];
        tot += sh[u];
      }
      const uint32_t off = wb + inc - e.len;
      if (!e.lng) {
        place_small(gimg, off, e.head, e.k0);
        place128(gimg, off + e.k0 + e.z, e.t0, e.t1, e.tlen);
      } else {
        LdsSink ls{gimg, 0, 0};
        emit_word(ls, off, x, w, p.n, p.jp, arow, eol, g.cols);
        ls.flush();
      }
      __syncthreads();
      if (threadIdx.x == 0 && tot != L) atomicOr(&a.flags[3], 1u);  // word_len disagrees with the emission
      write_row(gimg, L, gb_abs(a, id, plane), -1, a.out_g, a.gfrag + 2 * id, threadIdx.x,
                blockDim.x);
    }
    __syncthreads();  // the images and sh are reused by the next row
  }
}

template <bool PREDICT, bool DO_G, bool DO_E>
__global__ __launch_bounds__(256) void k_emit_rest(FusedArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t gimg[kGImg];
  __shared__ __attribute__((aligned(16))) uint32_t eimg[kEImg];
  __shared__ uint32_t s_lut[512];
  __shared__ uint32_t sh[16];  // (wide_prefix: up to 8 waves)
  __shared__ int sf[4];
  const int lane = lane_id(), v = (int)wave_id(), nw = blockDim.x >> 6;
  if (DO_G)
    for (uint32_t i = threadIdx.x; i < 512; i += blockDim.x) s_lut[i] = reinterpret_cast<const uint32_t*>(a.lut + 256)[i];
  __syncthreads();
  // the scan's list (first-1 rows it did not walk), then the walked rows that are mixed-k or hold
  // their plane's first 1
  const uint32_t nrest = __hip_atomic_load(a.counter + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const uint32_t nwalk = DO_G ? __hip_atomic_load(a.counter + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
  for (uint32_t i = blockIdx.x; i < nrest + nwalk; i += gridDim.x)
    rest_row<PREDICT, DO_G, DO_E>(a, i < nrest ? a.rest_ids[i] : a.walk_ids[i - nrest], i >= nrest, gimg, eimg, s_lut,
                                  sh, sf);
  // the class kernels' path (a.cls): the LEN scan listed every row too long for an LDS image, so the
  // slow rows are written here, one wave per row, overlapping the class kernels (no k_rows_global)
  if (DO_G && !PREDICT && a.cls) {
    const uint32_t nslow = __hip_atomic_load(a.slow_n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (uint32_t li = blockIdx.x * nw + v; li < nslow; li += gridDim.x * nw) row_global<false>(a, a.slow_ids[li], lane);
  }
}

// Both classes in one launch: persistent waves take their share of each list, the k = 0 rows first.
// The waves reach the byte-table rows at different times, so the copies (memory-bound) and the
// byte-table rows (issue-bound) run side by side instead of one launch after the other. (Odd waves
// starting on the k = 1 rows measured 196-198 µs against 192-193, round 4.)
#ifndef BIC_K01_OCC
#define BIC_K01_OCC 4  // a minimum of workgroups (one wave per SIMD each) per CU for k_emit_k01 (0: none;
                       // the compiler then took 133 VGPRs, three per CU)
#endif
// At most 112 registers, one fewer than the compiler takes by itself: four workgroups then leave 64 of a
// SIMD's 512 for one wave of k_emit_rest (59 registers, allocated as 64), whose rows otherwise wait for
// these persistent waves to end (k_emit_rest ended 3-9 us after this kernel). The attribute counts
// architectural registers, half of this target's unified file, hence 56; launch_staged_emit checks what the
// build gave (k01_regs_checked).
constexpr int kK01Regs = 112;
template <int WPL>
__attribute__((amdgpu_num_vgpr(kK01Regs / 2)))
__global__ __launch_bounds__(256, BIC_K01_OCC ? BIC_K01_OCC : 1) void k_emit_k01(FusedArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[4 * kGImg];
  __shared__ uint32_t s_lut[512];
  const int lane = lane_id();
  [[maybe_unused]] const uint32_t gwv = (1u << 19) + 8192u + blockIdx.x * 4u + wave_id();  // (XSTAMP index)
  XSTAMP(gwv, 0);
  uint32_t* gimg = lds + wave_id() * kGImg;
  // every wave writes the whole table itself (the same values as the others): its own reads then
  // follow its own writes, and the kernel needs no workgroup barrier
  for (uint32_t i = lane; i < 512; i += 64) s_lut[i] = reinterpret_cast<const uint32_t*>(a.lut + 256)[kK1Table + i];
  const uint32_t nb = gridDim.x, nw = nb * 4;
  // (the wave index through readfirstlane: the compiler then knows i0, and every branch on it, is uniform)
  const uint32_t i0 = xcd_remap(blockIdx.x, nb) * 4 + wave_id();
  k0_rows<WPL>(a, i0, nw);
  XSTAMP(gwv, 1);
  k1_rows<WPL>(a, i0, nw, gimg, s_lut);
  XSTAMP(gwv, 3);
}

__global__ __launch_bounds__(1024) void k_plane_bases(FusedArgs a) {
  __shared__ uint64_t tmp[17];
  plane_bases(a, tmp);
}

// Combine the fragments of the words rows share: the row holding a shared word's first bit
// owns it and ORs in the head fragments of the following rows that start inside that word.
__global__ __launch_bounds__(256) void k_fixup(const uint64_t* __restrict__ boff, const uint64_t* __restrict__ len,
                                               const uint64_t* __restrict__ frag, uint64_t* __restrict__ out,
                                               const uint64_t* __restrict__ boff2, const uint64_t* __restrict__ len2,
                                               const uint64_t* __restrict__ frag2, uint64_t* __restrict__ out2,
                                               uint32_t rows, uint64_t nrows, uint32_t second,
                                               const uint64_t* __restrict__ gbase = nullptr, uint64_t slot_bits = 0,
                                               const uint64_t* __restrict__ efix = nullptr, uint64_t* eout = nullptr,
                                               uint64_t eslot = 0, uint32_t enp = 0, uint32_t* zc = nullptr,
                                               uint64_t* zr = nullptr, uint64_t zn = 0) {
  eg_fix_bit(efix, eout, eslot, enp);  // (EG source: after every reader of the residual rows)
  if (zr) {  // single / two-pass encoder: its counters and 2 zn look-back records cleared for the next call
    const uint64_t zi = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (zi < zn) {
      zr[zi] = 0;
      zr[zn + zi] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x < 64) zc[threadIdx.x] = 0;
  }
  // blocks [second, ...) serve the second stream (EG) when both streams are written
  if (blockIdx.x >= second) {
    boff = boff2;
    len = len2;
    frag = frag2;
    out = out2;
    gbase = nullptr;
  }
  const uint64_t id = (uint64_t)(blockIdx.x >= second ? blockIdx.x - second : blockIdx.x) * 256 + threadIdx.x;
  if (id >= nrows) return;
  const uint64_t pend = (id / rows + 1) * (uint64_t)rows;
  // gbase: the first stream's offsets are slot-relative, its planes packed from word gbase[plane]
  const uint64_t sft = gbase ? gbase[id / rows] * 64 - (id / rows) * slot_bits : 0;
  // every load this row usually needs is issued at once (the row, its two fragments, the next row's
  // offset, length and head fragment): one memory round trip instead of three dependent ones
  const bool nx = id + 1 < pend;
  const uint64_t G = boff[id] + sft, L = len[id] & kLenMask;  // (the staged encoder's glen carries row flags)
  const uint64_t f0 = frag[2 * id], f1 = frag[2 * id + 1];
  const uint64_t G1 = nx ? boff[id + 1] + sft : 0, L1 = nx ? len[id + 1] & kLenMask : 0, h1 = nx ? frag[2 * id + 2] : 0;
  if (L == 0) return;
  const uint64_t wt = (G + L - 1) >> 6, wh = G >> 6;
  const uint64_t wb = wt * 64;
  if (wb < G) return;                     // the word's first bit belongs to an earlier row
  if (wb + 64 <= G + L) return;           // a whole word of this row: already stored
  uint64_t v = (wh == wt) ? f0 : f1;
  if (!nx || L1 == 0 || G1 >= wb + 64) {
    out[wt] = bswap64(v);
    return;
  }
  v |= h1;
  for (uint64_t r2 = id + 2; r2 < pend; ++r2) {
    if ((len[r2] & kLenMask) == 0 || boff[r2] + sft >= wb + 64) break;
    v |= frag[2 * r2];
  }
  out[wt] = bswap64(v);
}

// the fixup of any row encoder that leaves its shared words as fragments (bic_egad.hip)
void launch_fixup_rows(hipStream_t s, const uint64_t* boff, const uint64_t* len, const uint64_t* frag, uint64_t* out,
                       uint32_t rows, uint64_t nrows) {
  const uint32_t grid = (uint32_t)((nrows + 255) / 256);
  k_fixup<<<grid, 256, 0, s>>>(boff, len, frag, out, boff, len, frag, out, rows, nrows, 0xffffffffu);
}

// ------------------------------------------------------------------------------------
// The scratch arena's layout, stated once: every block in order with its size in bytes (n = rows *
// planes; every size a multiple of 8). Points a's fields into the arena at base and returns its size.
static size_t fused_layout(const Geom& g, FusedArena& a, void* base) {
  const size_t n = (size_t)g.rows * g.nplanes, np = g.nplanes;
  uintptr_t p = reinterpret_cast<uintptr_t>(base);
  auto take = [&](auto*& field, size_t bytes) {
    field = reinterpret_cast<std::remove_reference_t<decltype(field)>>(p);
    p += bytes;
  };
  take(a.counter, 256);
  take(a.ones_rec, n * 8), take(a.bits_rec, n * 8);
  take(a.gboff, n * 8), take(a.glen, n * 8), take(a.gfrag, 2 * n * 8), take(a.gslow, n * 8);
  take(a.eboff, n * 8), take(a.elen, n * 8), take(a.efrag, 2 * n * 8), take(a.slow_ids, n * 8);
  take(a.krec, n * kMaxStrips * 16), take(a.kpos, n * kMaxStrips * 4), take(a.sones, n * kMaxStrips * 4);
  take(a.row_o, n * 4), take(a.walk_ids, n * 4), take(a.rest_ids, n * 4), take(a.walk_o, n * 4);
  take(a.pones, np * 8), take(a.gbase, np * 8), take(a.ebase, np * 8), take(a.efix, np * 8);
  take(a.cls, 2 * n * 16);  // the k = 0 list and the k = 1 list, two u64 words per entry
  take(a.sink, 512);
  char* unassigned;  // (kept: the arena's size stays what it was)
  take(unassigned, 1024 + 64 + 64);
  a.slow_n = a.counter + 1;
  a.zero_bytes = 256 + n * 16;  // counter, ones_rec, bits_rec
  return p - reinterpret_cast<uintptr_t>(base);
}

size_t fused_scratch_bytes(const Geom& g) {
  FusedArena a;
  return fused_layout(g, a, nullptr);
}

FusedArena carve_fused_arena(void* base, const Geom& g) {
  FusedArena a;
  fused_layout(g, a, base);
  return a;
}

// (a plane's pixels fit 32 bits: row_o, and the ONES scan's packed pair, hold a plane's 1-count in 32)
bool fused_supported(const Geom& g) { return g.used <= 256 && (uint64_t)g.rows * g.cols <= 0xffffffffull; }

#ifdef BIC_STAMPS
int read_stamps(uint64_t* host, size_t n) {
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_stamps), n * 8, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : 3;
}
#endif

// Staged encoder: per-row counts, scans and Golomb lengths -- every row's offsets known up front.
void launch_staged_prefix(hipStream_t s, const FusedCall& c, bool golomb_lengths) {
  const FusedArgs a = make_fused_args(c);
  const Geom& g = c.g;
  if (!c.rq.counted) launch_row_ones(s, g, c.planes, c.predict, c.ar.sones, c.ar.krec, c.ar.kpos, c.ar.counter);
  const uint32_t sgrid = (g.rows + kScanChunk - 1) / kScanChunk * g.nplanes;
  if (golomb_lengths) k_scan_rows<true, true><<<sgrid, kScanThreads, 0, s>>>(a);
  else k_scan_rows<true, false><<<sgrid, kScanThreads, 0, s>>>(a);
  if (golomb_lengths) {
    const uint32_t wwv = (kWalkSplit * g.used + 63) / 64;  // k_row_walk: waves per row (<= 8)
    if (c.predict) k_row_walk<true><<<kWalkWaves / wwv, 64 * wwv, 0, s>>>(a);
    else k_row_walk<false><<<kWalkWaves / wwv, 64 * wwv, 0, s>>>(a);
    k_scan_rows<false, false><<<sgrid, kScanThreads, 0, s>>>(a);  // (+ the row index)
  }
  // packed output: the planes' start words (the rows' Golomb offsets stay slot-relative: gb_abs)
  // -- as the LEN scan's last workgroup instead, its device-scope release fences (an L2 write-back
  // per workgroup) made C4's prefix 99 -> 153 us
  if (a.off_g || a.off_e) k_plane_bases<<<1, 1024, 0, s>>>(a);
}

// one resident wave set: as many workgroups per CU as the instance's registers and LDS allow
// (WPL = 4: <= 128 VGPRs, 4; WPL = 1: 7), queried once per instance
static int emit_occupancy(const void* fn) {
  int occ = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, 64 * kEmitWaves, 0) != hipSuccess || occ < 1) occ = 4;
  return std::min(occ, 8);
}
// k_emit_k01's register bound (kK01Regs) as built: more registers, or any scratch, and k_emit_rest no
// longer fits beside it or its rows spill -- said once, since the streams stay right and only time is lost
static bool k01_regs_checked(const void* fn) {
  hipFuncAttributes fa{};
  if (hipFuncGetAttributes(&fa, fn) != hipSuccess) return false;
  const bool ok = fa.numRegs <= kK01Regs && fa.localSizeBytes == 0;
  if (!ok)
    std::fprintf(stderr, "bic_fused.hip: k_emit_k01 was built with %d registers and %zu bytes of scratch (expected <= %d, 0)\n",
                 fa.numRegs, (size_t)fa.localSizeBytes, kK01Regs);
  return ok;
}

// Staged encoder: every row written independently, persistent grids (more rows per wave when the
// image is larger).
void launch_staged_emit(hipStream_t s, const FusedCall& c, const EmitStreams& es) {
  const FusedArgs a = make_fused_args(c);
  const Geom& g = c.g;
  const bool dg = a.out_g != nullptr, de = a.out_e != nullptr && !a.esrc;  // de: the emission writes EG
  if (!dg && !de) return;  // EG source without Golomb: the count pass and the ONES scan wrote it all
  const uint64_t nrows = (uint64_t)g.rows * g.nplanes;
  static thread_local int cus = 0;  // the device's CU count, asked once
  if (!cus) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (cus <= 0) cus = 256;
  }
  // k_emit_rest (listed rows, latency bound: few workgroups) first, on the aux stream when there
  // is one, so that it can overlap the main launch, which skips the listed rows' parts
  const uint32_t nwv = (g.used + 63) / 64;  // waves per row in k_emit_rest
  const uint32_t rgrid = (uint32_t)std::min<uint64_t>(nrows, (uint64_t)cus * 32 / nwv);  // 32 waves per CU (16: C4 +6 us; 4: C3 +30 us -- the listed rows are latency-bound)
  hipStream_t rs = s;
  if (es.aux && es.fork && es.join && hipEventRecord(es.fork, s) == hipSuccess &&
      hipStreamWaitEvent(es.aux, es.fork, 0) == hipSuccess)
    rs = es.aux;
  // (bic_prof_*: events around the main emission kernel alone, on its stream s -- the roofline kernel's
  // launch, without the fork / join of the second stream; null: not timed)
  auto main_ev = [&](hipEvent_t e) {
    if (e && hipEventRecord(e, s) == hipSuccess && e == es.main1 && es.main_rec) *es.main_rec = true;
  };
  using Kernel = void (*)(FusedArgs);
  auto emit = [&](Kernel rest, Kernel main, int occ) {  // (main: workgroups of kEmitWaves waves)
    rest<<<rgrid, 64 * nwv, 0, rs>>>(a);
    main_ev(es.main0);
    const uint64_t egrid = std::min<uint64_t>((nrows + kEmitWaves - 1) / kEmitWaves, (uint64_t)cus * (uint32_t)occ);
    main<<<(uint32_t)egrid, 64 * kEmitWaves, 0, s>>>(a);
    main_ev(es.main1);
  };
  if (a.esrc) {  // Golomb alone, the residual rows from the EG stream
    with_wpl(g, [&](auto w) {
      if (a.cls) {  // one kernel for the two row classes
        static const int occ = emit_occupancy(reinterpret_cast<const void*>(&k_emit_k01<w()>));
        [[maybe_unused]] static const bool regs = k01_regs_checked(reinterpret_cast<const void*>(&k_emit_k01<w()>));
        emit(k_emit_rest<false, true, false>, k_emit_k01<w()>, occ);
      } else {
        static const int occ = emit_occupancy(reinterpret_cast<const void*>(&k_emit_known<w(), false, true, false, true>));
        emit(k_emit_rest<false, true, false>, k_emit_known<w(), false, true, false, true>, occ);
      }
    });
  } else {
    with_row_kernel(g, c.predict != 0, dg, de, [&](auto w, auto p, auto cg, auto ce) {
      static const int occ = emit_occupancy(reinterpret_cast<const void*>(&k_emit_known<w(), p(), cg(), ce()>));
      emit(k_emit_rest<p(), cg(), ce()>, k_emit_known<w(), p(), cg(), ce()>, occ);
    });
  }
  if (rs != s && (hipEventRecord(es.join, rs) != hipSuccess || hipStreamWaitEvent(s, es.join, 0) != hipSuccess))
    (void)hipStreamSynchronize(rs);  // no join event: wait on the host rather than race
}

// The LDS-overflow rows and the words adjacent rows share.
void launch_fused_finish(hipStream_t s, const FusedCall& c) {
  const FusedArgs a = make_fused_args(c);
  const Geom& g = c.g;
  const FusedArena& ar = c.ar;
  const bool staged = c.mode == kEncStaged;
  const bool dg = a.out_g != nullptr, de = a.out_e != nullptr && !a.esrc;
  const uint64_t nrows = (uint64_t)g.rows * g.nplanes;
  const uint32_t fgrid = (uint32_t)((nrows + 255) / 256);
  // a fixed small grid walks the list of LDS-overflow rows (usually empty); block 0 also clears
  // the EG source's one bit per plane (eg_fix_bit)
  // (a.cls: k_emit_rest wrote the slow rows; single kernel: k_encode_rows did)
  if ((dg && c.mode != kEncSingle && !a.cls) || (!dg && a.esrc)) {
    if (c.predict) k_rows_global<true><<<dg ? 256 : 1, 256, 0, s>>>(a);
    else k_rows_global<false><<<dg ? 256 : 1, 256, 0, s>>>(a);
  }
  if (!dg && !de) return;
  k_fixup<<<dg && de ? 2 * fgrid : fgrid, 256, 0, s>>>(dg ? ar.gboff : ar.eboff, dg ? ar.glen : ar.elen,
                                                      dg ? ar.gfrag : ar.efrag, dg ? a.out_g : a.out_e,
                                                      ar.eboff, ar.elen, ar.efrag, a.out_e, g.rows, nrows,
                                                      dg && de ? fgrid : 0xffffffffu,
                                                      dg && staged && a.off_g ? ar.gbase : nullptr,
                                                      a.slot_g * 64, dg ? a.efix : nullptr, a.out_e, a.slot_e, g.nplanes,
                                                      ar.counter, !staged ? ar.ones_rec : nullptr, nrows);
}

}  // namespace bic

#ifdef BIC_STAMPS  // the stamps build is one unit: the look-back kernels write the same g_stamps
#include "bic_fused_lookback.hip"
#endif
