// bic_fused_lookback.hip -- the row encoders that resolve the dependencies between rows with
// decoupled look-backs inside one launch. The staged encoder (bic_fused.hip) is the default; these
// serve the small batches (bic_capi_rows.cpp staged_pays; BIC_OPT_SINGLE_KERNEL forces the single kernel)
// and are its cross-checks (BIC_OPT_TWO_PASS). The single kernel (k_encode_rows):
//  * tiles are claimed in order through an atomic ticket, so every tile a workgroup looks back
//    at was claimed earlier and is running or finished (no deadlock, whatever the dispatch order);
//  * the tile's 1-count is published at once and a decoupled look-back over the earlier tiles
//    of the plane yields the number of samples before each row (the Golomb coder state);
//  * lane strings are OR'd into an LDS row image; the tile's bit length is published and a
//    second look-back gives its offset.
// The two-pass option (k_len_rows, k_emit_rows) computes lengths and offsets first and then
// writes every row independently; same output, slower.
// Inter-workgroup records are 8-byte {flag, value} granules written and polled with
// agent-scope atomics (cdna_hip_programming.md §6 Guideline 16, R2), spins bounded.
#include "bic_fused.h"

namespace bic {

// One workgroup = one TILE of kTileRows consecutive rows of one plane (one wave per row). Tiles
// are claimed in order through one atomic ticket counter with the planes interleaved (tile t ->
// plane t % nplanes), so the planes' look-back chains advance side by side and any idle CU takes
// the oldest pending tile of any plane; one look-back per tile (by wave 0) serves its rows, which
// combine their counts through LDS. (Per-plane counters bound to blockIdx were measured slower:
// 793-918 us vs 682 us for C3, the claims themselves are not the limit.)
template <int WPL, bool PREDICT, bool DO_G, bool DO_E>
__global__ __launch_bounds__(64 * kTileRows, 8) void k_encode_rows(FusedArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kTileRows * (kGImg + kEImg)];
  __shared__ uint64_t sh_cnt[kTileRows], sh_len[kTileRows], sh_pre[2];
  __shared__ uint32_t sh_tile;
  __shared__ uint32_t s_lut[512];  // k = 1, 2 byte tables
  const Geom& g = a.g;
  // (the wave index left divergent here: as a scalar the compiler re-schedules this kernel's row loop
  // and C2 measured 0.032 -> 0.033-0.035 ms)
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  uint32_t* gimg = lds + wave * (kGImg + kEImg);
  uint32_t* eimg = gimg + kGImg;
  const uint32_t tpp = (g.rows + kTileRows - 1) / kTileRows;  // tiles per plane
  if (threadIdx.x == 0) sh_tile = atomicAdd(a.counter, 1u);
  if (threadIdx.x < 512) s_lut[threadIdx.x] = reinterpret_cast<const uint32_t*>(a.lut + 256)[threadIdx.x];
  __syncthreads();
  const uint64_t tile = sh_tile;
  if (tile >= (uint64_t)tpp * g.nplanes) return;  // uniform over the workgroup
  const uint32_t plane = (uint32_t)(tile % g.nplanes), trow = (uint32_t)(tile / g.nplanes);
  const uint64_t rbase = (uint64_t)plane * tpp;  // this plane's first tile record
  const uint64_t rid = rbase + trow;             // this tile's record
  const uint32_t row = trow * kTileRows + wave;
  const bool valid = row < g.rows;
  const uint64_t id = (uint64_t)plane * g.rows + row;  // per-row output records
  STAMP(0);

  // ---- residual row -> EG image (~R, pad-masked, EOL '1'); 1-count; first 1 ----------------
  uint32_t ones = 0;
  int fcol = INT_MAX;
  if (valid) {
    if constexpr (DO_G) lds_image_zero32(gimg, kGImg / 4);  // the Golomb image (row loads in flight)
    uint64_t rr[WPL];
    resid_row<WPL, PREDICT>(a.planes, g, plane, row, rr);
#pragma unroll
    for (int t = 0; t < WPL; ++t) {
      const uint32_t w = t * 64 + lane;
      const uint64_t r = rr[t];
      ones += (uint32_t)__popcll(r);
      if (r && fcol == INT_MAX) fcol = (int)(w * 64 + __builtin_clzll(r));
      if (w < g.used) {
        const uint64_t v = ~r & (w == g.used - 1 ? g.trail : ~0ull);
        eimg[2 * w] = (uint32_t)(v >> 32);
        eimg[2 * w + 1] = (uint32_t)v;
      }
    }
    if (lane < kPad + 1) eimg[2 * g.used + lane] = 0;
    ones = wave_sum_u32(ones);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) eimg[g.cols >> 5] |= 0x80000000u >> (g.cols & 31);  // EOL '1'
  }
  STAMP(1);
  if (lane == 0) sh_cnt[wave] = ones;
  __syncthreads();

  // ---- samples before this row: ones of earlier rows (+ one EOL sample per row) ----
#ifdef BIC_STAMPS
  if (a.known) {
    if (threadIdx.x == 0) sh_pre[0] = g_known[0][rid];
  } else
#endif
  if (wave == 0) {
    uint64_t tile_ones = 0;
    for (int q = 0; q < kTileRows; ++q) tile_ones += sh_cnt[q];
    uint64_t O = 0;
    if (trow == 0) {
      if (lane == 0) rec_store(&a.ones_rec[rid], kInc | tile_ones);
    } else {
      if (lane == 0) rec_store(&a.ones_rec[rid], kAgg | tile_ones);
      O = lookback(a.ones_rec, rbase, rid, a.flags);
      if (lane == 0) rec_store(&a.ones_rec[rid], kInc | (O + tile_ones));
    }
    if (lane == 0) sh_pre[0] = O;
#ifdef BIC_STAMPS
    if (lane == 0 && rid < (1u << 17)) g_known[0][rid] = O;
#endif
  }
  __syncthreads();
  STAMP(2);
  uint64_t O = sh_pre[0];
  for (int q = 0; q < wave; ++q) O += sh_cnt[q];

  // ---- Golomb length of the row (word_len: no codewords formed), published for the tile at once:
  // the tiles after this one find its bit count before its codewords exist, so the bit-offset
  // look-back does not wait on any tile's emission. Wave 0 looks back while the others emit. ----
  uint64_t L = 0;
  if constexpr (DO_G) {
    if (valid) {
      StepState st{(uint32_t)(O + row), -1};
      const uint32_t arow = row * (g.cols + 1);
      uint32_t ll = 0;
      for (uint32_t w0 = 0; w0 < g.used; w0 += 64) {
        const uint32_t w = w0 + lane;
        const uint64_t x = img_resid(eimg, g, w);
        uint32_t n;
        int jp;
        step_prefix(x, w, st, n, jp);
        uint32_t kor = 0;
        ll += word_len(x, w, n, jp, arow, w == g.used - 1, g.cols, kor);
      }
      L = wave_sum_u32(ll);
    }
    if (lane == 0) sh_len[wave] = L;
    __syncthreads();
#ifdef BIC_STAMPS
    if (a.known) {
      if (threadIdx.x == 0) sh_pre[1] = g_known[1][rid];
    } else
#endif
    if (wave == 0) {
      uint64_t tile_bits = 0;
      for (int q = 0; q < kTileRows; ++q) tile_bits += sh_len[q];
      uint64_t Gt = 0;
      if (trow == 0) {
        if (lane == 0) rec_store(&a.bits_rec[rid], kInc | tile_bits);
      } else {
        if (lane == 0) rec_store(&a.bits_rec[rid], kAgg | tile_bits);
        Gt = lookback(a.bits_rec, rbase, rid, a.flags);
        if (lane == 0) rec_store(&a.bits_rec[rid], kInc | (Gt + tile_bits));
      }
      if (lane == 0) sh_pre[1] = Gt;
#ifdef BIC_STAMPS
      if (lane == 0 && rid < (1u << 17)) g_known[1][rid] = Gt;
#endif
    }
  }

  // ---- EG as written (eg.cpp:20-37): per row ~R then '1'; a '0' after the plane's first 1 ----
  if (DO_E && valid) {
    const bool f_here = O == 0 && ones > 0;
    fcol = wave_min(fcol);
    const uint64_t Le = (uint64_t)g.cols + 1 + (f_here ? 1 : 0);
    const uint64_t Ge_rel = (uint64_t)row * (g.cols + 1) + (O > 0 ? 1 : 0);
    const uint64_t cap = a.slot_e * 64;
    const uint64_t Ge = (uint64_t)plane * cap + Ge_rel;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (Ge_rel + Le <= cap) {
      write_row(eimg, Le, Ge, f_here ? (int64_t)fcol + 1 : -1, a.out_e, a.efrag + 2 * id);
      if (lane == 0) { a.eboff[id] = Ge; a.elen[id] = Le; }
    } else if (lane == 0) {
      a.eboff[id] = Ge;
      a.elen[id] = 0;  // overflowed: nothing written, fixup skips
      atomicOr(&a.flags[0], 1u);
    }
    if (lane == 0 && row == g.rows - 1) a.bits_e[plane] = Ge_rel + Le;
  }

  STAMP(3);
  // ---- Golomb codewords into the row image (rows longer than the LDS window: row_global_at below) ----
  if constexpr (DO_G) {
    constexpr uint32_t kCapBits = (kGImg - kPad) * 32;
    const bool fits = L <= kCapBits;
#ifdef BIC_STAMPS
    uint32_t dbg_slow = 0;
#endif
    if (valid && fits) {
      StepState st{(uint32_t)(O + row), -1};
      const uint32_t arow = row * (g.cols + 1);
      uint64_t loc = 0;
      for (uint32_t w0 = 0; w0 < g.used; w0 += 64) {
        const uint32_t w = w0 + lane;
        const uint64_t x = img_resid(eimg, g, w);
        uint32_t n;
        int jp;
        step_prefix(x, w, st, n, jp);
        const bool eol = w == g.used - 1;
        const LaneEnc e = encode_word(x, w, n, jp, arow, eol, g.cols, ByteTables{s_lut, a.lut});
#ifdef BIC_STAMPS
        dbg_slow += (e.path == 3 ? 1u : 0u) + (e.lng ? 1000u : 0u) + (e.path == 1 ? 1000000u : 0u);
#endif
        const uint32_t inc = wave_incl_sum_u32(e.len);
        const uint64_t off = loc + inc - e.len;
        loc += lane63_u32(inc);
        if (!e.lng) {
          place_small(gimg, (uint32_t)off, e.head, e.k0);
          place128(gimg, (uint32_t)(off + e.k0 + e.z), e.t0, e.t1, e.tlen);
        } else {
          LdsSink ls{gimg, 0, 0};
          emit_word(ls, (uint32_t)off, x, w, n, jp, arow, eol, g.cols);
          ls.flush();
        }
      }
      if (lane == 0 && loc != L) atomicOr(&a.flags[3], 1u);  // word_len disagrees with the emission
    }
    STAMP(4);
#ifdef BIC_STAMPS
    {
      const uint32_t tot = wave_sum_u32(dbg_slow);
      if (lane == 0 && (uint64_t)id * 8 + 7 < (1u << 21)) g_stamps[(uint64_t)id * 8 + 7] = tot;
    }
#endif
    __syncthreads();
    STAMP(5);
    if (valid) {
      uint64_t Grel = sh_pre[1];
      for (int q = 0; q < wave; ++q) Grel += sh_len[q];
      const uint64_t cap = a.slot_g * 64;
      const uint64_t G = (uint64_t)plane * cap + Grel;
      if (lane == 0 && row == g.rows - 1) a.bits_g[plane] = Grel + L;
      if (Grel + L <= cap) {
        if (fits) {
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          __builtin_amdgcn_wave_barrier();
          write_row(gimg, L, G, -1, a.out_g, a.gfrag + 2 * id);
        }
        if (lane == 0) {
          a.gboff[id] = G;
          a.glen[id] = L;
          a.gslow[id] = 0;
        }
        // a row longer than the LDS window: written here, straight to global memory (no list, no
        // k_rows_global launch)
        if (!fits) row_global_at<PREDICT>(a, id, plane, row, G, L, O + row + 1, lane);
      } else if (lane == 0) {
        a.gboff[id] = G;
        a.glen[id] = 0;
        a.gslow[id] = 0;
        atomicOr(&a.flags[0], 1u);
      }
    }
    STAMP(6);
  }
}

// ==========================================================================================
// Two-pass encoder. Pass 1 (k_len_rows) runs the look-back chains with nothing but lengths:
// per 8-row tile the ones count, the ones prefix, each row's Golomb length (byte tables, no
// codeword strings) and the bits prefix; it stores, per row, the ones before it and both
// streams' bit offsets. Pass 2 (k_emit_rows) then writes every row independently -- no
// look-back, no workgroup barrier -- streaming each row's codewords through a small LDS window
// whose complete words go straight to HBM. A row's first and last word (shared with the
// neighbouring rows) go to the fragment table, as in the single-pass kernel.
// ==========================================================================================
constexpr int kWin = 1024;                      // u32 words of one wave's output window (also holds
                                                // the EG image of a plane's first-1 row)
constexpr uint32_t kIterCap = (kWin - 8) * 32 - 128;  // bits one 64-word step may emit

template <int WPL, bool PREDICT, bool DO_G, bool DO_E>
__global__ __launch_bounds__(64 * kTileRows, 8) void k_len_rows(FusedArgs a) {
  // (sh_len apart from sh_cnt: a wave that finishes its length early must not overwrite the 1-counts
  // a slower wave is still summing for its O -- one array for both raced: a wrong O, a wrong length,
  // about 1 in 15 two-pass calls, tools/dbg_twopass.py)
  __shared__ uint64_t sh_cnt[kTileRows], sh_len[kTileRows], sh_pre[2];
  __shared__ uint32_t sh_tile;
  __shared__ uint32_t s_lut[512];
  const Geom& g = a.g;
  const int lane = lane_id(), wave = (int)wave_id();
  const uint32_t tpp = (g.rows + kTileRows - 1) / kTileRows;
  if (threadIdx.x == 0) sh_tile = atomicAdd(a.counter, 1u);
  if (DO_G && threadIdx.x < 512) s_lut[threadIdx.x] = reinterpret_cast<const uint32_t*>(a.lut + 256)[threadIdx.x];
  __syncthreads();
  const uint64_t tile = sh_tile;
  if (tile >= (uint64_t)tpp * g.nplanes) return;  // uniform over the workgroup
  const uint32_t plane = (uint32_t)(tile % g.nplanes), trow = (uint32_t)(tile / g.nplanes);
  const uint64_t rbase = (uint64_t)plane * tpp, rid = rbase + trow;
  const uint32_t row = trow * kTileRows + wave;
  const bool valid = row < g.rows;
  const uint64_t id = (uint64_t)plane * g.rows + row;

  uint64_t rr[WPL];
  uint32_t ones = 0;
  if (valid) {
    resid_row<WPL, PREDICT>(a.planes, g, plane, row, rr);
#pragma unroll
    for (int t = 0; t < WPL; ++t) ones += (uint32_t)__popcll(rr[t]);
    ones = wave_sum_u32(ones);
  }
  if (lane == 0) sh_cnt[wave] = ones;
  __syncthreads();
  if (wave == 0) {
    uint64_t tile_ones = 0;
    for (int q = 0; q < kTileRows; ++q) tile_ones += sh_cnt[q];
    uint64_t O = 0;
    if (trow == 0) {
      if (lane == 0) rec_store(&a.ones_rec[rid], kInc | tile_ones);
    } else {
      if (lane == 0) rec_store(&a.ones_rec[rid], kAgg | tile_ones);
      O = lookback(a.ones_rec, rbase, rid, a.flags);
      if (lane == 0) rec_store(&a.ones_rec[rid], kInc | (O + tile_ones));
    }
    if (lane == 0) sh_pre[0] = O;
  }
  __syncthreads();
  uint64_t O = sh_pre[0];
  for (int q = 0; q < wave; ++q) O += sh_cnt[q];

  if (DO_E && valid && lane == 0) {  // EG as written: ~R then '1' per row; a '0' after the plane's first 1
    const uint64_t Le = (uint64_t)g.cols + 1 + ((O == 0 && ones > 0) ? 1 : 0);
    const uint64_t Ge_rel = (uint64_t)row * (g.cols + 1) + (O > 0 ? 1 : 0);
    const uint64_t cap = a.slot_e * 64;
    a.eboff[id] = (uint64_t)plane * cap + Ge_rel;
    if (Ge_rel + Le <= cap) {
      a.elen[id] = Le;
    } else {
      a.elen[id] = 0;
      atomicOr(&a.flags[0], 1u);
    }
    if (row == g.rows - 1) a.bits_e[plane] = Ge_rel + Le;
  }
  if (valid && lane == 0) a.row_o[id] = (uint32_t)O;

  if constexpr (DO_G) {
    uint64_t L = 0;
    uint32_t step_max = 0;
    if (valid) {
      StepState st{(uint32_t)(O + row), -1};
      const uint32_t arow = row * (g.cols + 1);
#pragma unroll
      for (int t = 0; t < WPL; ++t) {
        const uint32_t w = t * 64 + lane;
        if (t * 64 >= (int)g.used) break;
        uint32_t n;
        int jp;
        step_prefix(rr[t], w, st, n, jp);
        uint32_t kor = 0;
        const uint32_t tot = wave_sum_u32(word_len(rr[t], w, n, jp, arow, w == g.used - 1, g.cols, kor));
        L += tot;
        step_max = max(step_max, tot);
      }
    }
    if (lane == 0) sh_len[wave] = L;
    __syncthreads();
    if (wave == 0) {
      uint64_t tile_bits = 0;
      for (int q = 0; q < kTileRows; ++q) tile_bits += sh_len[q];
      uint64_t Gt = 0;
      if (trow == 0) {
        if (lane == 0) rec_store(&a.bits_rec[rid], kInc | tile_bits);
      } else {
        if (lane == 0) rec_store(&a.bits_rec[rid], kAgg | tile_bits);
        Gt = lookback(a.bits_rec, rbase, rid, a.flags);
        if (lane == 0) rec_store(&a.bits_rec[rid], kInc | (Gt + tile_bits));
      }
      if (lane == 0) sh_pre[1] = Gt;
    }
    __syncthreads();
    if (valid && lane == 0) {
      uint64_t Grel = sh_pre[1];
      for (int q = 0; q < wave; ++q) Grel += sh_len[q];
      const uint64_t cap = a.slot_g * 64;
      a.gboff[id] = (uint64_t)plane * cap + Grel;
      if (row == g.rows - 1) a.bits_g[plane] = Grel + L;
      if (Grel + L <= cap) {
        a.glen[id] = L;
        a.gslow[id] = step_max > kIterCap ? O + row + 1 : 0;  // k_rows_global writes such rows
        if (step_max > kIterCap) a.slow_ids[atomicAdd(a.slow_n, 1u)] = id;
      } else {
        a.glen[id] = 0;
        a.gslow[id] = 0;
        atomicOr(&a.flags[0], 1u);
      }
    }
  }
}

template <int WPL, bool PREDICT, bool DO_G, bool DO_E>
__global__ __launch_bounds__(64 * kTileRows, 8) void k_emit_rows(FusedArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kTileRows * kWin];
  __shared__ uint32_t s_lut[512];
  const Geom& g = a.g;
  const int lane = lane_id(), wave = (int)wave_id();
  uint32_t* win = lds + wave * kWin;
  if (DO_G && threadIdx.x < 512) s_lut[threadIdx.x] = reinterpret_cast<const uint32_t*>(a.lut + 256)[threadIdx.x];
  __syncthreads();  // the only workgroup barrier
  const uint64_t id = (uint64_t)blockIdx.x * kTileRows + wave;
  if (id >= (uint64_t)g.rows * g.nplanes) return;
  const uint32_t plane = (uint32_t)(id / g.rows), row = (uint32_t)(id % g.rows);
  const bool do_g = DO_G && a.glen[id] != 0 && a.gslow[id] == 0;
  const bool do_e = DO_E && a.elen[id] != 0;
  if (!do_g && !do_e) return;
  if (do_g) lds_image_zero32(win, kWin / 4);
  uint64_t rr[WPL];
  resid_row<WPL, PREDICT>(a.planes, g, plane, row, rr);
  const uint32_t O = a.row_o[id];

  if (do_e) {
    const uint64_t Ge = a.eboff[id], Le = a.elen[id];
    if (Le == (uint64_t)g.cols + 1) {
      eg_row_regs<WPL>(rr, g, Ge, Le, a.out_e, a.efrag + 2 * id);
    } else {
      // the plane's first 1 is in this row: EG image with the inserted '0' (once per plane)
      uint32_t* eimg = win;  // reused before the Golomb window is live
      int fcol = INT_MAX;
#pragma unroll
      for (int t = 0; t < WPL; ++t) {
        const uint32_t w = t * 64 + lane;
        if (rr[t] && fcol == INT_MAX) fcol = (int)(w * 64 + __builtin_clzll(rr[t]));
        if (w < g.used) {
          const uint64_t v = ~rr[t] & (w == g.used - 1 ? g.trail : ~0ull);
          eimg[2 * w] = (uint32_t)(v >> 32);
          eimg[2 * w + 1] = (uint32_t)v;
        }
      }
      if (lane < kPad + 1) eimg[2 * g.used + lane] = 0;
      fcol = wave_min(fcol);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      if (lane == 0) eimg[g.cols >> 5] |= 0x80000000u >> (g.cols & 31);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      write_row(eimg, Le, Ge, (int64_t)fcol + 1, a.out_e, a.efrag + 2 * id);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      if (do_g) {
        lds_image_zero32(win, kWin / 4);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
      }
    }
  }

  if constexpr (DO_G) {
    if (!do_g) return;
    const uint64_t G = a.gboff[id], L = a.glen[id];
    uint64_t* out = a.out_g;
    uint64_t* frag = a.gfrag + 2 * id;
    uint64_t wbase = G & ~63ull;  // absolute bit of win[0]
    const uint64_t first_word = G >> 6;
    StepState st{O + row, -1};
    const uint32_t arow = row * (g.cols + 1);
    uint64_t loc = 0;  // row bits placed so far
#pragma unroll
    for (int t = 0; t < WPL; ++t) {
      const uint32_t w = t * 64 + lane;
      if (t * 64 >= (int)g.used) break;
      const uint64_t x = rr[t];
      uint32_t n;
      int jp;
      step_prefix(x, w, st, n, jp);
      const bool eol = w == g.used - 1;
      const LaneEnc e = encode_word<true>(x, w, n, jp, arow, eol, g.cols, ByteTables{s_lut, a.lut});
      const uint32_t inc = wave_incl_sum_u32(e.len);
      const uint32_t p = (uint32_t)(G + loc - wbase) + inc - e.len;  // window bit of this lane's string
      if (!e.lng) {
        place_small(win, p, e.head, e.k0);
        place128(win, p + e.k0 + e.z, e.t0, e.t1, e.tlen);
      } else {
        LdsSink ls{win, 0, 0};
        emit_word(ls, p, x, w, n, jp, arow, eol, g.cols);
        ls.flush();
      }
      loc += lane63_u32(inc);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      // flush the complete 64-bit words; the row's first word, if shared, is a fragment
      const uint32_t nfull = (uint32_t)((G + loc - wbase) >> 6);
      for (uint32_t q = lane; q < nfull; q += 64) {
        const uint64_t v = ((uint64_t)win[2 * q] << 32) | win[2 * q + 1];
        const uint64_t wi = (wbase >> 6) + q;
        if (wi == first_word && (G & 63)) frag[0] = v;
        else out[wi] = bswap64(v);
      }
      if (nfull) {  // carry the partial word to the front, clear the rest
        const uint32_t c0 = win[2 * nfull], c1 = win[2 * nfull + 1];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (uint32_t q = 2 + lane; q < 2 * nfull + 2; q += 64) win[q] = 0;
        if (lane == 0) { win[0] = c0; win[1] = c1; }
        wbase += 64ull * nfull;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
      }
    }
    // the row's last word, if it ends inside one
    if ((G + L) & 63) {
      if (lane == 0) {
        const uint64_t v = ((uint64_t)win[0] << 32) | win[1];
        if ((wbase >> 6) == first_word) frag[0] = v;
        else frag[1] = v;
      }
    }
  }
}

// (the staged encoder's count pass zeroes its counters itself: kZeroWords)
void launch_lookback_clear(hipStream_t s, const FusedCall& c) {
  if (!c.rq.zero_ready) launch_fill(s, c.ar.counter, 0, c.ar.zero_bytes);
}

void launch_lookback_rows(hipStream_t s, const FusedCall& c) {
  const FusedArgs a = make_fused_args(c);
  const Geom& g = c.g;
  const uint64_t nrows = (uint64_t)g.rows * g.nplanes;
  const uint32_t grid = (uint32_t)((g.rows + kTileRows - 1) / kTileRows * (uint64_t)g.nplanes);  // one per tile
  const uint32_t egrid = (uint32_t)((nrows + kTileRows - 1) / kTileRows);                       // one per 16 rows
  const dim3 blk(64 * kTileRows);
  with_row_kernel(g, c.predict != 0, a.out_g != nullptr, a.out_e != nullptr, [&](auto w, auto p, auto dg, auto de) {
    if (c.mode == kEncSingle) {
      k_encode_rows<w(), p(), dg(), de()><<<grid, blk, 0, s>>>(a);
    } else {
      k_len_rows<w(), p(), dg(), de()><<<grid, blk, 0, s>>>(a);
      k_emit_rows<w(), p(), dg(), de()><<<egrid, blk, 0, s>>>(a);
    }
  });
}

}  // namespace bic
