// bic_bsvd.hip -- the steps of the reference's binary dictionary learning on the device
// (include/bic.h "binary dictionary learning"):
//
//  * bsvd.cpp:399-460 update_coefficients_basic (= :1029-1107 _omp, rows are independent): greedy
//    sparse coding, per row of E the atom (row of D) at least Hamming distance, first in k among
//    equals (:423-437, strict <), XORed in while it lowers the row's weight (:439-447);
//  * bsvd.cpp:463-527 update_dictionary_steepest: atom by atom, in order, the per-column majority over
//    the rows that use the atom (:486-506), the change carried into those rows of E (:512-520);
//  * bsvd.cpp:530-735 update_dictionary_proximus (= :822-1027 _omp, the same text): per atom, rounds of that
//    vote for the one atom and a vote of every row's coefficient against the atom, until a round changes nothing;
//  * bsvd.cpp:1220 add(E, X, E) after mul(A, D, E): the word-wise XOR;
//  * bsvd.cpp:99-267 initialize_model_neighbor / _partition / _random_centroids / _random_centroids_xor: D and A
//    from the data, every atom a vote over its member rows (these mask E's last word: see there).
//
// Matrices are in the plane layout (bic.h): row-major u64 words, column j at bit 63 - j % 64 of word
// j / 64. Distances, weights and XORs run over the mw = ceil(m / 64) whole words of a row, as dist,
// weight and add do (binmat.cpp:57-67, 463-512); words past mw (the pitch) are never touched.
#include "bic_bsvd_dev.h"

#include <algorithm>

namespace bic {

// ------------------------------------------------------------------------------------------------
// Sparse coding. One row per wave: lane w < mw holds word w of E_i, lane w < ceil(p / 64) word w of
// A_i, and a copy of E_i sits in LDS where every lane reads it (same address: a broadcast). The atoms
// are in LDS word-major (word w of atom k at tile[w * ta + k]), so the 64 lanes of a wave, one atom
// each, read 64 consecutive words. A lane runs kBsvdJ atoms per E word it reads. The least key
// (dist << 12) | k over the wave is the least distance and, among equals, the least k.
//
// D is resident (loaded once per workgroup, waves then run their rows without meeting) while
// roundup64(p) * mw words fit in kBsvdTileWords; otherwise every round streams it through LDS in
// tiles of ta atoms, the four rows of a workgroup in step, the running minimum carried across tiles.
// ------------------------------------------------------------------------------------------------
constexpr uint32_t kBsvdTileWords = 7680;  // 60 KiB of atoms + 2 KiB of rows: two workgroups per CU
constexpr int kBsvdJ = 4;

__device__ __forceinline__ int bsvd_scan(const uint64_t* erow, const uint64_t* tile, uint32_t ta, uint32_t cnt,
                                         uint32_t k0, uint32_t mw, int best) {
  const uint32_t lane = lane_id();
  for (uint32_t base = 0; base < cnt; base += 64 * kBsvdJ) {
    uint32_t d[kBsvdJ];
#pragma unroll
    for (int j = 0; j < kBsvdJ; ++j) d[j] = 0;
    for (uint32_t w = 0; w < mw; ++w) {
      const uint64_t e = erow[w];
      const uint64_t* col = tile + w * ta + base + lane;
#pragma unroll
      for (int j = 0; j < kBsvdJ; ++j)  // (wave-uniform guard; ta is a multiple of 64, so base + 64 j + lane < ta)
        if (base + 64 * j < cnt) d[j] += (uint32_t)__popcll(e ^ col[64 * j]);
    }
#pragma unroll
    for (int j = 0; j < kBsvdJ; ++j) {
      const uint32_t k = base + 64 * j + lane;
      if (k < cnt) best = min(best, (int)((d[j] << 12) | (k0 + k)));
    }
  }
  return best;
}

__device__ __forceinline__ void bsvd_load_tile(uint64_t* tile, uint32_t ta, const uint64_t* D, uint32_t d_wpr,
                                               uint32_t k0, uint32_t cnt, uint32_t mw) {
  for (uint32_t idx = threadIdx.x; idx < cnt * mw; idx += blockDim.x) {
    const uint32_t k = idx / mw, w = idx - k * mw;
    tile[w * ta + k] = D[(uint64_t)(k0 + k) * d_wpr + w];
  }
}

// the step of one row once the wave knows its best key: true if the atom was taken
__device__ __forceinline__ bool bsvd_take(int best, uint64_t& ew, uint64_t& aw, uint64_t* erow, const uint64_t* D,
                                          uint32_t d_wpr, uint32_t mw) {
  const uint32_t lane = lane_id();
  const uint32_t wgt = wave_total_u32((uint32_t)__popcll(ew));  // (lanes >= mw hold 0)
  const uint32_t bestd = (uint32_t)best >> 12, bestk = (uint32_t)best & 4095u;
  if (bestd >= wgt) return false;  // bsvd.cpp:439: only a strictly lower weight is a step
  if (lane < mw) {
    ew ^= D[(uint64_t)bestk * d_wpr + lane];
    erow[lane] = ew;
  }
  if (lane == (bestk >> 6)) aw ^= BIC_MSB >> (bestk & 63u);  // Ai.flip(0, bestk): may switch an atom off
  __builtin_amdgcn_wave_barrier();
  return true;
}

template <bool RESIDENT>
__global__ __launch_bounds__(256) void k_bsvd_coef(uint64_t* __restrict__ E, uint32_t n, uint32_t mw, uint32_t e_wpr,
                                                   const uint64_t* __restrict__ D, uint32_t p, uint32_t d_wpr,
                                                   uint64_t* __restrict__ A, uint32_t a_wpr, uint32_t ta,
                                                   unsigned long long* changed) {
  extern __shared__ __attribute__((aligned(16))) uint64_t bsvd_lds[];
  const uint32_t lane = lane_id(), wave = wave_id();
  uint64_t* erow = bsvd_lds + wave * 64;
  uint64_t* tile = bsvd_lds + 4 * 64;
  const uint32_t pw = (p + 63) / 64;
  const uint32_t max_steps = 64 * mw;  // every step lowers the row's weight, which is at most 64 mw
  uint32_t nchanged = 0;
  if constexpr (RESIDENT) {
    bsvd_load_tile(tile, ta, D, d_wpr, 0, p, mw);
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * 4 + wave; i < n; i += (uint64_t)gridDim.x * 4) {
      uint64_t ew = lane < mw ? E[i * e_wpr + lane] : 0ull;
      uint64_t aw = lane < pw ? A[i * a_wpr + lane] : 0ull;
      if (lane < mw) erow[lane] = ew;
      __builtin_amdgcn_wave_barrier();
      bool ch = false;
      for (uint32_t step = 0; step <= max_steps; ++step) {
        const int best = wave_min(bsvd_scan(erow, tile, ta, p, 0, mw, INT_MAX));
        if (!bsvd_take(best, ew, aw, erow, D, d_wpr, mw)) break;
        ch = true;
      }
      if (ch) {
        if (lane < mw) E[i * e_wpr + lane] = ew;
        if (lane < pw) A[i * a_wpr + lane] = aw;
        ++nchanged;
      }
    }
  } else {
    const uint32_t ngroups = (n + 3) / 4;
    for (uint32_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
      const uint64_t i = (uint64_t)g * 4 + wave;
      bool active = i < n;  // wave-uniform
      uint64_t ew = (active && lane < mw) ? E[i * e_wpr + lane] : 0ull;
      uint64_t aw = (active && lane < pw) ? A[i * a_wpr + lane] : 0ull;
      if (lane < mw) erow[lane] = ew;
      bool ch = false;
      for (uint32_t step = 0; step <= max_steps; ++step) {
        // (the barrier also separates the last tile's readers from the next round's first load)
        if (!__syncthreads_or(active ? 1 : 0)) break;
        int best = INT_MAX;
        for (uint32_t k0 = 0; k0 < p; k0 += ta) {
          const uint32_t cnt = min(ta, p - k0);
          if (k0) __syncthreads();
          bsvd_load_tile(tile, ta, D, d_wpr, k0, cnt, mw);
          __syncthreads();
          if (active) best = bsvd_scan(erow, tile, ta, cnt, k0, mw, best);
        }
        if (active) {
          best = wave_min(best);
          if (bsvd_take(best, ew, aw, erow, D, d_wpr, mw)) ch = true;
          else active = false;
        }
      }
      if (ch) {
        if (lane < mw) E[i * e_wpr + lane] = ew;
        if (lane < pw) A[i * a_wpr + lane] = aw;
        ++nchanged;
      }
      __syncthreads();  // the next group's rows overwrite erow
    }
  }
  if (lane == 0 && nchanged && changed) atomicAdd(changed, (unsigned long long)nchanged);
}

void launch_bsvd_coef(hipStream_t s, uint64_t* E, uint32_t n, uint32_t m, uint32_t e_wpr, const uint64_t* D,
                      uint32_t p, uint32_t d_wpr, uint64_t* A, uint32_t a_wpr, uint64_t* changed) {
  const uint32_t mw = (m + 63) / 64, p64 = (p + 63) / 64 * 64;
  const bool resident = (uint64_t)p64 * mw <= kBsvdTileWords;
  const uint32_t ta = resident ? p64 : kBsvdTileWords / mw / 64 * 64;  // mw <= 64: at least 64 atoms
  const size_t lds = (size_t)(4 * 64 + (size_t)ta * mw) * 8;
  const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)n + 3) / 4, 512);
  if (!grid) return;
  auto* ch = reinterpret_cast<unsigned long long*>(changed);
  if (resident)
    k_bsvd_coef<true><<<grid, 256, lds, s>>>(E, n, mw, e_wpr, D, p, d_wpr, A, a_wpr, ta, ch);
  else
    k_bsvd_coef<false><<<grid, 256, lds, s>>>(E, n, mw, e_wpr, D, p, d_wpr, A, a_wpr, ta, ch);
}

// ------------------------------------------------------------------------------------------------
// Dictionary update. At = the transpose of A: row k is the bit row of atom k's users. A workgroup
// owns wpb words of it, i.e. 64 wpb rows of E, for the whole update; the thread (slot, w) walks the
// users in the At words a0 + slot, a0 + slot + nslots, .. and touches word w of each. So a word of E
// is read and written by one thread only, whatever the atom, and one launch can do both
//
//   * atom k - 1's change: E_i ^= delta (D_k-1 ^ its new value) for its users, and
//   * atom k's column counts over E_i of its users, then in bit-sliced carry-save counters (five
//     planes: 31 rows between two flushes into the workgroup's LDS counts), LDS counts to the global
//     ones with atomicAdd.
//
// The workgroup that takes the last ticket of the launch turns the counts into the new atom: with
// U users and c' the count of E's bit, the count of (E ^ D_k)'s bit is c' where D_k's bit is 0 and
// U - c' where it is 1; the new bit is count > U / 2 (bsvd.cpp:502-506) for j < m, D_k's own bit
// past m. It stores delta, D_k and the flag "delta != 0", counts the atom in *changed and leaves the
// counts, U and the ticket zero for the next atom. Nothing waits on another workgroup: the launches
// k = k_lo .. k_hi are ordered on the stream (one atom each), or, when one workgroup owns every row,
// it walks all the atoms in one launch. k = p only applies atom p - 1's change.
// ------------------------------------------------------------------------------------------------
// PROX: the atom half of one PROXIMUS round (bsvd.cpp:628-671) for atom k_lo = k_hi, round pr of the budget:
// the same counts and the same vote, but the change is left to k_bsvd_prox_coef (which passes over every
// row anyway), the atom is counted in *changed once however many rounds change it, and the round is counted.
template <bool PROX>
__global__ __launch_bounds__(256) void k_bsvd_dict(uint64_t* __restrict__ E, uint32_t m, uint32_t mw, uint32_t lg,
                                                   uint32_t e_wpr, uint64_t* __restrict__ D, uint32_t p,
                                                   uint32_t d_wpr, const uint64_t* __restrict__ At, uint32_t atw,
                                                   uint32_t wpb, uint32_t k_lo, uint32_t k_hi, uint32_t* cnt,
                                                   uint64_t* delta, uint32_t* misc, unsigned long long* changed,
                                                   uint32_t pr, uint32_t pflags) {
  __shared__ uint32_t lcnt[64 * 64];
  __shared__ uint32_t s_users, s_last, s_u, s_any;
  const uint32_t t = threadIdx.x, lane = lane_id(), wave = wave_id();
  if constexpr (PROX) {
    if (prox_leaves<true>(misc, k_lo, pr, pflags) || k_lo >= p) return;  // (k_lo = p: the last atom's stall check)
  }
  const uint32_t w = t & ((1u << lg) - 1u), slot = t >> lg, nslots = 256u >> lg;
  const uint32_t a0 = blockIdx.x * wpb, a1 = min(a0 + wpb, atw);
  const bool mine = w < mw;
  for (uint32_t k = k_lo; k <= k_hi; ++k) {
    if (!PROX && k > 0 && ld_agent(&misc[2])) {  // atom k - 1 changed: carry it into its users' rows
      const uint64_t dl = mine ? ld_agent(&delta[w]) : 0ull;
      const uint64_t* at = At + (uint64_t)(k - 1) * atw;
      for (uint32_t a = a0 + slot; a < a1; a += nslots) {
        uint64_t bits = at[a];
        while (bits) {
          const uint32_t b = (uint32_t)__builtin_clzll(bits);
          bits &= ~(BIC_MSB >> b);
          if (mine) E[((uint64_t)a * 64 + b) * e_wpr + w] ^= dl;
        }
      }
    }
    if (k >= p) break;
    for (uint32_t j = t; j < mw * 64; j += 256) lcnt[j] = 0;
    if (t == 0) s_users = 0;
    __syncthreads();
    {
      const uint64_t* at = At + (uint64_t)k * atw;
      uint64_t pl[kBsvdPlanes];
#pragma unroll
      for (int q = 0; q < kBsvdPlanes; ++q) pl[q] = 0;
      uint32_t nacc = 0, users = 0;
      for (uint32_t a = a0 + slot; a < a1; a += nslots) {
        uint64_t bits = at[a];
        if (w == 0) users += (uint32_t)__popcll(bits);
        while (bits) {
          const uint32_t b = (uint32_t)__builtin_clzll(bits);
          bits &= ~(BIC_MSB >> b);
          if (mine) {
            uint64_t carry = E[((uint64_t)a * 64 + b) * e_wpr + w];
#pragma unroll
            for (int q = 0; q < kBsvdPlanes; ++q) {  // the vertical adder: plane q holds bit q of 64 counts
              const uint64_t c2 = pl[q] & carry;
              pl[q] ^= carry;
              carry = c2;
            }
            if (++nacc == kBsvdFlush) {
              bsvd_flush(pl, lcnt + w * 64);
              nacc = 0;
            }
          }
        }
      }
      if (mine && nacc) bsvd_flush(pl, lcnt + w * 64);
      if (users) atomicAdd(&s_users, users);
    }
    __syncthreads();
    for (uint32_t j = t; j < mw * 64; j += 256)
      if (lcnt[j]) atomicAdd(&cnt[j], lcnt[j]);
    if (t == 0 && s_users) atomicAdd(&misc[0], s_users);
    __threadfence();
    __syncthreads();
    if (t == 0) {
      s_last = atomicAdd(&misc[1], 1u) == gridDim.x - 1 ? 1u : 0u;
      s_any = 0;
    }
    __syncthreads();
    if (!s_last) return;  // (gridDim.x > 1: the launch holds one atom)
    __threadfence();
    if (t == 0) {
      s_u = atomicExch(&misc[0], 0u);
      atomicExch(&misc[1], 0u);
    }
    __syncthreads();
    const uint32_t U = s_u;
    bool any = false;
    for (uint32_t wi = wave; wi < mw; wi += 4) {  // wave-uniform: one word of the atom per wave
      const uint32_t j = wi * 64 + lane;
      const uint64_t dk = D[(uint64_t)k * d_wpr + wi];
      const uint32_t c0 = atomicExch(&cnt[j], 0u);
      const bool dbit = (dk >> (63 - lane)) & 1ull;
      const uint32_t c = dbit ? U - c0 : c0;
      const bool nb = (U && j < m) ? c > U / 2 : dbit;  // U = 0: the atom is skipped (bsvd.cpp:499)
      const uint64_t nw = __builtin_bitreverse64(__builtin_amdgcn_ballot_w64(nb));
      const uint64_t dl = dk ^ nw;
      if (lane == 0) {
        __hip_atomic_store(&delta[wi], dl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (dl) D[(uint64_t)k * d_wpr + wi] = nw;
      }
      any |= dl != 0;
    }
    if (any && lane == 0) atomicOr(&s_any, 1u);
    __syncthreads();
    if (t == 0) {
      __hip_atomic_store(&misc[2], s_any, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if constexpr (PROX) {
        st_agent(&misc[kProxAgain + (pr & 1u)], s_any);  // the coefficient half ORs its flips in
        atomicAdd(reinterpret_cast<unsigned long long*>(&misc[kProxRounds]), 1ull);
        const uint32_t before = (pflags & kProxFresh) ? 0u : ld_agent(&misc[kProxKch]);
        if (s_any && !before) atomicAdd(changed, 1ull);  // bsvd.cpp:659, 724: once per atom
        st_agent(&misc[kProxKch], before | s_any);
      } else {
        if (s_any) atomicAdd(changed, 1ull);
      }
    }
    __threadfence();
    __syncthreads();
  }
}

size_t bsvd_dict_scratch_bytes(uint32_t n, uint32_t p) {
  return kBsvdDictHead + (size_t)p * (((size_t)n + 63) / 64) * 8;
}

uint32_t bsvd_dict_blocks(uint32_t n) {
  const uint32_t atw = (n + 63) / 64;
  const uint32_t want = std::min<uint32_t>(256, (atw + 15) / 16);  // at least 16 words of At (1,024 rows) each
  const uint32_t wpb = (atw + want - 1) / want;
  return (atw + wpb - 1) / wpb;
}

namespace {
struct DictArena {
  uint32_t *misc, *cnt;
  uint64_t *delta, *At;
};
DictArena dict_arena(void* scratch) {
  uint8_t* base = static_cast<uint8_t*>(scratch);
  return {reinterpret_cast<uint32_t*>(base), reinterpret_cast<uint32_t*>(base + 64),
          reinterpret_cast<uint64_t*>(base + 64 + 64 * 64 * 4), reinterpret_cast<uint64_t*>(base + kBsvdDictHead)};
}
}  // namespace

void launch_bsvd_dict_prepare(hipStream_t s, uint32_t n, uint32_t p, const uint64_t* A, uint32_t a_wpr,
                              void* scratch) {
  const DictArena ar = dict_arena(scratch);
  const uint32_t pw = (p + 63) / 64, atw = (n + 63) / 64;
  launch_fill(s, ar.misc, 0, 64 + (size_t)64 * 64 * 4);  // U, the ticket, the flag; the column counts
  // the transpose's grid holds four 64-row blocks per unit of gridDim.y (at most 65,535): in chunks of rows
  for (uint32_t r0 = 0; r0 < n; r0 += kGf2MaxRows) {
    const uint32_t rows = std::min(n - r0, kGf2MaxRows);
    launch_gf2_transpose(s, A + (uint64_t)r0 * a_wpr, rows, a_wpr, pw, p, ar.At + r0 / 64, atw, (rows + 63) / 64);
  }
}

void launch_bsvd_dict_atoms(hipStream_t s, uint64_t* E, uint32_t n, uint32_t m, uint32_t e_wpr, uint64_t* D,
                            uint32_t p, uint32_t d_wpr, void* scratch, uint32_t k_lo, uint32_t k_hi,
                            uint64_t* changed) {
  const DictArena ar = dict_arena(scratch);
  const uint32_t mw = (m + 63) / 64, atw = (n + 63) / 64;
  uint32_t lg = 0;
  while ((1u << lg) < mw) ++lg;
  const uint32_t grid = bsvd_dict_blocks(n), wpb = (atw + grid - 1) / grid;
  k_bsvd_dict<false><<<grid, 256, 0, s>>>(E, m, mw, lg, e_wpr, D, p, d_wpr, ar.At, atw, wpb, k_lo, k_hi, ar.cnt,
                                          ar.delta, ar.misc, reinterpret_cast<unsigned long long*>(changed), 0u, 0u);
}

// ------------------------------------------------------------------------------------------------
// PROXIMUS (bsvd.cpp:530-735). Per atom, rounds of two launches: k_bsvd_dict<true>, the atom half, and
// k_bsvd_prox_coef, the coefficient half (:676-719) over ALL rows, one row per lane:
//
//   1. a user takes the atom half's pending change, E_i ^= delta (whole words; delta is 0 past m);
//   2. c = |E_i & D_k| over j < m (D_k's last word masked); |S| = |D_k| over j < m;
//   3. Aw = c for a non-user, |S| - c for a user; the new A(i,k) is Aw > |S| / 2 (|S| = 0: no vote);
//   4. where it differs, A(i,k) flips and E_i ^= D_k for j < m;
//   5. the wave's ballot of the new bits is its word of row k of At, which the next atom half reads:
//      A and At agree after every launch.
//
// `again` (by round parity) is the atom half's "delta != 0" ORed with "some coefficient flipped": the next
// round runs if it is set, the launches of the rounds after a round that moved nothing leave at once
// (prox_leaves). No workgroup waits for another; the order is the stream's.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bsvd_prox_coef(uint64_t* __restrict__ E, uint32_t n, uint32_t m, uint32_t mw,
                                                        uint32_t e_wpr, const uint64_t* __restrict__ D,
                                                        uint32_t d_wpr, uint64_t* __restrict__ A, uint32_t a_wpr,
                                                        uint64_t* __restrict__ At, uint32_t atw, uint32_t k,
                                                        uint32_t pr, uint32_t* misc, const uint64_t* delta) {
  __shared__ uint64_t s_dm[64], s_dl[64];
  if (prox_leaves<false>(misc, k, pr, 0u)) return;
  const uint32_t t = threadIdx.x, lane = lane_id(), wave = wave_id();
  const bool pend = ld_agent(&misc[2]) != 0;
  if (t < mw) {
    uint64_t dk = D[(uint64_t)k * d_wpr + t];
    if (t == mw - 1 && (m & 63u)) dk &= ~0ull << (64 - (m & 63u));  // j < m only (bsvd.cpp:681)
    s_dm[t] = dk;
    s_dl[t] = pend ? ld_agent(&delta[t]) : 0ull;
  }
  __syncthreads();
  uint32_t S = 0;
  for (uint32_t w = 0; w < mw; ++w) S += (uint32_t)__popcll(s_dm[w]);
  uint64_t* atk = At + (uint64_t)k * atw;
  for (uint32_t wv = blockIdx.x * 4 + wave; wv < atw; wv += gridDim.x * 4) {  // wave-uniform
    const uint64_t aw = atk[wv];
    if (!S && !(pend && aw)) continue;  // no vote (:694) and no user with a change to take
    const uint64_t i = (uint64_t)wv * 64 + lane;
    const bool live = i < n;
    const bool a = (aw >> (63 - lane)) & 1ull;  // (At's bits past n are 0)
    uint64_t* row = E + i * e_wpr;
    uint32_t c = 0;
    if (live)
      for (uint32_t w = 0; w < mw; ++w) c += (uint32_t)__popcll((row[w] ^ (a ? s_dl[w] : 0ull)) & s_dm[w]);
    const bool nb = S ? (live && (a ? S - c : c) > S / 2) : a;
    const bool flip = nb != a;
    if (live && ((a && pend) || flip))
      for (uint32_t w = 0; w < mw; ++w) {
        const uint64_t x = (a ? s_dl[w] : 0ull) ^ (flip ? s_dm[w] : 0ull);
        if (x) row[w] ^= x;
      }
    if (flip) A[i * a_wpr + (k >> 6)] ^= BIC_MSB >> (k & 63u);
    const uint64_t nw = __builtin_bitreverse64(__builtin_amdgcn_ballot_w64(nb));
    if (nw != aw && lane == 0) {
      atk[wv] = nw;
      atomicOr(&misc[kProxAgain + (pr & 1u)], 1u);
    }
  }
}

// (launch_bsvd_dict_prepare's fill covers the schedule's words)
void launch_bsvd_prox_clear_stall(hipStream_t s, void* scratch) {
  launch_fill(s, dict_arena(scratch).misc + kProxStalled, 0, 4);
}

void launch_bsvd_prox_atom(hipStream_t s, uint64_t* E, uint32_t n, uint32_t m, uint32_t e_wpr, uint64_t* D,
                           uint32_t p, uint32_t d_wpr, void* scratch, uint32_t k, uint32_t r, uint32_t budget,
                           bool check_prev, bool fresh) {
  const DictArena ar = dict_arena(scratch);
  const uint32_t mw = (m + 63) / 64, atw = (n + 63) / 64;
  uint32_t lg = 0;
  while ((1u << lg) < mw) ++lg;
  const uint32_t blocks = bsvd_dict_blocks(n), wpb = (atw + blocks - 1) / blocks;
  // (the previous atom's last budgeted round is round budget - 1: that is the parity of its `again`)
  const uint32_t pflags = (check_prev ? kProxCheckPrev : 0u) | (fresh ? kProxFresh : 0u) |
                          (((budget - 1) & 1u) ? kProxPrevParity : 0u);
  k_bsvd_dict<true><<<k < p ? blocks : 1u, 256, 0, s>>>(
      E, m, mw, lg, e_wpr, D, p, d_wpr, ar.At, atw, wpb, k, k, ar.cnt, ar.delta, ar.misc,
      reinterpret_cast<unsigned long long*>(ar.misc + kProxChanged), r, pflags);
}

void launch_bsvd_prox_coef(hipStream_t s, uint64_t* E, uint32_t n, uint32_t m, uint32_t e_wpr, const uint64_t* D,
                           uint32_t d_wpr, uint64_t* A, uint32_t a_wpr, void* scratch, uint32_t k, uint32_t r) {
  const DictArena ar = dict_arena(scratch);
  const uint32_t mw = (m + 63) / 64, atw = (n + 63) / 64;
  const uint32_t grid = std::min<uint32_t>((atw + 3) / 4, 2048);
  k_bsvd_prox_coef<<<grid, 256, 0, s>>>(E, n, m, mw, e_wpr, D, d_wpr, A, a_wpr, ar.At, atw, k, r, ar.misc, ar.delta);
}

// E ^= X over the first mw words of every row (add(E, X, E), binmat.cpp:463-480)
__global__ __launch_bounds__(256) void k_bsvd_xor(uint64_t* __restrict__ E, uint32_t e_wpr,
                                                  const uint64_t* __restrict__ X, uint32_t x_wpr, uint64_t total,
                                                  uint32_t mw) {
  for (uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (uint64_t)gridDim.x * 256) {
    const uint64_t i = idx / mw;
    const uint32_t w = (uint32_t)(idx - i * mw);
    E[i * e_wpr + w] ^= X[i * x_wpr + w];
  }
}

void launch_bsvd_xor(hipStream_t s, uint64_t* E, uint32_t n, uint32_t m, uint32_t e_wpr, const uint64_t* X,
                     uint32_t x_wpr) {
  const uint32_t mw = (m + 63) / 64;
  const uint64_t total = (uint64_t)n * mw;
  const uint32_t grid = (uint32_t)std::min<uint64_t>((total + 255) / 256, 4096);
  if (grid) k_bsvd_xor<<<grid, 256, 0, s>>>(E, e_wpr, X, x_wpr, total, mw);
}

// ------------------------------------------------------------------------------------------------
// Model initialisers (bsvd.cpp:99-267; bic.h "model initialisers"). Every atom is a vote over a set of
// member rows of E, and the atoms are independent: workgroup (k, s) takes atom k and the s-th share of
// the rows. As in k_bsvd_dict the thread (slot, w) holds word w of the row its slot is at, the rows go
// kInitAhead at a time so that their loads are in flight together, a member row is added to the
// bit-sliced carry-save planes (flushed into the workgroup's LDS counts every 31 rows), and the LDS
// counts go to the atom's global ones with atomicAdd. Who is a member:
//
//   kInitNeighbor   the rows that meet the pick row sel[k] (E_j & E_pick != 0 over j < m), each added
//                   masked with the pick; the threads of a row learn "some word met" from the wave's ballot;
//   kInitPartition  the rows with the pivot column sel[k] set (k < nsel; the other atoms are stored zero);
//   kInitCentroids  the rows with sel[j] = k; kInitXor the same, with one XOR word in place of counts;
//   kInitColw       every row below n (the host passes the sampled row count): the column weights that
//                   col_weight (binmat.cpp:80-92) sees, left in the counts for k_bsvd_init_rank.
//
// E's last word is masked (get_block, binmat.h:188-190). The workgroup that takes the atom's last ticket
// reads the counts and u back (atomicExch: they are zero again afterwards), forms the atom by the mode's
// rule and stores its first mw words. No workgroup waits for another.
// ------------------------------------------------------------------------------------------------
constexpr int kInitNeighbor = 0, kInitPartition = 1, kInitCentroids = 2, kInitXor = 3, kInitColw = 4;
constexpr uint32_t kInitAhead = 4;

template <int MODE>
__global__ __launch_bounds__(256) void k_bsvd_init(const uint64_t* __restrict__ E, uint32_t n, uint32_t m, uint32_t mw,
                                                   uint32_t lg, uint32_t e_wpr, uint64_t* __restrict__ D,
                                                   uint32_t d_wpr, const uint32_t* __restrict__ sel, uint32_t nsel,
                                                   uint32_t chunk, uint32_t* cnt, uint32_t* ucnt, uint32_t* tick) {
  __shared__ uint32_t lcnt[64 * 64];
  __shared__ uint64_t s_pick[64];  // kInitNeighbor: the pick row, masked; kInitXor: the workgroup's XOR
  __shared__ uint32_t s_users, s_last, s_u;
  const uint32_t t = threadIdx.x, lane = lane_id(), wave = wave_id();
  const uint32_t k = blockIdx.x;
  const uint32_t w = t & ((1u << lg) - 1u), slot = t >> lg, nslots = 256u >> lg;
  const bool mine = w < mw;
  const uint64_t wmask = (w == mw - 1 && (m & 63u)) ? ~0ull << (64 - (m & 63u)) : ~0ull;
  // what a member is tested against: the atom itself, or the pick row / pivot column the atom was given
  uint32_t key = k;
  if constexpr (MODE == kInitNeighbor || MODE == kInitPartition) key = k < nsel ? sel[k] : ~0u;
  if constexpr (MODE == kInitPartition) {
    if (k >= nsel) {  // "the other atoms are left uninitialized" (:216): they keep D.clear()'s zero
      if (blockIdx.y == 0 && t < mw) D[(uint64_t)k * d_wpr + t] = 0ull;
      return;
    }
  }
  for (uint32_t j = t; j < mw * 64; j += 256) lcnt[j] = 0;
  if (t < 64) s_pick[t] = 0ull;
  if (t == 0) s_users = 0;
  __syncthreads();
  if constexpr (MODE == kInitNeighbor) {  // (a pick >= n is skipped: no row meets a zero pick, the atom stays zero)
    if (key < n && slot == 0 && mine) s_pick[w] = E[(uint64_t)key * e_wpr + w] & wmask;
    __syncthreads();
  }
  const uint64_t pick = (MODE == kInitNeighbor && mine) ? s_pick[w] : 0ull;
  const uint32_t gsh = lane & ~((1u << lg) - 1u);  // the first lane of this row's threads
  const uint64_t gmask = lg == 6 ? ~0ull : ((1ull << (1u << lg)) - 1ull);
  const uint64_t r0 = (uint64_t)blockIdx.y * chunk, r1 = r0 + chunk < n ? r0 + chunk : (uint64_t)n;
  uint64_t pl[kBsvdPlanes];
#pragma unroll
  for (int q = 0; q < kBsvdPlanes; ++q) pl[q] = 0;
  uint64_t xr = 0;
  uint32_t nacc = 0, users = 0;
  for (uint64_t base = r0; base < r1; base += (uint64_t)nslots * kInitAhead) {  // (uniform over the workgroup)
    uint64_t x[kInitAhead];
    bool mem[kInitAhead];
#pragma unroll
    for (uint32_t a = 0; a < kInitAhead; ++a) {
      const uint64_t j = base + (uint64_t)a * nslots + slot;
      const bool live = j < r1;
      x[a] = (live && mine) ? E[j * e_wpr + w] & wmask : 0ull;
      if constexpr (MODE == kInitNeighbor) x[a] &= pick;
      if constexpr (MODE == kInitPartition)
        mem[a] = live && ((E[j * e_wpr + (key >> 6)] >> (63u - (key & 63u))) & 1ull);
      if constexpr (MODE == kInitCentroids || MODE == kInitXor) mem[a] = live && sel[j] == key;
      if constexpr (MODE == kInitColw) mem[a] = live;
    }
    if constexpr (MODE == kInitNeighbor) {  // (every lane of the wave is here: the ballots come before any branch)
#pragma unroll
      for (uint32_t a = 0; a < kInitAhead; ++a)
        mem[a] = ((__builtin_amdgcn_ballot_w64(x[a] != 0ull) >> gsh) & gmask) != 0ull;
    }
#pragma unroll
    for (uint32_t a = 0; a < kInitAhead; ++a) {
      if (!mem[a]) continue;
      if (w == 0) ++users;
      if (!mine) continue;
      if constexpr (MODE == kInitXor) {
        xr ^= x[a];
      } else {
        uint64_t carry = x[a];
#pragma unroll
        for (int q = 0; q < kBsvdPlanes; ++q) {
          const uint64_t c2 = pl[q] & carry;
          pl[q] ^= carry;
          carry = c2;
        }
        if (++nacc == kBsvdFlush) {
          bsvd_flush(pl, lcnt + w * 64);
          nacc = 0;
        }
      }
    }
  }
  if constexpr (MODE == kInitXor) {
    if (mine && xr) atomicXor(reinterpret_cast<unsigned long long*>(&s_pick[w]), (unsigned long long)xr);
  } else {
    if (mine && nacc) bsvd_flush(pl, lcnt + w * 64);
  }
  if (users) atomicAdd(&s_users, users);
  __syncthreads();
  if constexpr (MODE == kInitXor) {  // (two u32 halves of the atom's XOR: cnt[2 w], cnt[2 w + 1])
    auto* gx = reinterpret_cast<unsigned long long*>(cnt) + (uint64_t)k * mw;
    if (t < mw && s_pick[t]) atomicXor(&gx[t], (unsigned long long)s_pick[t]);
  } else {
    uint32_t* gc = cnt + (uint64_t)k * mw * 64;
    for (uint32_t j = t; j < mw * 64; j += 256)
      if (lcnt[j]) atomicAdd(&gc[j], lcnt[j]);
  }
  if constexpr (MODE == kInitColw) return;  // the counts are the result
  if (t == 0 && s_users) atomicAdd(&ucnt[k], s_users);
  __threadfence();
  __syncthreads();
  if (t == 0) s_last = atomicAdd(&tick[k], 1u) == gridDim.y - 1 ? 1u : 0u;
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  if (t == 0) {
    s_u = atomicExch(&ucnt[k], 0u);
    atomicExch(&tick[k], 0u);
  }
  __syncthreads();
  const uint32_t U = s_u;
  if constexpr (MODE == kInitXor) {
    auto* gx = reinterpret_cast<unsigned long long*>(cnt) + (uint64_t)k * mw;
    if (t < mw) D[(uint64_t)k * d_wpr + t] = atomicExch(&gx[t], 0ull);
  } else {
    uint32_t* gc = cnt + (uint64_t)k * mw * 64;
    for (uint32_t wi = wave; wi < mw; wi += 4) {  // wave-uniform: one word of the atom per wave
      const uint32_t j = wi * 64 + lane;
      const uint32_t c = atomicExch(&gc[j], 0u);
      bool nb;
      if constexpr (MODE == kInitCentroids) nb = 2u * c >= U;            // :161, a tie sets the bit, U = 0: all ones
      else if constexpr (MODE == kInitNeighbor) nb = U && c >= U / 2;    // :258-260 (U = 0: a zero or skipped pick)
      else nb = c >= U / 2;                                             // :214, U <= 1: all ones
      const uint64_t nw = __builtin_bitreverse64(__builtin_amdgcn_ballot_w64(nb && j < m));
      if (lane == 0) D[(uint64_t)k * d_wpr + wi] = nw;
    }
  }
}

// A.clear() over the first pw words of every row, and, with sel, A.set(i, sel[i]) (:118, :152); an index >= p is
// skipped (the row stays zero). One thread per word.
__global__ __launch_bounds__(256) void k_bsvd_init_coef(uint64_t* __restrict__ A, uint32_t n, uint32_t p, uint32_t pw,
                                                        uint32_t a_wpr, const uint32_t* __restrict__ sel) {
  const uint64_t total = (uint64_t)n * pw;
  for (uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (uint64_t)gridDim.x * 256) {
    const uint64_t i = idx / pw;
    const uint32_t w = (uint32_t)(idx - i * pw);
    uint64_t v = 0;
    if (sel) {
      const uint32_t k = sel[i];
      if (k < p && (k >> 6) == w) v = BIC_MSB >> (k & 63u);
    }
    A[i * a_wpr + w] = v;
  }
}

// counting_sort + ranking[m - k - 1] (util.cpp:7-51, bsvd.cpp:195-201): the k-th pivot is the column of rank k
// by (weight descending, column ascending); one workgroup, every column counts the columns before it.
__global__ __launch_bounds__(1024) void k_bsvd_init_rank(const uint32_t* __restrict__ colw, uint32_t m,
                                                         uint32_t* __restrict__ pivots) {
  __shared__ uint32_t s_w[4096];
  for (uint32_t c = threadIdx.x; c < m; c += 1024) s_w[c] = colw[c];
  __syncthreads();
  for (uint32_t c = threadIdx.x; c < m; c += 1024) {
    const uint32_t wc = s_w[c];
    uint32_t rank = 0;
    for (uint32_t o = 0; o < m; ++o) {
      const uint32_t wo = s_w[o];
      rank += (wo > wc || (wo == wc && o < c)) ? 1u : 0u;
    }
    pivots[rank] = c;
  }
}

// bit 63 - i % 64 of word i / 64: row i of E is non-zero over j < m. One row per lane.
__global__ __launch_bounds__(256) void k_bsvd_init_nonzero(const uint64_t* __restrict__ E, uint32_t n, uint32_t m,
                                                           uint32_t mw, uint32_t e_wpr, uint64_t* __restrict__ bitmap) {
  const uint32_t lane = lane_id(), nwords = (n + 63) / 64;
  const uint64_t last = (m & 63u) ? ~0ull << (64 - (m & 63u)) : ~0ull;
  for (uint32_t wv = blockIdx.x * 4 + wave_id(); wv < nwords; wv += gridDim.x * 4) {  // wave-uniform
    const uint64_t i = (uint64_t)wv * 64 + lane;
    uint64_t any = 0;
    if (i < n) {
      for (uint32_t w = 0; w + 1 < mw; ++w) any |= E[i * e_wpr + w];
      any |= E[i * e_wpr + mw - 1] & last;
    }
    const uint64_t bits = __builtin_bitreverse64(__builtin_amdgcn_ballot_w64(any != 0ull));
    if (lane == 0) bitmap[wv] = bits;
  }
}

namespace {
struct InitArena {
  uint32_t *tick, *ucnt, *colw, *pivots, *cnt;
  size_t zero_bytes;  // the counters from the arena's start
};
InitArena init_arena(void* scratch, uint32_t m, uint32_t p) {
  uint32_t* base = static_cast<uint32_t*>(scratch);
  const size_t mw = (m + 63) / 64;
  return {base, base + 4096, base + 2 * 4096, base + 3 * 4096, base + 4 * 4096, (4 * 4096 + (size_t)p * mw * 64) * 4};
}
}  // namespace

size_t bsvd_init_scratch_bytes(uint32_t n, uint32_t m, uint32_t p) {
  // the counters; then what bic_bsvd_initialize keeps: n or p indices, or the bitmap of non-zero rows
  return init_arena(nullptr, m, p).zero_bytes + (size_t)std::max(n, p) * 4 + 8;
}

void* bsvd_init_scratch_tail(void* scratch, uint32_t m, uint32_t p) {
  return static_cast<uint8_t*>(scratch) + init_arena(nullptr, m, p).zero_bytes;
}

void launch_bsvd_init(hipStream_t s, int mi, const uint64_t* E, uint32_t n, uint32_t m, uint32_t e_wpr, uint64_t* D,
                      uint32_t p, uint32_t d_wpr, uint64_t* A, uint32_t a_wpr, const uint32_t* sel, void* scratch) {
  const InitArena ar = init_arena(scratch, m, p);
  const uint32_t mw = (m + 63) / 64, pw = (p + 63) / 64;
  uint32_t lg = 0;
  while ((1u << lg) < mw) ++lg;
  launch_fill(s, scratch, 0, ar.zero_bytes);
  const bool cent = mi == kInitCentroids || mi == kInitXor;
  const uint64_t awords = (uint64_t)n * pw;
  k_bsvd_init_coef<<<(uint32_t)std::min<uint64_t>((awords + 255) / 256, 4096), 256, 0, s>>>(A, n, p, pw, a_wpr,
                                                                                          cent ? sel : nullptr);
  // shares of at least 1,024 rows, about 2,048 workgroups in all (at most 65,535 shares: gridDim.y)
  auto shares = [&](uint32_t rows, uint32_t atoms, uint32_t* chunk) {
    const uint32_t want = std::max(1u, std::min((2048u + atoms - 1) / atoms, (rows + 1023u) / 1024u));
    *chunk = (rows + want - 1) / want;
    return (rows + *chunk - 1) / *chunk;
  };
  uint32_t chunk = 0;
  if (mi == kInitPartition) {
    const uint32_t nsamp = (n + mw - 1) / mw, nsel = std::min(p, m);
    const uint32_t sy = shares(nsamp, 1, &chunk);
    k_bsvd_init<kInitColw><<<dim3(1, sy), 256, 0, s>>>(E, nsamp, m, mw, lg, e_wpr, D, d_wpr, nullptr, 0, chunk,
                                                        ar.colw, ar.ucnt, ar.tick);
    k_bsvd_init_rank<<<1, 1024, 0, s>>>(ar.colw, m, ar.pivots);
    const uint32_t gy = shares(n, nsel, &chunk);
    k_bsvd_init<kInitPartition><<<dim3(p, gy), 256, 0, s>>>(E, n, m, mw, lg, e_wpr, D, d_wpr, ar.pivots, nsel, chunk,
                                                             ar.cnt, ar.ucnt, ar.tick);
    return;
  }
  const uint32_t gy = shares(n, p, &chunk);
  const dim3 grid(p, gy);
  if (mi == kInitNeighbor)
    k_bsvd_init<kInitNeighbor><<<grid, 256, 0, s>>>(E, n, m, mw, lg, e_wpr, D, d_wpr, sel, p, chunk, ar.cnt, ar.ucnt,
                                                    ar.tick);
  else if (mi == kInitCentroids)
    k_bsvd_init<kInitCentroids><<<grid, 256, 0, s>>>(E, n, m, mw, lg, e_wpr, D, d_wpr, sel, p, chunk, ar.cnt, ar.ucnt,
                                                     ar.tick);
  else
    k_bsvd_init<kInitXor><<<grid, 256, 0, s>>>(E, n, m, mw, lg, e_wpr, D, d_wpr, sel, p, chunk, ar.cnt, ar.ucnt,
                                               ar.tick);
}

void launch_bsvd_init_nonzero(hipStream_t s, const uint64_t* E, uint32_t n, uint32_t m, uint32_t e_wpr,
                              uint64_t* bitmap) {
  const uint32_t nwords = (n + 63) / 64;
  k_bsvd_init_nonzero<<<std::min<uint32_t>((nwords + 3) / 4, 2048), 256, 0, s>>>(E, n, m, (m + 63) / 64, e_wpr, bitmap);
}

}  // namespace bic
