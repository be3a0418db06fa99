// bic_bsvd_wide.hip -- the three dictionary-learning steps of bic_bsvd.hip for rows of any width up to
// 1,048,576 bits (include/bic.h "wide rows"): what the role-switching learners (bsvd.cpp:1247-1434) run in
// the exchanged role, where an atom is a row of the transposed coefficients and as wide as the sample
// count, and what matrix mode runs on images wider than 4,096 columns. Same meaning, word for word, as the
// narrow kernels: whole words in distances, weights and XORs, D_k's last word masked in the PROXIMUS
// coefficient vote, padding bits of D and A never changed, words past a row's own never touched.
//
// A row no longer fits a wave, so the shapes differ:
//
//  * sparse coding: one workgroup per row, the row left in E (it is changed in place: every step the
//    reference takes is stored anyway), waves over the atoms, lanes over the words, the least
//    (distance, k) over the workgroup through LDS, repeated inside the launch until no atom lowers the weight;
//  * steepest rule: bit c of every atom, and every later use of it, depends on column c of E alone, so a
//    workgroup owns a chunk of kWideCW words of columns and walks all p atoms in order by itself, in one
//    launch; only "atom k changed" is combined across chunks (a flag per atom, ORed, counted afterwards);
//  * PROXIMUS: the narrow schedule (bic_bsvd.hip; two launches per round, the budget, the words read back
//    per batch), the atom half over column chunks, the coefficient half one wave per row.
//
// No workgroup waits for another. Rows are indexed as size_t(i) * wpr: n * wpr passes 32 bits.
#include "bic_bsvd_dev.h"

#include <algorithm>

namespace bic {

// ------------------------------------------------------------------------------------------------
// Sparse coding. A wave scans kWideJ atoms per pass over the row (one read of E's word against kWideJ of
// D's); the key is (distance << 32) | k: a distance reaches 2^20, past the narrow kernel's 20 bits.
// The weight after a step is the distance that won it.
// ------------------------------------------------------------------------------------------------
constexpr int kWideJ = 4;

__global__ __launch_bounds__(256) void k_bsvdw_coef(uint64_t* E, uint32_t n, uint32_t mw, uint32_t e_wpr,
                                                    const uint64_t* __restrict__ D, uint32_t p, uint32_t d_wpr,
                                                    uint64_t* A, uint32_t a_wpr, unsigned long long* changed) {
  __shared__ unsigned long long s_key[4];
  __shared__ uint32_t s_wgt[4];
  const uint32_t t = threadIdx.x, lane = lane_id(), wave = wave_id();
  uint32_t nchanged = 0;
  for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
    uint64_t* row = E + (size_t)i * e_wpr;
    uint32_t c = 0;
    for (uint32_t w = t; w < mw; w += 256) c += (uint32_t)__popcll(row[w]);
    c = wave_total_u32(c);
    if (lane == 0) s_wgt[wave] = c;
    __syncthreads();
    uint32_t wgt = s_wgt[0] + s_wgt[1] + s_wgt[2] + s_wgt[3];
    bool ch = false;
    for (;;) {  // (every step lowers the weight)
      unsigned long long best = ~0ull;
      for (uint32_t k0 = wave * kWideJ; k0 < p; k0 += 4 * kWideJ) {  // wave-uniform
        uint32_t d[kWideJ];
        const uint64_t* dk[kWideJ];
#pragma unroll
        for (int j = 0; j < kWideJ; ++j) {
          d[j] = 0;
          dk[j] = D + (size_t)min(k0 + j, p - 1) * d_wpr;  // (an atom past p is scanned and dropped)
        }
        for (uint32_t w = lane; w < mw; w += 64) {
          const uint64_t e = row[w];
#pragma unroll
          for (int j = 0; j < kWideJ; ++j) d[j] += (uint32_t)__popcll(e ^ dk[j][w]);
        }
#pragma unroll
        for (int j = 0; j < kWideJ; ++j) {
          const unsigned long long key = ((unsigned long long)wave_total_u32(d[j]) << 32) | (k0 + j);
          if (k0 + j < p && key < best) best = key;  // strict <, k ascending: the first k among equals
        }
      }
      if (lane == 0) s_key[wave] = best;
      __syncthreads();
      best = s_key[0];
#pragma unroll
      for (int q = 1; q < 4; ++q) best = s_key[q] < best ? s_key[q] : best;
      const uint32_t bestd = (uint32_t)(best >> 32), bestk = (uint32_t)best;
      if (bestd >= wgt) break;  // bsvd.cpp:439: only a strictly lower weight is a step
      const uint64_t* db = D + (size_t)bestk * d_wpr;
      for (uint32_t w = t; w < mw; w += 256) row[w] ^= db[w];
      if (t == 0) A[(size_t)i * a_wpr + (bestk >> 6)] ^= BIC_MSB >> (bestk & 63u);  // may switch an atom off
      wgt = bestd;
      ch = true;
      __syncthreads();  // the row's new words before the next scan; s_key read before it is written again
    }
    if (ch) ++nchanged;
    __syncthreads();
  }
  if (t == 0 && nchanged && changed) atomicAdd(changed, (unsigned long long)nchanged);
}

// ------------------------------------------------------------------------------------------------
// One atom over one chunk of columns (both dictionary rules). The users of atom k are the set bits of row k
// of At (the transpose of A); they are listed in LDS kWideBatch words of At (4,096 rows) at a time, and the
// thread (slot, w) adds word w0 + w of the users slot, slot + nslots, .. of the list to its bit-sliced
// counters. With U users and c' the count of E's bit, the count of (E ^ D_k)'s bit is c' where D_k's bit is
// 0 and U - c' where it is 1; the new bit is count > U / 2 (bsvd.cpp:502-506) for j < m, D_k's own past m.
// A change is carried into the users' rows at once: nobody else reads or writes these columns.
// ------------------------------------------------------------------------------------------------
constexpr uint32_t kWideCW = 16;     // words of a column chunk: 128-byte segments of a row
constexpr uint32_t kWideBatch = 64;  // words of At listed at a time

struct WideLds {
  uint32_t cnt[kWideCW * 64];
  uint32_t list[kWideBatch * 64];
  uint32_t pop[kWideBatch];
  uint64_t delta[kWideCW];
  uint32_t nlist, any;
};

// the rows with a bit set in words a0 .. a0 + kWideBatch - 1 of `at`, ascending, into L.list: their number
__device__ __forceinline__ uint32_t wide_list(const uint64_t* at, uint32_t a0, uint32_t atw, WideLds& L) {
  const uint32_t t = threadIdx.x;
  uint64_t bits = 0;
  if (t < kWideBatch) {
    if (a0 + t < atw) bits = ld_agent(&at[a0 + t]);
    L.pop[t] = (uint32_t)__popcll(bits);
  }
  __syncthreads();
  if (t < kWideBatch) {
    uint32_t off = 0;
    for (uint32_t q = 0; q < t; ++q) off += L.pop[q];
    const uint32_t base = (a0 + t) * 64;
    while (bits) {
      const uint32_t b = (uint32_t)__builtin_clzll(bits);
      bits &= ~(BIC_MSB >> b);
      L.list[off++] = base + b;
    }
    if (t == kWideBatch - 1) L.nlist = off;
  }
  __syncthreads();
  return L.nlist;
}

// true (in every thread) if the chunk's words w0 .. w0 + cw - 1 of atom k changed
__device__ __forceinline__ bool wide_atom(uint64_t* E, uint32_t m, uint32_t e_wpr, uint64_t* D, uint32_t d_wpr,
                                          const uint64_t* At, uint32_t atw, uint32_t k, uint32_t w0, uint32_t cw,
                                          WideLds& L) {
  const uint32_t t = threadIdx.x, lane = lane_id(), wave = wave_id();
  const uint32_t w = t % kWideCW, slot = t / kWideCW, nslots = 256u / kWideCW;
  const bool mine = w < cw;
  const uint64_t* at = At + (size_t)k * atw;
  for (uint32_t j = t; j < kWideCW * 64; j += 256) L.cnt[j] = 0;
  if (t == 0) L.any = 0;  // (wide_list's barriers come before the first use of either)
  uint64_t pl[kBsvdPlanes];
#pragma unroll
  for (int q = 0; q < kBsvdPlanes; ++q) pl[q] = 0;
  uint32_t nacc = 0, U = 0;
  for (uint32_t a0 = 0; a0 < atw; a0 += kWideBatch) {
    if (a0) __syncthreads();  // the last batch's list has been read
    const uint32_t nl = wide_list(at, a0, atw, L);
    U += nl;
    if (mine)
      for (uint32_t u = slot; u < nl; u += nslots) {
        uint64_t carry = E[(size_t)L.list[u] * e_wpr + w0 + w];
#pragma unroll
        for (int q = 0; q < kBsvdPlanes; ++q) {  // the vertical adder: plane q holds bit q of 64 counts
          const uint64_t c2 = pl[q] & carry;
          pl[q] ^= carry;
          carry = c2;
        }
        if (++nacc == kBsvdFlush) {
          bsvd_flush(pl, L.cnt + w * 64);
          nacc = 0;
        }
      }
  }
  if (mine && nacc) bsvd_flush(pl, L.cnt + w * 64);
  __syncthreads();
  bool any = false;
  for (uint32_t wi = wave; wi < cw; wi += 4) {  // wave-uniform: one word of the atom per wave
    const uint32_t j = (w0 + wi) * 64 + lane;
    const uint64_t dk = D[(size_t)k * d_wpr + w0 + wi];
    const uint32_t c0 = L.cnt[wi * 64 + lane];
    const bool dbit = (dk >> (63 - lane)) & 1ull;
    const uint32_t c = dbit ? U - c0 : c0;
    const bool nb = (U && j < m) ? c > U / 2 : dbit;  // U = 0: the atom is skipped (bsvd.cpp:499)
    const uint64_t nw = __builtin_bitreverse64(__builtin_amdgcn_ballot_w64(nb));
    const uint64_t dl = dk ^ nw;
    if (lane == 0) {
      L.delta[wi] = dl;
      if (dl) D[(size_t)k * d_wpr + w0 + wi] = nw;
    }
    any |= dl != 0;
  }
  if (any && lane == 0) atomicOr(&L.any, 1u);
  __syncthreads();
  const bool chg = L.any != 0;
  __syncthreads();  // (the next atom clears L.any)
  if (!chg) return false;
  const uint64_t dl = mine ? L.delta[w] : 0ull;
  for (uint32_t a0 = 0; a0 < atw; a0 += kWideBatch) {
    uint32_t nl = U;  // one batch: the list still stands
    if (atw > kWideBatch) {
      if (a0) __syncthreads();
      nl = wide_list(at, a0, atw, L);
    }
    if (dl)
      for (uint32_t u = slot; u < nl; u += nslots) E[(size_t)L.list[u] * e_wpr + w0 + w] ^= dl;
  }
  __syncthreads();  // the users' rows before the next atom counts them; the list before it is rebuilt
  return true;
}

// the steepest rule (bsvd.cpp:463-527): every atom in order, flags[k] |= 1 where atom k changed
__global__ __launch_bounds__(256) void k_bsvdw_dict(uint64_t* E, uint32_t m, uint32_t mw, uint32_t e_wpr, uint64_t* D,
                                                    uint32_t p, uint32_t d_wpr, const uint64_t* At, uint32_t atw,
                                                    uint32_t* flags) {
  __shared__ WideLds L;
  const uint32_t w0 = blockIdx.x * kWideCW, cw = min(kWideCW, mw - w0);
  for (uint32_t k = 0; k < p; ++k)
    if (wide_atom(E, m, e_wpr, D, d_wpr, At, atw, k, w0, cw, L) && threadIdx.x == 0) atomicOr(&flags[k], 1u);
}

__global__ __launch_bounds__(256) void k_bsvdw_count(const uint32_t* flags, uint32_t p, unsigned long long* changed) {
  uint32_t c = 0;
  for (uint32_t k = threadIdx.x; k < p; k += 256) c += flags[k] ? 1u : 0u;
  c = wave_total_u32(c);
  if (lane_id() == 0 && c) atomicAdd(changed, (unsigned long long)c);
}

// ------------------------------------------------------------------------------------------------
// PROXIMUS (bsvd.cpp:530-735) on the narrow schedule's words (bic_bsvd_dev.h). The atom half of a round is
// wide_atom over the column chunks; the workgroup that takes the launch's last ticket does what the narrow
// atom half's last workgroup does, with "delta != 0" ORed over the chunks in misc[kProxAny]. The change is
// already in E when the coefficient half runs, so that half needs no delta: one wave per row,
//
//   c = |E_i & D_k| over j < m (D_k's last word masked), |S| = |D_k| over j < m, Aw = c for a non-user and
//   |S| - c for a user; the new A(i,k) is Aw > |S| / 2 (|S| = 0: no vote); where it differs A(i,k) and its
//   bit in At flip (the rows of a word of At are in different waves: an atomic XOR) and E_i ^= D_k for j < m.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bsvdw_prox_atom(uint64_t* E, uint32_t m, uint32_t mw, uint32_t e_wpr,
                                                         uint64_t* D, uint32_t p, uint32_t d_wpr, const uint64_t* At,
                                                         uint32_t atw, uint32_t k, uint32_t* misc, uint32_t pr,
                                                         uint32_t pflags) {
  __shared__ WideLds L;
  __shared__ uint32_t s_last;
  if (prox_leaves<true>(misc, k, pr, pflags) || k >= p) return;  // (k = p: the last atom's stall check)
  const uint32_t w0 = blockIdx.x * kWideCW, cw = min(kWideCW, mw - w0);
  const bool any = wide_atom(E, m, e_wpr, D, d_wpr, At, atw, k, w0, cw, L);
  if (threadIdx.x == 0) {
    if (any) atomicOr(&misc[kProxAny], 1u);
    __threadfence();
    s_last = atomicAdd(&misc[1], 1u) == gridDim.x - 1 ? 1u : 0u;
  }
  __syncthreads();
  if (!s_last || threadIdx.x != 0) return;
  __threadfence();
  const uint32_t all = atomicExch(&misc[kProxAny], 0u);
  atomicExch(&misc[1], 0u);
  st_agent(&misc[kProxAgain + (pr & 1u)], all);  // the coefficient half ORs its flips in
  atomicAdd(reinterpret_cast<unsigned long long*>(&misc[kProxRounds]), 1ull);
  const uint32_t before = (pflags & kProxFresh) ? 0u : ld_agent(&misc[kProxKch]);
  if (all && !before) atomicAdd(reinterpret_cast<unsigned long long*>(&misc[kProxChanged]), 1ull);  // once per atom
  st_agent(&misc[kProxKch], before | all);
}

__global__ __launch_bounds__(256) void k_bsvdw_prox_coef(uint64_t* E, uint32_t n, uint32_t m, uint32_t mw,
                                                         uint32_t e_wpr, const uint64_t* __restrict__ D,
                                                         uint32_t d_wpr, uint64_t* A, uint32_t a_wpr, uint64_t* At,
                                                         uint32_t atw, uint32_t k, uint32_t pr, uint32_t* misc) {
  __shared__ uint32_t s_part[4];
  if (prox_leaves<false>(misc, k, pr, 0u)) return;
  const uint32_t t = threadIdx.x, lane = lane_id(), wave = wave_id();
  const uint64_t* dk = D + (size_t)k * d_wpr;
  const uint64_t lastm = (m & 63u) ? ~0ull << (64 - (m & 63u)) : ~0ull;  // j < m only (bsvd.cpp:681)
  uint32_t c = 0;
  for (uint32_t w = t; w < mw; w += 256) c += (uint32_t)__popcll(dk[w] & (w == mw - 1 ? lastm : ~0ull));
  c = wave_total_u32(c);
  if (lane == 0) s_part[wave] = c;
  __syncthreads();
  const uint32_t S = s_part[0] + s_part[1] + s_part[2] + s_part[3];
  if (!S) return;  // no vote (:694)
  const uint64_t kbit = BIC_MSB >> (k & 63u);
  for (uint32_t i = blockIdx.x * 4 + wave; i < n; i += gridDim.x * 4) {  // wave-uniform
    uint64_t* row = E + (size_t)i * e_wpr;
    const uint64_t aword = A[(size_t)i * a_wpr + (k >> 6)];
    const bool a = (aword & kbit) != 0;
    c = 0;
    for (uint32_t w = lane; w < mw; w += 64) c += (uint32_t)__popcll(row[w] & dk[w] & (w == mw - 1 ? lastm : ~0ull));
    c = wave_total_u32(c);
    const bool nb = (a ? S - c : c) > S / 2;
    if (nb == a) continue;
    for (uint32_t w = lane; w < mw; w += 64) {
      const uint64_t x = dk[w] & (w == mw - 1 ? lastm : ~0ull);
      if (x) row[w] ^= x;
    }
    if (lane == 0) {
      A[(size_t)i * a_wpr + (k >> 6)] = aword ^ kbit;
      atomicXor(reinterpret_cast<unsigned long long*>(&At[(size_t)k * atw + (i >> 6)]),
                (unsigned long long)(BIC_MSB >> (i & 63u)));
      atomicOr(&misc[kProxAgain + (pr & 1u)], 1u);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// The arena is the narrow dictionary update's (launch_bsvd_dict_prepare: the schedule's words and the
// transpose of A) with the p flags of the steepest rule after it.
// ------------------------------------------------------------------------------------------------
namespace {
size_t wide_flags_offset(uint32_t n, uint32_t p) { return (bsvd_dict_scratch_bytes(n, p) + 7) & ~(size_t)7; }
uint32_t* wide_misc(void* scratch) { return static_cast<uint32_t*>(scratch); }
uint64_t* wide_at(void* scratch) { return reinterpret_cast<uint64_t*>(static_cast<uint8_t*>(scratch) + kBsvdDictHead); }
uint32_t wide_chunks(uint32_t m) { return ((m + 63) / 64 + kWideCW - 1) / kWideCW; }
}  // namespace

size_t bsvd_wide_scratch_bytes(uint32_t n, uint32_t p) { return wide_flags_offset(n, p) + (size_t)p * 4; }

void launch_bsvd_wide_coef(hipStream_t s, uint64_t* E, uint32_t n, uint32_t m, uint32_t e_wpr, const uint64_t* D,
                           uint32_t p, uint32_t d_wpr, uint64_t* A, uint32_t a_wpr, uint64_t* changed) {
  const uint32_t grid = std::min<uint32_t>(n, 2048);
  if (grid)
    k_bsvdw_coef<<<grid, 256, 0, s>>>(E, n, (m + 63) / 64, e_wpr, D, p, d_wpr, A, a_wpr,
                                      reinterpret_cast<unsigned long long*>(changed));
}

void launch_bsvd_wide_prepare(hipStream_t s, uint32_t n, uint32_t p, const uint64_t* A, uint32_t a_wpr,
                              void* scratch) {
  launch_bsvd_dict_prepare(s, n, p, A, a_wpr, scratch);
  launch_fill(s, static_cast<uint8_t*>(scratch) + wide_flags_offset(n, p), 0, (size_t)p * 4);
}

void launch_bsvd_wide_dict(hipStream_t s, uint64_t* E, uint32_t n, uint32_t m, uint32_t e_wpr, uint64_t* D,
                           uint32_t p, uint32_t d_wpr, void* scratch, uint64_t* changed) {
  uint32_t* flags = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(scratch) + wide_flags_offset(n, p));
  k_bsvdw_dict<<<wide_chunks(m), 256, 0, s>>>(E, m, (m + 63) / 64, e_wpr, D, p, d_wpr, wide_at(scratch), (n + 63) / 64,
                                              flags);
  k_bsvdw_count<<<1, 256, 0, s>>>(flags, p, reinterpret_cast<unsigned long long*>(changed));
}

void launch_bsvd_wide_prox_atom(hipStream_t s, uint64_t* E, uint32_t n, uint32_t m, uint32_t e_wpr, uint64_t* D,
                                uint32_t p, uint32_t d_wpr, void* scratch, uint32_t k, uint32_t r, uint32_t budget,
                                bool check_prev, bool fresh) {
  // (the previous atom's last budgeted round is round budget - 1: that is the parity of its `again`)
  const uint32_t pflags = (check_prev ? kProxCheckPrev : 0u) | (fresh ? kProxFresh : 0u) |
                          (((budget - 1) & 1u) ? kProxPrevParity : 0u);
  k_bsvdw_prox_atom<<<k < p ? wide_chunks(m) : 1u, 256, 0, s>>>(E, m, (m + 63) / 64, e_wpr, D, p, d_wpr,
                                                                 wide_at(scratch), (n + 63) / 64, k,
                                                                 wide_misc(scratch), r, pflags);
}

void launch_bsvd_wide_prox_coef(hipStream_t s, uint64_t* E, uint32_t n, uint32_t m, uint32_t e_wpr, const uint64_t* D,
                                uint32_t d_wpr, uint64_t* A, uint32_t a_wpr, void* scratch, uint32_t k, uint32_t r) {
  const uint32_t grid = std::min<uint32_t>((n + 3) / 4, 2048);
  k_bsvdw_prox_coef<<<grid, 256, 0, s>>>(E, n, m, (m + 63) / 64, e_wpr, D, d_wpr, A, a_wpr, wide_at(scratch),
                                         (n + 63) / 64, k, r, wide_misc(scratch));
}

}  // namespace bic
