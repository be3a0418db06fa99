// bic_bsvd_dev.h -- what the dictionary-learning kernels of bic_bsvd.hip (rows of at most 64 words) and
// bic_bsvd_wide.hip (rows of any width) share on the device: the agent-scope loads and stores of the
// schedule's words, the bit-sliced column counters and the PROXIMUS schedule's leave test.
#pragma once
#include "bic_device.h"

namespace bic {

__device__ __forceinline__ uint32_t ld_agent(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint64_t ld_agent(const uint64_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(uint32_t* p, uint32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Bit-sliced carry-save counters: plane q holds bit q of 64 column counts, so five planes take 31 rows
// between two flushes into the 64 LDS counts of the word.
constexpr int kBsvdPlanes = 5;
constexpr uint32_t kBsvdFlush = (1u << kBsvdPlanes) - 1;

__device__ __forceinline__ void bsvd_flush(uint64_t (&pl)[kBsvdPlanes], uint32_t* lc) {
  for (uint32_t b = 0; b < 64; ++b) {
    uint32_t c = 0;
#pragma unroll
    for (int q = 0; q < kBsvdPlanes; ++q) c |= (uint32_t)((pl[q] >> (63 - b)) & 1ull) << q;
    if (c) atomicAdd(&lc[b], c);
  }
#pragma unroll
  for (int q = 0; q < kBsvdPlanes; ++q) pl[q] = 0;
}

// misc: [0] U, [1] ticket, [2] delta != 0; the PROXIMUS schedule's words (below): [3], [4] `again` by round
// parity, [5] `stalled` (atom + 1, sticky), [6] the atom's bits changed in an earlier round, [7] the wide atom
// half's "delta != 0" ORed over its workgroups, [8..9] u64 rounds run, [12..13] u64 atoms changed
constexpr uint32_t kProxAgain = 3, kProxStalled = 5, kProxKch = 6, kProxAny = 7, kProxRounds = 8, kProxChanged = 12;
static_assert(kProxStalled * 4 == kBsvdProxStalled && kProxRounds * 4 == kBsvdProxRounds &&
              kProxChanged * 4 == kBsvdProxChanged, "the host reads these words back");
constexpr uint32_t kProxCheckPrev = 1, kProxFresh = 2, kProxPrevParity = 4;

// Whether a launch of the PROXIMUS schedule leaves at once (the same answer in every workgroup: the words it
// reads are written by earlier launches only, or, `stalled`, by this launch where `again` already says leave).
// Round pr > 0 leaves when round pr - 1 moved nothing. The atom half of round 0 looks at the atom before: if
// its last budgeted round still moved something, that atom is recorded in `stalled`, and every later launch
// leaves until the host has read the word, cleared it and enqueued from that atom again.
template <bool ATOM>
__device__ __forceinline__ bool prox_leaves(uint32_t* misc, uint32_t k, uint32_t pr, uint32_t pflags) {
  if (ld_agent(&misc[kProxStalled])) return true;
  if (pr == 0) {
    if (!ATOM || !(pflags & kProxCheckPrev)) return false;
    if (!ld_agent(&misc[kProxAgain + ((pflags & kProxPrevParity) ? 1 : 0)])) return false;
    if (blockIdx.x == 0 && threadIdx.x == 0) st_agent(&misc[kProxStalled], k);  // atom k - 1, plus one
    return true;
  }
  if (ld_agent(&misc[kProxAgain + ((pr - 1) & 1u)])) return false;
  if (ATOM && blockIdx.x == 0 && threadIdx.x == 0) st_agent(&misc[kProxAgain + (pr & 1u)], 0u);
  return true;
}

}  // namespace bic
