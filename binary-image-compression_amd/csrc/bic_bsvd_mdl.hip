// bic_bsvd_mdl.hip -- what the reference's MDL model-order searches (bsvd.cpp:1438-1717) need on the device
// (include/bic.h "MDL model order"):
//
//  * bsvd.cpp:1450-1456 the weights behind model_codelength: |E|, |D_k| and |A_k| (column k of A), every read
//    masked at the row's trailing word as get_block does (binmat.h:188-190);
//  * bsvd.cpp:1578-1583 the backward search's removal scores: |E ^ A_k^t D_k| for every atom k at once, as
//    |E| + the sum over atom k's users of |E_i ^ D_k| - |E_i|: work proportional to A's set bits;
//  * bsvd.cpp:1594-1610 and :1497-1513 a model shrunk by one atom and grown by one, in place.
//
// Plane layout as in bic_bsvd.hip. Every sum is an integer sum (LDS and global atomic adds): the order of the adds
// does not matter, so the results are the same from run to run. No workgroup waits for another.
#include "bic_bsvd_dev.h"

#include <algorithm>

namespace bic {

namespace {
// the mask of a row's last word: the top m - 64 (mw - 1) bits
__host__ __device__ inline uint64_t tail_mask(uint32_t cols) {
  const uint32_t b = cols & 63u;
  return b ? ~(~0ull >> b) : ~0ull;
}
inline uint32_t log2_ceil(uint32_t v, uint32_t cap) {
  uint32_t lg = 0;
  while ((1u << lg) < v && lg < cap) ++lg;
  return lg;
}
// rows of mw words that one workgroup takes at a time: about 16 Ki words, indexed in 32 bits
inline uint32_t chunk_rows(uint32_t mw) { return std::max<uint32_t>(1u, 16384u / mw); }
}  // namespace

// ------------------------------------------------------------------------------------------------
// |E| over columns < m. A workgroup walks chunks of rpc rows as one flat run of rpc * mw words (rows of a
// few words would leave most of a wave idle otherwise); one LDS add per thread, one global add per workgroup.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bsvd_mdl_weight(const uint64_t* __restrict__ E, uint32_t n, uint32_t mw,
                                                         uint32_t e_wpr, uint64_t tail, uint32_t rpc,
                                                         unsigned long long* we) {
  __shared__ unsigned long long s_sum;
  if (threadIdx.x == 0) s_sum = 0;
  __syncthreads();
  unsigned long long acc = 0;
  const uint64_t nchunks = ((uint64_t)n + rpc - 1) / rpc;
  for (uint64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const uint64_t r0 = c * rpc;
    const uint32_t cnt = (n - r0 < rpc ? (uint32_t)(n - r0) : rpc) * mw;
    for (uint32_t j = threadIdx.x; j < cnt; j += 256) {
      const uint32_t r = j / mw, w = j - r * mw;
      uint64_t v = E[(r0 + r) * e_wpr + w];
      if (w + 1 == mw) v &= tail;
      acc += (uint32_t)__popcll(v);
    }
  }
  if (acc) atomicAdd(&s_sum, acc);
  __syncthreads();
  if (threadIdx.x == 0 && s_sum) atomicAdd(we, s_sum);
}

// |D_k| over columns < m: one wave per atom, stored (not added)
__global__ __launch_bounds__(256) void k_bsvd_mdl_weight_rows(const uint64_t* __restrict__ D, uint32_t p, uint32_t mw,
                                                              uint32_t d_wpr, uint64_t tail, uint32_t* wd) {
  const uint32_t lane = lane_id(), k = blockIdx.x * 4 + wave_id();
  if (k >= p) return;  // (wave-uniform)
  uint32_t c = 0;
  for (uint32_t w = lane; w < mw; w += 64) {
    uint64_t v = D[(uint64_t)k * d_wpr + w];
    if (w + 1 == mw) v &= tail;
    c += (uint32_t)__popcll(v);
  }
  c = wave_total_u32(c);
  if (lane == 0) wd[k] = c;
}

// The column counts of A for k < p: thread (slot, w) adds word w of the rows slot, slot + nslots, .. of its
// workgroup's share into bit-sliced counters (bic_bsvd_dev.h), those into the workgroup's LDS counts, those
// into wa. Columns >= p (A's padding) are counted in LDS and never stored.
__global__ __launch_bounds__(256) void k_bsvd_mdl_weight_cols(const uint64_t* __restrict__ A, uint32_t n, uint32_t p,
                                                              uint32_t pw, uint32_t a_wpr, uint32_t lg, uint32_t* wa) {
  __shared__ uint32_t lcnt[64 * 64];
  const uint32_t t = threadIdx.x, w = t & ((1u << lg) - 1u), slot = t >> lg, nslots = 256u >> lg;
  for (uint32_t j = t; j < pw * 64; j += 256) lcnt[j] = 0;
  __syncthreads();
  if (w < pw) {
    uint64_t pl[kBsvdPlanes];
#pragma unroll
    for (int q = 0; q < kBsvdPlanes; ++q) pl[q] = 0;
    uint32_t nacc = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * nslots + slot; i < n; i += (uint64_t)gridDim.x * nslots) {
      uint64_t carry = A[i * a_wpr + w];
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
    if (nacc) bsvd_flush(pl, lcnt + w * 64);
  }
  __syncthreads();
  for (uint32_t k = t; k < p; k += 256)
    if (lcnt[k]) atomicAdd(&wa[k], lcnt[k]);
}

void launch_bsvd_mdl_weights(hipStream_t s, const uint64_t* E, uint32_t n, uint32_t m, uint32_t e_wpr, const uint64_t* D,
                             uint32_t p, uint32_t d_wpr, const uint64_t* A, uint32_t a_wpr, uint64_t* we, uint32_t* wd,
                             uint32_t* wa) {
  const uint32_t mw = (m + 63) / 64, rpc = chunk_rows(mw);
  const uint64_t tail = tail_mask(m);
  launch_fill(s, we, 0, 8);
  const uint64_t nchunks = ((uint64_t)n + rpc - 1) / rpc;
  k_bsvd_mdl_weight<<<(uint32_t)std::min<uint64_t>(nchunks, 1024), 256, 0, s>>>(
      E, n, mw, e_wpr, tail, rpc, reinterpret_cast<unsigned long long*>(we));
  if (!p) return;
  launch_fill(s, wa, 0, (size_t)p * 4);
  k_bsvd_mdl_weight_rows<<<(p + 3) / 4, 256, 0, s>>>(D, p, mw, d_wpr, tail, wd);
  const uint32_t pw = (p + 63) / 64, lg = log2_ceil(pw, 6), nslots = 256u >> lg;
  const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)n + nslots - 1) / nslots, 512);
  k_bsvd_mdl_weight_cols<<<grid, 256, 0, s>>>(A, n, p, pw, a_wpr, lg, wa);
}

// ------------------------------------------------------------------------------------------------
// The removal scores. One wave per row i: it holds A_i (a word per lane, the last one masked at p) and walks its
// set bits; for atom k the lanes share the words of (E_i ^ D_k) - E_i, and lane 0 adds the signed difference of the
// two weights to the workgroup's LDS score of k (two's complement in 64 bits, so the adds commute). D_k is read
// where it lies: nothing is staged, so no number of atoms has to fit into LDS. The workgroup's scores, and
// its rows' own weight (slot p), go to the global ones at the end; k_bsvd_mdl_drop_finish adds |E| to every score.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bsvd_mdl_drop(const uint64_t* __restrict__ E, uint32_t n, uint32_t mw,
                                                       uint32_t e_wpr, uint64_t tail, const uint64_t* __restrict__ D,
                                                       uint32_t p, uint32_t d_wpr, const uint64_t* __restrict__ A,
                                                       uint32_t a_wpr, unsigned long long* score,
                                                       unsigned long long* we) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long mdl_acc[];  // p scores, then the rows' weight
  const uint32_t t = threadIdx.x, lane = lane_id(), wave = wave_id();
  const uint32_t pw = (p + 63) / 64;
  const uint64_t ptail = tail_mask(p);
  for (uint32_t k = t; k <= p; k += 256) mdl_acc[k] = 0;
  __syncthreads();
  for (uint64_t i = (uint64_t)blockIdx.x * 4 + wave; i < n; i += (uint64_t)gridDim.x * 4) {
    const uint64_t* e = E + i * e_wpr;
    uint64_t aw = lane < pw ? A[i * a_wpr + lane] : 0ull;
    if (lane + 1 == pw) aw &= ptail;
    uint64_t e0 = lane < mw ? e[lane] : 0ull;  // the row's first 64 words stay in registers
    if (lane + 1 == mw) e0 &= tail;
    uint32_t ew = (uint32_t)__popcll(e0);
    for (uint32_t w = lane + 64; w < mw; w += 64) {
      uint64_t v = e[w];
      if (w + 1 == mw) v &= tail;
      ew += (uint32_t)__popcll(v);
    }
    ew = wave_total_u32(ew);
    uint64_t nz = __ballot(aw != 0ull);
    while (nz) {  // (wave-uniform)
      const uint32_t wl = (uint32_t)__builtin_ctzll(nz);
      nz &= nz - 1;
      uint64_t bits = (uint64_t)__shfl((unsigned long long)aw, (int)wl);
      while (bits) {
        const uint32_t b = (uint32_t)__builtin_clzll(bits);
        bits &= ~(BIC_MSB >> b);
        const uint32_t k = wl * 64 + b;
        const uint64_t* d = D + (uint64_t)k * d_wpr;
        uint32_t c = 0;
        if (lane < mw) {
          uint64_t v = d[lane];
          if (lane + 1 == mw) v &= tail;
          c = (uint32_t)__popcll(v ^ e0);
        }
        for (uint32_t w = lane + 64; w < mw; w += 64) {
          uint64_t v = d[w] ^ e[w];
          if (w + 1 == mw) v &= tail;
          c += (uint32_t)__popcll(v);
        }
        c = wave_total_u32(c);
        if (lane == 0) atomicAdd(&mdl_acc[k], (unsigned long long)((long long)c - (long long)ew));
      }
    }
    if (lane == 0 && ew) atomicAdd(&mdl_acc[p], (unsigned long long)ew);
  }
  __syncthreads();
  for (uint32_t k = t; k < p; k += 256)
    if (mdl_acc[k]) atomicAdd(&score[k], mdl_acc[k]);
  if (t == 0 && mdl_acc[p]) atomicAdd(we, mdl_acc[p]);
}

__global__ __launch_bounds__(256) void k_bsvd_mdl_drop_finish(unsigned long long* score, uint32_t p,
                                                              const unsigned long long* we) {
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k < p) score[k] += *we;
}

size_t bsvd_mdl_drop_scratch_bytes() { return 64; }

void launch_bsvd_mdl_drop_weights(hipStream_t s, const uint64_t* E, uint32_t n, uint32_t m, uint32_t e_wpr,
                                  const uint64_t* D, uint32_t p, uint32_t d_wpr, const uint64_t* A, uint32_t a_wpr,
                                  uint64_t* score, void* scratch) {
  const uint32_t mw = (m + 63) / 64;
  auto* we = reinterpret_cast<unsigned long long*>(scratch);
  auto* sc = reinterpret_cast<unsigned long long*>(score);
  launch_fill(s, we, 0, 8);
  launch_fill(s, score, 0, (size_t)p * 8);
  const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)n + 3) / 4, 1024);
  k_bsvd_mdl_drop<<<grid, 256, ((size_t)p + 1) * 8, s>>>(E, n, mw, e_wpr, tail_mask(m), D, p, d_wpr, A, a_wpr, sc, we);
  k_bsvd_mdl_drop_finish<<<(p + 255) / 256, 256, 0, s>>>(sc, p, we);
}

// ------------------------------------------------------------------------------------------------
// One atom out. D: rows k + 1 .. p - 1 move down one row. A workgroup owns a band of word columns; its slots
// take nslots consecutive rows per round, every slot reads the row above its own, the workgroup meets, then
// every slot stores: a round's stores touch only rows that the same round has read. A: a wave per row, a word
// per lane, the neighbour's top bit through a shuffle (no word is read after it was written); columns > k move
// one place towards the MSB, and everything from column p - 1 on inside the row's ceil(p / 64) words becomes 0.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bsvd_mdl_drop_row(uint64_t* D, uint32_t p, uint32_t mw, uint32_t d_wpr,
                                                           uint32_t k, uint32_t lg) {
  const uint32_t t = threadIdx.x, wl = t & ((1u << lg) - 1u), slot = t >> lg, nslots = 256u >> lg;
  const uint32_t w = (blockIdx.x << lg) + wl;
  const bool mine = w < mw;
  for (uint32_t r0 = k; r0 + 1 < p; r0 += nslots) {  // (the same trip count in every thread)
    const uint32_t r = r0 + slot;
    const bool act = mine && r + 1 < p;
    const uint64_t v = act ? D[(uint64_t)(r + 1) * d_wpr + w] : 0ull;
    __syncthreads();
    if (act) D[(uint64_t)r * d_wpr + w] = v;
  }
}

__global__ __launch_bounds__(256) void k_bsvd_mdl_drop_col(uint64_t* A, uint32_t n, uint32_t p, uint32_t a_wpr,
                                                           uint32_t k) {
  const uint32_t lane = lane_id(), pw = (p + 63) / 64, kw = k >> 6, kb = k & 63u, q = p - 1;
  for (uint64_t i = (uint64_t)blockIdx.x * 4 + wave_id(); i < n; i += (uint64_t)gridDim.x * 4) {
    const uint64_t v = lane < pw ? A[i * a_wpr + lane] : 0ull;
    uint64_t nx = (uint64_t)__shfl_down((unsigned long long)v, 1u);
    if (lane + 1 >= pw) nx = 0ull;
    const uint64_t sh = (v << 1) | (nx >> 63);
    const uint64_t hi = kb ? ~(~0ull >> kb) : 0ull;  // word kw: the columns before k stay
    uint64_t out = lane > kw ? sh : ((v & hi) | (sh & ~hi));
    if (lane * 64u >= q) out = 0ull;
    else if (lane * 64u + 64u > q) out &= ~(~0ull >> (q - lane * 64u));
    if (lane >= kw && lane < pw) A[i * a_wpr + lane] = out;
  }
}

void launch_bsvd_mdl_drop_atom(hipStream_t s, uint64_t* D, uint32_t p, uint32_t m, uint32_t d_wpr, uint64_t* A,
                               uint32_t n, uint32_t a_wpr, uint32_t k) {
  const uint32_t mw = (m + 63) / 64, lg = log2_ceil(mw, 8);
  if (k + 1 < p) k_bsvd_mdl_drop_row<<<(mw + (1u << lg) - 1) >> lg, 256, 0, s>>>(D, p, mw, d_wpr, k, lg);
  k_bsvd_mdl_drop_col<<<(uint32_t)std::min<uint64_t>(((uint64_t)n + 3) / 4, 2048), 256, 0, s>>>(A, n, p, a_wpr, k);
}

// ------------------------------------------------------------------------------------------------
// One atom in: row p of D = atom masked at m; column p of A = bit 63 of every row of coefs, the columns after
// it inside word p / 64 cleared (word p / 64 is written whole when p is a multiple of 64).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bsvd_mdl_append(uint64_t* D, uint32_t p, uint32_t mw, uint32_t d_wpr,
                                                         uint64_t tail, const uint64_t* __restrict__ atom, uint64_t* A,
                                                         uint32_t n, uint32_t a_wpr, const uint64_t* __restrict__ coefs,
                                                         uint32_t c_wpr, uint32_t row_blocks) {
  if (blockIdx.x < row_blocks) {
    const uint32_t w = blockIdx.x * 256 + threadIdx.x;
    if (w < mw) D[(uint64_t)p * d_wpr + w] = w + 1 == mw ? atom[w] & tail : atom[w];
    return;
  }
  const uint32_t pwi = p >> 6, b = p & 63u;
  for (uint64_t i = (uint64_t)(blockIdx.x - row_blocks) * 256 + threadIdx.x; i < n;
       i += (uint64_t)(gridDim.x - row_blocks) * 256) {
    const uint64_t old = b ? A[i * a_wpr + pwi] & ~(~0ull >> b) : 0ull;
    A[i * a_wpr + pwi] = old | ((coefs[i * c_wpr] & BIC_MSB) >> b);
  }
}

void launch_bsvd_mdl_append_atom(hipStream_t s, uint64_t* D, uint32_t p, uint32_t m, uint32_t d_wpr, uint64_t* A,
                                 uint32_t n, uint32_t a_wpr, const uint64_t* atom, const uint64_t* coefs,
                                 uint32_t c_wpr) {
  const uint32_t mw = (m + 63) / 64, row_blocks = (mw + 255) / 256;
  const uint32_t col_blocks = (uint32_t)std::min<uint64_t>(((uint64_t)n + 255) / 256, 2048);
  k_bsvd_mdl_append<<<row_blocks + col_blocks, 256, 0, s>>>(D, p, mw, d_wpr, tail_mask(m), atom, A, n, a_wpr, coefs,
                                                             c_wpr, row_blocks);
}

// dst (rows x words, pitch d_wpr) = src (pitch s_wpr): the searches' working copies
__global__ __launch_bounds__(256) void k_bsvd_mdl_copy(uint64_t* __restrict__ dst, uint32_t d_wpr,
                                                       const uint64_t* __restrict__ src, uint32_t s_wpr, uint32_t rows,
                                                       uint32_t words, uint32_t rpc) {
  const uint64_t nchunks = ((uint64_t)rows + rpc - 1) / rpc;
  for (uint64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const uint64_t r0 = c * rpc;
    const uint32_t cnt = (rows - r0 < rpc ? (uint32_t)(rows - r0) : rpc) * words;
    for (uint32_t j = threadIdx.x; j < cnt; j += 256) {
      const uint32_t r = j / words, w = j - r * words;
      dst[(r0 + r) * d_wpr + w] = src[(r0 + r) * s_wpr + w];
    }
  }
}

void launch_bsvd_mdl_copy(hipStream_t s, uint64_t* dst, uint32_t d_wpr, const uint64_t* src, uint32_t s_wpr,
                          uint32_t rows, uint32_t words) {
  if (!rows || !words) return;
  const uint32_t rpc = chunk_rows(words);
  const uint64_t nchunks = ((uint64_t)rows + rpc - 1) / rpc;
  k_bsvd_mdl_copy<<<(uint32_t)std::min<uint64_t>(nchunks, 2048), 256, 0, s>>>(dst, d_wpr, src, s_wpr, rows, words, rpc);
}

}  // namespace bic
