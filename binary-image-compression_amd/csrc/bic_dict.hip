// bic_dict.hip -- the growing-dictionary tile coder of compress2_test.cpp:79-129 (variant 2) and
// compress3_test.cpp:87-149 (variant 3) on one plane.
//
// Per W x W tile in raster order: the atom of the dictionary at least Hamming distance (first among
// equals, :86-98 / :94-106), the two code lengths (:103,115 / :116,128), match or no match, and
// whether the tile joins the dictionary (variant 2: every tile that is not a match, :122-126;
// variant 3: every tile with bestd > T, whatever its mode, :143-147). The drivers never write the
// image, so the distance of every (tile, atom) pair is known up front; only the membership of the
// dictionary is serial. Tiles are resolved in blocks of B:
//
//   * k_dict_gather: every tile's W rows as left-aligned words (P), its atom window's rows (Q: the
//     drivers store the tile's INDEX pair (i, j) and read the window at PIXEL (i, j), so Q differs
//     from P unless step = W), its weight and nomatch_len; keys = (W*W, 0), |D| = 0;
//   * per block, k_dict_dist: the block's tiles against the atoms that were in the dictionary when
//     the block began. The grid is sized for the most atoms there can be (one per earlier tile) and
//     reads |D| from device memory; the host never does. A workgroup stages one chunk of atoms in
//     LDS, word-major, a wave takes one tile at a time, a lane one atom (kDictJ per tile word read);
//     the wave's least (distance, atom) goes to the tile's key with a 64-bit atomicMin;
//   * per block, k_dict_resolve: one workgroup walks the block, 64 tiles at a time. Each lane decides
//     one tile with the |D| and the keys as they stand; the tiles up to and including the first one
//     that joins are final and are written out; the new atom's distance goes into the keys of the
//     block's later tiles (strict <: it is the last atom, so it only wins when closer), 64 tiles per
//     wave; the rest decide again. One round per join, not per tile, and no barrier inside a round.
//
// Variant 3's two sample sequences (every tile but the first, :117-122) are then coded by the match
// loop's k_match_code (bic_match.hip).
#include "bic_device.h"

#include <algorithm>

namespace bic {

namespace {

constexpr uint32_t kDictTileWords = 4096;  // the distance kernel's atoms in LDS (32 KiB: four workgroups per CU)
constexpr int kDictJ = 4;                  // atoms per lane per tile word read
constexpr uint32_t kDictGroup = 32;        // tiles per distance workgroup (8 per wave)
constexpr uint32_t kDictMaxBlock = 1024;   // tiles per block at most; and block * roundup8(W) <= kDictBlockWords
constexpr uint32_t kDictBlockWords = 4096; // the resolve kernel's P and Q images (32 KiB each)
constexpr uint32_t kDictAutoBlock = 256;

__host__ __device__ inline uint32_t dict_chunk_atoms(uint32_t W) {
  const uint32_t a = kDictTileWords / W / 64 * 64;
  return a < 64 ? 64 : a > 512 ? 512 : a;  // (W <= 64: 64 atoms of W words fit)
}

__global__ __launch_bounds__(256) void k_dict_gather(DictArgs a, uint32_t ntiles, bool own_q) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= ntiles) return;
  const FlatImage img{a.I, a.rows, a.used, a.wpr};
  const uint32_t W = a.W, ti = t / a.nx, tj = t - ti * a.nx;
  const uint64_t topW = W >= 64 ? ~0ull : ~(~0ull >> W);
  uint32_t w = 0;
  for (uint32_t r = 0; r < W; ++r) {
    const uint64_t p = img.window(ti * W + r, tj * W) & topW;
    a.P[(uint64_t)t * W + r] = p;
    w += (uint32_t)__popcll(p);
  }
  if (own_q)
    for (uint32_t r = 0; r < W; ++r) a.Q[(uint64_t)t * W + r] = img.window(ti * a.step + r, tj * a.step) & topW;
  a.wt[t] = w;
  a.nml[t] = (uint64_t)((1.0 + a.enuml[w]) + a.h);  // :103 / :116, the driver's order of additions
  a.keys[t] = (unsigned long long)(W * W) << 32;      // bestk = 0, bestd = W*W (:84 / :92)
  if (t == 0) a.state[0] = a.state[1] = a.state[2] = 0;
}

__global__ __launch_bounds__(256) void k_dict_dist(DictArgs a, uint32_t t0, uint32_t bn, uint32_t A) {
  __shared__ uint64_t tile[kDictTileWords];
  __shared__ uint64_t erows[4][64];
  const uint32_t nD = (uint32_t)a.state[0], k0 = blockIdx.x * A;
  if (k0 >= nD) return;
  const uint32_t cnt = min(A, nD - k0), W = a.W, lane = lane_id(), wave = wave_id();
  for (uint32_t idx = threadIdx.x; idx < cnt * W; idx += 256) {
    const uint32_t k = idx / W, w = idx - k * W;
    tile[w * A + k] = a.Q[(uint64_t)a.dict_tiles[k0 + k] * W + w];
  }
  __syncthreads();
  uint64_t* erow = erows[wave];
  const uint32_t M = W * W;
  const uint32_t i_hi = min(bn, (blockIdx.y + 1) * kDictGroup);
  for (uint32_t i = blockIdx.y * kDictGroup + wave; i < i_hi; i += 4) {  // wave-uniform
    const uint32_t t = t0 + i;
    if (lane < W) erow[lane] = a.P[(uint64_t)t * W + lane];
    __builtin_amdgcn_wave_barrier();
    uint32_t bd = M, bk = 0;
    for (uint32_t base = 0; base < cnt; base += 64 * kDictJ) {
      uint32_t d[kDictJ];
#pragma unroll
      for (int j = 0; j < kDictJ; ++j) d[j] = 0;
      for (uint32_t w = 0; w < W; ++w) {
        const uint64_t e = erow[w];
        const uint64_t* col = tile + w * A + base + lane;
#pragma unroll
        for (int j = 0; j < kDictJ; ++j)  // (wave-uniform guard; A is a multiple of 64, so base + 64 j + lane < A)
          if (base + 64 * j < cnt) d[j] += (uint32_t)__popcll(e ^ col[64 * j]);
      }
#pragma unroll
      for (int j = 0; j < kDictJ; ++j) {  // a lane's atoms in increasing order: strict < keeps the first
        const uint32_t k = base + 64 * j + lane;
        if (k < cnt && d[j] < bd) {
          bd = d[j];
          bk = k0 + k;
        }
      }
    }
    const unsigned long long key = wave_min_u64(((unsigned long long)bd << 32) | bk);
    if (lane == 0 && (uint32_t)(key >> 32) < M) atomicMin(&a.keys[t], key);
    __builtin_amdgcn_wave_barrier();  // the next tile's rows overwrite erow
  }
}

__device__ __forceinline__ uint32_t ceil_log2(uint32_t n) { return n <= 1 ? 0 : 32 - (uint32_t)__clz(n - 1); }

__global__ __launch_bounds__(256) void k_dict_resolve(DictArgs a, uint32_t t0, uint32_t bn) {
  // word-major, rows padded with zero words to a multiple of 8: row r of tile j at [r * bn + j]
  __shared__ uint64_t Pl[kDictBlockWords], Ql[kDictBlockWords];
  __shared__ double E[64 * 64 + 1];
  __shared__ unsigned long long keys[kDictMaxBlock];
  __shared__ uint64_t nml[kDictMaxBlock];
  __shared__ uint32_t wts[kDictMaxBlock];
  const uint32_t W = a.W, M = W * W, Wp = (W + 7) & ~7u;
  for (uint32_t idx = threadIdx.x; idx < bn * Wp; idx += 256) {
    const uint32_t r = idx / bn, j = idx - r * bn;
    Pl[idx] = r < W ? a.P[(uint64_t)(t0 + j) * W + r] : 0ull;
    Ql[idx] = r < W ? a.Q[(uint64_t)(t0 + j) * W + r] : 0ull;
  }
  for (uint32_t e = threadIdx.x; e <= M; e += 256) E[e] = a.enuml[e];
  for (uint32_t j = threadIdx.x; j < bn; j += 256) {
    keys[j] = a.keys[t0 + j];
    nml[j] = a.nml[t0 + j];
    wts[j] = a.wt[t0 + j];
  }
  __syncthreads();
  // Every wave decides the same 64 tiles from the same values (its own register copy of their keys, the
  // read-only tables), so all four agree on which tile joins next without exchanging anything; wave 0
  // alone writes the results. On a join every wave updates its copy of the current 64 keys, and the keys
  // of the later tiles, in LDS, are split over the waves (64 tiles each): no barrier inside a round, one
  // per 64 tiles, before their keys are read.
  const uint32_t lane = lane_id(), wave = wave_id();
  auto closer = [&](uint32_t jj, uint32_t i, unsigned long long kk, uint32_t atom) {  // tile jj against Q_i
    const uint32_t cur = (uint32_t)(kk >> 32);
    if (!cur) return kk;  // (a perfect match stays: the search stops at the first distance 0)
    uint32_t d = 0;
    for (uint32_t r = 0; r < Wp; r += 8) {  // eight rows' loads in flight
      uint64_t x[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) x[u] = Pl[(r + u) * bn + jj] ^ Ql[(r + u) * bn + i];
#pragma unroll
      for (int u = 0; u < 8; ++u) d += (uint32_t)__popcll(x[u]);
    }
    return d < cur ? ((unsigned long long)d << 32) | atom : kk;  // strict <: the last atom wins only when closer
  };
  uint32_t nD = uni_u32((uint32_t)a.state[0]);
  uint64_t L = 0, matches = 0;  // this lane's share (wave 0)
  for (uint32_t c0 = 0; c0 < bn; c0 += 64) {
    const uint32_t j = c0 + lane, t = t0 + j;
    const bool valid = j < bn;
    const uint32_t w = valid ? wts[j] : 0;
    const uint64_t nm = valid ? nml[j] : 0;
    if (c0) __syncthreads();  // the other waves' updates of these keys
    unsigned long long key = valid ? keys[j] : 0ull;
    uint32_t start = 0;
    while (start < 64) {  // one round per join (the same in every wave)
      const uint32_t bd = (uint32_t)(key >> 32), bk = (uint32_t)key;
      bool match = false, join = true;  // an empty dictionary: push, no match (:104-109 / :117-122)
      uint64_t ml = 0;
      if (nD) {
        ml = (uint64_t)(((1.0 + (double)ceil_log2(nD)) + E[bd]) + a.h);  // :115 / :128
        match = nm > ml;                                                  // :118 / :131
        join = a.variant == 2 ? !match : bd > a.T;                        // :122-126 / :143
      }
      const bool pending = valid && lane >= start;
      const uint64_t jb = __builtin_amdgcn_ballot_w64(pending && join);
      const uint32_t first = jb ? (uint32_t)__builtin_ctzll(jb) : 64u;
      if (wave == 0 && pending && lane <= first) {  // final: no earlier tile of the block joins any more
        a.bestk[t] = bk;
        a.bestd[t] = bd;
        a.dsize[t] = nD;
        a.weights[t] = match ? bd : w;
        a.modes[t] = match ? 'x' : 'o';
        a.joined[t] = lane == first ? 1 : 0;
        const uint64_t len = match ? ml : nm;
        a.lens[t] = (uint32_t)len;
        L += len;
        matches += match ? 1 : 0;
      }
      if (first == 64) break;
      const uint32_t i = c0 + first;  // tile t0 + i becomes atom nD
      if (threadIdx.x == 0) a.dict_tiles[nD] = t0 + i;
      if (valid && lane > first) key = closer(j, i, key, nD);
      for (uint32_t q0 = c0 + 64 * (1 + wave); q0 < bn; q0 += 256) {
        const uint32_t jj = q0 + lane;
        if (jj < bn) keys[jj] = closer(jj, i, keys[jj], nD);
      }
      ++nD;
      start = first + 1;
    }
  }
  if (wave != 0) return;
#pragma unroll
  for (int dd = 32; dd >= 1; dd >>= 1) {
    L += shfl_u64(L, (int)lane ^ dd);
    matches += shfl_u64(matches, (int)lane ^ dd);
  }
  if (lane == 0) {
    a.state[0] = nD;
    a.state[1] += L;
    a.state[2] += matches;
  }
}

// stats: [0] matches, [1] / [2] bits of golomb_match / golomb_nomatch (variant 3: k_match_code's), [3] L,
// [4] the final |D|
__global__ void k_dict_finish(const uint64_t* state, uint32_t variant, uint64_t* stats) {
  stats[0] = state[2];
  if (variant == 2) stats[1] = stats[2] = 0;
  stats[3] = state[1];
  stats[4] = state[0];
}

size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

uint32_t dict_block_tiles(uint32_t W, uint32_t code) {
  const uint32_t fit = std::min(kDictMaxBlock, kDictBlockWords / ((W + 7) / 8 * 8));  // (k_dict_resolve's padded rows)
  return std::min(code ? code : kDictAutoBlock, fit);
}

size_t dict_scratch_bytes(size_t ntiles, uint32_t W) {
  return 256 + up256(ntiles * 8) * 2 + up256(ntiles * W * 8) * 2 + up256(ntiles * 4) * 7 + up256(ntiles) * 2 + 256;
}

void dict_carve(DictArgs& a, void* scratch) {
  const size_t nt = (size_t)a.nx * a.ny;
  char* c = static_cast<char*>(scratch);
  auto take = [&](size_t bytes) {
    char* p = c;
    c += up256(bytes);
    return p;
  };
  a.state = reinterpret_cast<uint64_t*>(take(256));
  a.keys = reinterpret_cast<unsigned long long*>(take(nt * 8));
  a.nml = reinterpret_cast<uint64_t*>(take(nt * 8));
  a.P = reinterpret_cast<uint64_t*>(take(nt * a.W * 8));
  a.Q = a.step == a.W ? a.P : reinterpret_cast<uint64_t*>(take(nt * a.W * 8));
  a.wt = reinterpret_cast<uint32_t*>(take(nt * 4));
  a.lens = reinterpret_cast<uint32_t*>(take(nt * 4));
  uint32_t** u32s[5] = {&a.bestk, &a.bestd, &a.dsize, &a.weights, &a.dict_tiles};
  for (uint32_t** p : u32s)
    if (!*p) *p = reinterpret_cast<uint32_t*>(take(nt * 4));
  if (!a.modes) a.modes = reinterpret_cast<uint8_t*>(take(nt));
  if (!a.joined) a.joined = reinterpret_cast<uint8_t*>(take(nt));
  a.noflags = reinterpret_cast<uint32_t*>(take(256));
}

void launch_dict_gather(hipStream_t s, const DictArgs& a) {
  const uint32_t nt = a.nx * a.ny;
  k_dict_gather<<<(nt + 255) / 256, 256, 0, s>>>(a, nt, a.Q != a.P);
}

void launch_dict_dist(hipStream_t s, const DictArgs& a, uint32_t t0, uint32_t bn) {
  if (!t0) return;
  const uint32_t A = dict_chunk_atoms(a.W);
  k_dict_dist<<<dim3((t0 + A - 1) / A, (bn + kDictGroup - 1) / kDictGroup), 256, 0, s>>>(a, t0, bn, A);
}

void launch_dict_resolve(hipStream_t s, const DictArgs& a, uint32_t t0, uint32_t bn) {
  k_dict_resolve<<<1, 256, 0, s>>>(a, t0, bn);
}

void launch_dict_finish(hipStream_t s, const DictArgs& a, uint64_t* stats) {
  k_dict_finish<<<1, 1, 0, s>>>(a.state, a.variant, stats);
}

}  // namespace bic
