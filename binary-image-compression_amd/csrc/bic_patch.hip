// bic_patch.hip -- the image mode of the dictionary-learning driver on the device (include/bic.h "image mode"):
//
//  * bsvd_test.cpp:89-97 the W x W tiles of a plane as the rows of X (copy_submatrix_to + copy_vectorized_to +
//    set_row), read with get_submatrix's flat word indexing (binmat.cpp:267-298);
//  * bsvd_test.cpp:130-139 the rows of X put back as tiles (copy_row_to + set_vectorized + set_submatrix);
//  * util.cpp:53-82 render_mosaic's image: the rows of a matrix as w x w tiles on a grid with a one-pixel gutter.
//
// Plane layout as everywhere: rows of 64-bit words, column j at MSB >> (j % 64). In all three kernels one thread
// forms one OUTPUT word from bit fields of the source (a field: a run of bits that is contiguous in both; at most
// two source words per field, joined by a funnel shift), so nothing is read back, nothing is added atomically and
// the stores of a wave run along the output row. The gather and the scatter stage what a workgroup's output words
// read through LDS, in pieces sized by the host to fit kPatchLds words whatever W is. A workgroup walks its work
// items in a grid-stride loop: one launch per call, no workgroup waits for another.
#include "bic_internal.h"

#include <algorithm>

namespace bic {

namespace {

constexpr uint32_t kPatchBlock = 256;
constexpr uint32_t kPatchLds = 4096;        // words of LDS a workgroup stages into (32 KiB)
constexpr uint32_t kPatchWords = 512;       // output words a work item aims at
constexpr uint32_t kPatchMaxGrid = 1u << 16;

// len (1 .. 64) bits starting at bit `bit` of the word run w, left-aligned, the rest 0. w[1] is read only when
// the field crosses into it.
__device__ __forceinline__ uint64_t field(const uint64_t* w, uint32_t bit, uint32_t len) {
  const uint32_t sh = bit & 63u;
  w += bit >> 6;
  uint64_t v = w[0] << sh;
  if (sh + len > 64) v |= w[1] >> (64 - sh);
  return len < 64 ? v & ~(~0ull >> len) : v;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// Gather. A work item is (tile row ti, tiles tj0 .. tj0 + tn - 1, words q0 .. q0 + qn - 1 of their rows of X). It
// stages the image rows those words read (rlo .. rhi of the tile) over the columns of its tiles: LDS word (r, k)
// is FLAT word (ti W + rlo + r) used + w0 + k of the plane, 0 past the last row, so a tile that runs past the right
// edge finds the next row's first words where the flat indexing puts them.
// ------------------------------------------------------------------------------------------------
struct GatherGeom {
  uint32_t rows, used, wpr, W, nx, ny, xw, x_wpr;
  uint32_t T, Q, nct, ncq;  // tiles and words per work item, and how many of each a tile row / a row of X has
};

__global__ __launch_bounds__(kPatchBlock) void k_patches_gather(const uint64_t* __restrict__ I, GatherGeom g,
                                                                uint64_t* __restrict__ X) {
  __shared__ uint64_t lds[kPatchLds];
  const uint32_t W = g.W, m = W * W;
  const uint64_t per_row = (uint64_t)g.nct * g.ncq, items = per_row * g.ny;
  for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint32_t ti = (uint32_t)(item / per_row), rem = (uint32_t)(item - (uint64_t)ti * per_row);
    const uint32_t ct = rem / g.ncq, cq = rem - ct * g.ncq;
    const uint32_t tj0 = ct * g.T, tn = min(g.T, g.nx - tj0);
    const uint32_t q0 = cq * g.Q, qn = min(g.Q, g.xw - q0);
    const uint32_t rlo = (64u * q0) / W, rhi = min(W - 1u, (64u * (q0 + qn) - 1u) / W), nr = rhi - rlo + 1u;
    const uint32_t w0 = (tj0 * W) >> 6, cw = (((tj0 + tn) * W + 63u) >> 6) - w0 + 1u;
    for (uint32_t idx = threadIdx.x; idx < nr * cw; idx += kPatchBlock) {
      const uint32_t r = idx / cw, t = w0 + (idx - r * cw), dr = t / g.used, wk = t - dr * g.used;
      const uint64_t R = (uint64_t)ti * W + rlo + r + dr;
      lds[idx] = R < g.rows ? I[R * g.wpr + wk] : 0;
    }
    __syncthreads();
    const uint64_t li0 = (uint64_t)ti * g.nx + tj0;
    for (uint32_t o = threadIdx.x; o < tn * qn; o += kPatchBlock) {
      const uint32_t t = o / qn, q = q0 + (o - t * qn);
      const uint32_t bend = min(64u * q + 64u, m), col0 = (tj0 + t) * W - (w0 << 6);
      uint32_t b = 64u * q, r = b / W, c = b - r * W, pos = 0;
      uint64_t out = 0;
      while (b < bend) {
        const uint32_t len = min(W - c, bend - b);
        out |= field(lds + (r - rlo) * cw, col0 + c, len) >> pos;
        pos += len;
        b += len;
        c = 0;
        ++r;
      }
      X[(li0 + t) * g.x_wpr + q] = out;
    }
    __syncthreads();
  }
}

// The words a staged image row needs for T tiles (the first tile may start anywhere in its word, and a field may
// read one word past its own), and the image rows Q words of X can touch
inline uint32_t gather_cw(uint32_t T, uint32_t W) { return (uint32_t)(((uint64_t)T * W) >> 6) + 3u; }
inline uint32_t gather_nr(uint32_t Q, uint32_t W) { return std::min<uint64_t>(W, (64ull * Q) / W + 2u); }

void launch_patches_gather(hipStream_t s, const uint64_t* plane, uint32_t rows, uint32_t cols, uint32_t wpr, uint32_t W,
                           uint64_t* X, uint32_t x_wpr) {
  GatherGeom g;
  g.rows = rows;
  g.used = (cols + 63) / 64;
  g.wpr = wpr;
  g.W = W;
  g.nx = (cols + W - 1) / W;
  g.ny = (rows + W - 1) / W;
  g.xw = (W * W + 63) / 64;
  g.x_wpr = x_wpr;
  // whole rows of X while the W image rows of one tile fit, as many tiles as fit and as kPatchWords asks for;
  // otherwise one tile, and as many of its words as their image rows allow
  g.T = 1;
  g.Q = g.xw;
  if (W * gather_cw(1, W) <= kPatchLds) {
    g.T = std::min(g.nx, std::max(1u, kPatchWords / g.xw));
    while (g.T > 1 && W * gather_cw(g.T, W) > kPatchLds) g.T = (g.T + 1) / 2;
  } else {
    while (gather_nr(g.Q, W) * gather_cw(1, W) > kPatchLds) g.Q = (g.Q + 1) / 2;
  }
  g.nct = (g.nx + g.T - 1) / g.T;
  g.ncq = (g.xw + g.Q - 1) / g.Q;
  const uint64_t items = (uint64_t)g.nct * g.ncq * g.ny;
  k_patches_gather<<<(uint32_t)std::min<uint64_t>(items, kPatchMaxGrid), kPatchBlock, 0, s>>>(plane, g, X);
}

// ------------------------------------------------------------------------------------------------
// Scatter. A work item is (tile row ti, words wj0 .. wj0 + wn - 1 of the plane's rows, rows r0 .. r0 + rn - 1 of the
// tile row): whole output words, so tiles that share a word meet in one thread. It stages, for every tile its
// columns touch, the words of that tile's row of X that hold tile rows r0 .. r0 + rn - 1.
// ------------------------------------------------------------------------------------------------
struct ScatterGeom {
  uint32_t rows, cols, used, wpr, W, nx, ny, xw, x_wpr;
  uint32_t C, R, ncc, ncr;  // plane words and tile rows per work item, and how many of each a tile row has
};

__global__ __launch_bounds__(kPatchBlock) void k_patches_scatter(const uint64_t* __restrict__ X, ScatterGeom g,
                                                                 uint64_t* __restrict__ P) {
  __shared__ uint64_t lds[kPatchLds];
  const uint32_t W = g.W;
  const uint64_t per_row = (uint64_t)g.ncc * g.ncr, items = per_row * g.ny;
  for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint32_t ti = (uint32_t)(item / per_row), rem = (uint32_t)(item - (uint64_t)ti * per_row);
    const uint32_t cc = rem / g.ncr, cr = rem - cc * g.ncr;
    const uint32_t wj0 = cc * g.C, wn = min(g.C, g.used - wj0);
    const uint32_t r0 = cr * g.R;
    const uint64_t i0 = (uint64_t)ti * W + r0;
    if (i0 >= g.rows) continue;  // (the whole workgroup: the tile rows past the image are dropped)
    const uint32_t rn = (uint32_t)min((uint64_t)min(g.R, W - r0), g.rows - i0);
    const uint32_t x1 = min(64u * (wj0 + wn), g.cols);
    const uint32_t tja = (64u * wj0) / W, tn = (x1 - 1u) / W - tja + 1u;
    const uint32_t s0 = (r0 * W) >> 6, sn = (((r0 + rn) * W + 63u) >> 6) - s0 + 1u;
    const uint64_t li0 = (uint64_t)ti * g.nx + tja;
    for (uint32_t idx = threadIdx.x; idx < tn * sn; idx += kPatchBlock) {
      const uint32_t t = idx / sn, wq = s0 + (idx - t * sn);
      lds[idx] = wq < g.xw ? X[(li0 + t) * g.x_wpr + wq] : 0;
    }
    __syncthreads();
    for (uint32_t o = threadIdx.x; o < rn * wn; o += kPatchBlock) {
      const uint32_t r = o / wn, wj = wj0 + (o - r * wn);
      const uint32_t xend = min(64u * wj + 64u, g.cols), row0 = (r0 + r) * W - (s0 << 6);
      uint32_t x = 64u * wj, tj = x / W, c = x - tj * W, pos = 0;
      uint64_t out = 0;
      while (x < xend) {
        const uint32_t len = min(W - c, xend - x);
        out |= field(lds + (tj - tja) * sn, row0 + c, len) >> pos;
        pos += len;
        x += len;
        c = 0;
        ++tj;
      }
      P[(i0 + r) * g.wpr + wj] = out;
    }
    __syncthreads();
  }
}

// The tiles C plane words can touch, and the words of a row of X that R tile rows need (as gather_cw)
inline uint32_t scatter_tn(uint32_t C, uint32_t W, uint32_t nx) {
  return (uint32_t)std::min<uint64_t>(nx, (64ull * C + W - 2u) / W + 1u);
}
inline uint32_t scatter_sn(uint32_t R, uint32_t W) { return (uint32_t)(((uint64_t)R * W) >> 6) + 3u; }

void launch_patches_scatter(hipStream_t s, const uint64_t* X, uint32_t x_wpr, uint32_t W, uint64_t* plane,
                            uint32_t rows, uint32_t cols, uint32_t wpr) {
  ScatterGeom g;
  g.rows = rows;
  g.cols = cols;
  g.used = (cols + 63) / 64;
  g.wpr = wpr;
  g.W = W;
  g.nx = (cols + W - 1) / W;
  g.ny = (rows + W - 1) / W;
  g.xw = (W * W + 63) / 64;
  g.x_wpr = x_wpr;
  // whole tile rows and as many plane words as kPatchWords asks for while their tiles' rows of X fit; fewer
  // words, and from one word on fewer tile rows, where they do not
  g.R = W;
  g.C = std::min(g.used, std::max(1u, kPatchWords / W));
  while (g.C > 1 && scatter_tn(g.C, W, g.nx) * scatter_sn(W, W) > kPatchLds) g.C = (g.C + 1) / 2;
  while (scatter_tn(g.C, W, g.nx) * scatter_sn(g.R, W) > kPatchLds) g.R = (g.R + 1) / 2;
  g.ncc = (g.used + g.C - 1) / g.C;
  g.ncr = (W + g.R - 1) / g.R;
  const uint64_t items = (uint64_t)g.ncc * g.ncr * g.ny;
  k_patches_scatter<<<(uint32_t)std::min<uint64_t>(items, kPatchMaxGrid), kPatchBlock, 0, s>>>(X, g, plane);
}

// ------------------------------------------------------------------------------------------------
// Mosaic. Image row y = gw i + r, columns gw j + c: tile (i, j) is row i gn + j of D as w rows of w bits; r = w
// and c = w are the gutter. An atom is read by at most two rows of output words per tile row, so D is read where
// it lies.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPatchBlock) void k_mosaic(const uint64_t* __restrict__ D, uint32_t n, uint32_t d_wpr,
                                                        uint32_t w, uint32_t gn, uint32_t icols, uint32_t iw,
                                                        uint64_t words, uint64_t* __restrict__ img, uint32_t i_wpr) {
  const uint32_t gw = w + 1u;
  for (uint64_t o = (uint64_t)blockIdx.x * kPatchBlock + threadIdx.x; o < words; o += (uint64_t)gridDim.x * kPatchBlock) {
    const uint32_t y = (uint32_t)(o / iw), wq = (uint32_t)(o - (uint64_t)y * iw);
    const uint32_t i = y / gw, r = y - i * gw;
    uint64_t out = 0;
    if (r < w) {
      const uint32_t xend = min(64u * wq + 64u, icols);
      uint32_t x = 64u * wq, j = x / gw, c = x - j * gw;
      while (x < xend) {
        if (c == w) {  // the gutter column
          ++x;
          c = 0;
          ++j;
          continue;
        }
        const uint32_t len = min(min(w - c, xend - x), 64u), atom = i * gn + j;
        if (atom < n) out |= field(D + (uint64_t)atom * d_wpr, r * w + c, len) >> (x - 64u * wq);
        x += len;
        c += len;
      }
    }
    img[(uint64_t)y * i_wpr + wq] = out;
  }
}

void launch_mosaic(hipStream_t s, const uint64_t* D, uint32_t n, uint32_t d_wpr, uint32_t w, uint32_t gn, uint32_t irows,
                   uint32_t icols, uint64_t* image, uint32_t i_wpr) {
  const uint32_t iw = (icols + 63) / 64;
  const uint64_t words = (uint64_t)irows * iw;
  const uint64_t blocks = (words + kPatchBlock - 1) / kPatchBlock;
  k_mosaic<<<(uint32_t)std::min<uint64_t>(blocks, kPatchMaxGrid), kPatchBlock, 0, s>>>(D, n, d_wpr, w, gn, icols, iw,
                                                                                      words, image, i_wpr);
}

}  // namespace bic
