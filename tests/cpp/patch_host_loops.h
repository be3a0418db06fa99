// patch_host_loops.h -- the image-mode loops of the dictionary-learning driver over the host binary_matrix, as
// bsvd_test.cpp:78-100 and :126-139 write them, and small file helpers (patch_host_check.cpp, patch_api_check.cpp).
#pragma once
#include <cstdio>
#include <string>

#include "binmat.h"
#include "pbm.h"

// bsvd_test.cpp:78-100: the W x W tiles of I as the rows of X
inline void host_patches(const binary_matrix& I, idx_t W, binary_matrix& X) {
  const idx_t rows = I.get_rows(), cols = I.get_cols();
  const idx_t Ny = (W - 1 + rows) / W, Nx = (W - 1 + cols) / W;
  X.allocate(Nx * Ny, W * W);
  binary_matrix tile(W, W), vec(1, W * W);
  for (idx_t t = 0; t < Nx * Ny; ++t) {
    const idx_t i0 = (t / Nx) * W, j0 = (t % Nx) * W;
    I.copy_submatrix_to(i0, i0 + W, j0, j0 + W, tile);
    tile.copy_vectorized_to(vec);
    X.set_row(t, vec);
  }
  tile.destroy();
  vec.destroy();
}

// bsvd_test.cpp:126-139: the rows of E put back as the tiles of I
inline void host_unpatch(const binary_matrix& E, idx_t W, binary_matrix& I) {
  const idx_t rows = I.get_rows(), cols = I.get_cols();
  const idx_t Ny = (W - 1 + rows) / W, Nx = (W - 1 + cols) / W;
  binary_matrix tile(W, W), vec(1, W * W);
  for (idx_t t = 0; t < Nx * Ny; ++t) {
    E.copy_row_to(t, vec);
    tile.set_vectorized(vec);
    I.set_submatrix((t / Nx) * W, (t % Nx) * W, tile);
  }
  tile.destroy();
  vec.destroy();
}

inline bool load_pbm(const char* path, binary_matrix& M) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  idx_t rows = 0, cols = 0;
  bool ok = read_pbm_header(f, rows, cols) == PBM_OK;
  if (ok) {
    M.allocate(rows, cols);
    ok = read_pbm_data(f, M) == PBM_OK;
  }
  std::fclose(f);
  return ok;
}

inline bool store_pbm(const std::string& path, binary_matrix& M) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = write_pbm(M, f) == PBM_OK;
  return std::fclose(f) == 0 && ok;
}

// every word of M as it lies in memory (native byte order), pad bits included
inline bool store_words(const std::string& path, const binary_matrix& M) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const size_t n = M.get_rows() * M.get_blocks_per_row();
  const bool ok = std::fwrite(M.raw_blocks(), sizeof(block_t), n, f) == n;
  return std::fclose(f) == 0 && ok;
}

// read_pbm_data clears the pad bits of every row: set them all, so that a read of a pad column shows
inline void dirty_padding(binary_matrix& M) {
  const idx_t bpr = M.get_blocks_per_row(), used = M.get_cols() % BITS_PER_BLOCK;
  if (!used) return;
  for (idx_t i = 0; i < M.get_rows(); ++i) M.raw_blocks()[i * bpr + bpr - 1] |= ONES >> used;
}
