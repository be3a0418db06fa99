// bsvd_api_check.cpp -- include/bsvd.h through the C++ bridge (tests/test_gpu_bsvd_host.py):
//   bsvd_api_check X.pbm D.pbm A.pbm outE.pbm outD.pbm outA.pbm
// reads the data X (n x m), the atoms D (p x m) and the coefficients A (n x p), runs
// learn_model_traditional on the default device and writes E, D and A; prints "iters=<n>".
#include <cstdio>

#include "bsvd.h"
#include "pbm.h"

static bool load(const char* path, binary_matrix& M) {
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

static bool store(const char* path, binary_matrix& M) {
  FILE* f = std::fopen(path, "wb");
  if (!f) return false;
  const bool ok = write_pbm(M, f) == PBM_OK;
  return std::fclose(f) == 0 && ok;
}

int main(int argc, char** argv) {
  if (argc != 7) {
    std::fprintf(stderr, "usage: %s X.pbm D.pbm A.pbm outE.pbm outD.pbm outA.pbm\n", argv[0]);
    return 2;
  }
  binary_matrix X, D, A;
  if (!load(argv[1], X) || !load(argv[2], D) || !load(argv[3], A)) {
    std::fprintf(stderr, "cannot read the inputs\n");
    return 1;
  }
  if (D.get_cols() != X.get_cols() || A.get_rows() != X.get_rows() || A.get_cols() != D.get_rows()) {
    std::fprintf(stderr, "shapes do not fit\n");
    return 1;
  }
  binary_matrix E(X.get_rows(), X.get_cols());
  const idx_t iters = learn_model_traditional(X, E, D, A);
  std::printf("iters=%lu\n", (unsigned long)iters);
  if (!store(argv[4], E) || !store(argv[5], D) || !store(argv[6], A)) {
    std::fprintf(stderr, "cannot write the outputs\n");
    return 1;
  }
  return 0;
}
