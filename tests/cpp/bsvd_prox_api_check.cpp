// bsvd_prox_api_check.cpp -- include/bsvd.h's second dictionary rule through the C++ bridge
// (tests/test_gpu_bsvd_prox_host.py):
//   bsvd_prox_api_check [omp] E.pbm D.pbm A.pbm outE.pbm outD.pbm outA.pbm
// reads the residual E (n x m), the atoms D (p x m) and the coefficients A (n x p), runs
// update_dictionary_proximus (update_dictionary_proximus_omp with "omp") on the default device and
// writes E, D and A back; prints "changed=<n>".
#include <cstdio>
#include <cstring>

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
  const bool omp = argc == 8 && !std::strcmp(argv[1], "omp");
  if (argc != 7 && !omp) {
    std::fprintf(stderr, "usage: %s [omp] E.pbm D.pbm A.pbm outE.pbm outD.pbm outA.pbm\n", argv[0]);
    return 2;
  }
  char** a = argv + (omp ? 2 : 1);
  binary_matrix E, D, A;
  if (!load(a[0], E) || !load(a[1], D) || !load(a[2], A)) {
    std::fprintf(stderr, "cannot read the inputs\n");
    return 1;
  }
  if (D.get_cols() != E.get_cols() || A.get_rows() != E.get_rows() || A.get_cols() != D.get_rows()) {
    std::fprintf(stderr, "shapes do not fit\n");
    return 1;
  }
  const idx_t changed = omp ? update_dictionary_proximus_omp(E, D, A) : update_dictionary_proximus(E, D, A);
  std::printf("changed=%lu\n", (unsigned long)changed);
  if (!store(a[3], E) || !store(a[4], D) || !store(a[5], A)) {
    std::fprintf(stderr, "cannot write the outputs\n");
    return 1;
  }
  return 0;
}
