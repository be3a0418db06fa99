// bsvd_alter_check.cpp -- include/bsvd.h's role-switching learners, its update_dictionary global and its step
// functions on wide matrices, through the C++ bridge (tests/test_gpu_bsvd_alter_host.py):
//   bsvd_alter_check MODE first.pbm D.pbm A.pbm outE.pbm outD.pbm outA.pbm
// MODE is a learner -- traditional, alter1, alter3 (first.pbm is the data X, E is formed by the learner), or
// alter3_prox: update_dictionary is set to update_dictionary_proximus_omp for learn_model_alter3, then set back
// to update_dictionary_steepest, and learn_model_alter1 runs on a second copy of the inputs ("after=<its count>")
// -- or a step -- coef, steepest, proximus (first.pbm is the residual E). The default device runs it; E, D and A
// are written back; prints "result=<the function's return value>".
#include <cstdio>
#include <cstring>
#include <string>

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
  if (argc != 8) {
    std::fprintf(stderr, "usage: %s MODE first.pbm D.pbm A.pbm outE.pbm outD.pbm outA.pbm\n", argv[0]);
    return 2;
  }
  const std::string mode = argv[1];
  binary_matrix F, D, A;
  if (!load(argv[2], F) || !load(argv[3], D) || !load(argv[4], A)) {
    std::fprintf(stderr, "cannot read the inputs\n");
    return 1;
  }
  if (D.get_cols() != F.get_cols() || A.get_rows() != F.get_rows() || A.get_cols() != D.get_rows()) {
    std::fprintf(stderr, "shapes do not fit\n");
    return 1;
  }
  if (update_coefficients != update_coefficients_omp || update_dictionary != update_dictionary_steepest) {
    std::fprintf(stderr, "the globals do not have their documented defaults\n");
    return 1;
  }
  binary_matrix E;
  binary_matrix* out = &E;
  idx_t result = 0;
  if (mode == "coef" || mode == "steepest" || mode == "proximus") {
    out = &F;  // (F is the residual)
    if (mode == "coef") result = update_coefficients(F, D, A);
    else if (mode == "steepest") result = update_dictionary(F, D, A);
    else result = update_dictionary_proximus(F, D, A);
  } else {
    E.allocate(F.get_rows(), F.get_cols());
    if (mode == "traditional") {
      result = learn_model_traditional(F, E, D, A);
    } else if (mode == "alter1") {
      result = learn_model_alter1(F, E, D, A);
    } else if (mode == "alter3") {
      result = learn_model_alter3(F, E, D, A);
    } else if (mode == "alter3_prox") {
      binary_matrix E2, D2, A2;
      if (!load(argv[3], D2) || !load(argv[4], A2)) return 1;
      E2.allocate(F.get_rows(), F.get_cols());
      update_dictionary = update_dictionary_proximus_omp;
      result = learn_model_alter3(F, E, D, A);
      update_dictionary = update_dictionary_steepest;
      std::printf("after=%lu\n", (unsigned long)learn_model_alter1(F, E2, D2, A2));
    } else {
      std::fprintf(stderr, "unknown mode %s\n", mode.c_str());
      return 2;
    }
  }
  std::printf("result=%lu\n", (unsigned long)result);
  if (!store(argv[5], *out) || !store(argv[6], D) || !store(argv[7], A)) {
    std::fprintf(stderr, "cannot write the outputs\n");
    return 1;
  }
  return 0;
}
