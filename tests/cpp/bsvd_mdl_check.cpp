// bsvd_mdl_check.cpp -- include/bsvd.h's model code length and MDL model-order searches through the C++ bridge
// (tests/test_gpu_bsvd_mdl_host.py):
//   bsvd_mdl_check MODE first.pbm D.pbm A.pbm outE.pbm outD.pbm outA.pbm
// MODE is a search on the data X = first.pbm from the model (D, A) -- forward, backward, full_centroids
// (initialize_model = initialize_model_random_centroids first), backward_alter1 (learn_model_inner =
// learn_model_alter1 for the search, then set back, and the search runs again on a second copy of the inputs:
// "after=<its result>"), setup_backward (learn_model_setup(0, 0, 0, 5, 0), then learn_model) -- or codelength
// (first.pbm is the residual E; nothing is written). The default device runs it. E is written back, D and A at
// their new sizes unless the result is the empty model; prints "atoms=<rows of D>" and "result=<return value>"
// after the search's own lines.
#include <cstdio>
#include <cstring>
#include <iostream>
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
  if (learn_model != learn_model_traditional || learn_model_inner != learn_model_traditional ||
      initialize_model != initialize_model_neighbor || update_dictionary != update_dictionary_steepest) {
    std::fprintf(stderr, "the globals do not have their documented defaults\n");
    return 1;
  }
  if (mode == "codelength") {
    std::cout << "result=" << model_codelength(F, D, A) << std::endl;
    binary_matrix none;
    std::cout << "empty=" << model_codelength(F, none, none) << std::endl;
    return 0;
  }
  binary_matrix E;
  E.allocate(F.get_rows(), F.get_cols());
  idx_t result = 0;
  if (mode == "forward") {
    result = learn_model_mdl_forward_selection(F, E, D, A);
  } else if (mode == "backward") {
    result = learn_model_mdl_backward_selection(F, E, D, A);
  } else if (mode == "full_centroids") {
    initialize_model = initialize_model_random_centroids;
    result = learn_model_mdl_full_search(F, E, D, A);
  } else if (mode == "backward_alter1") {
    binary_matrix E2, D2, A2;
    if (!load(argv[3], D2) || !load(argv[4], A2)) return 1;
    E2.allocate(F.get_rows(), F.get_cols());
    learn_model_inner = learn_model_alter1;
    result = learn_model_mdl_backward_selection(F, E, D, A);
    learn_model_inner = learn_model_traditional;
    const idx_t after = learn_model_mdl_backward_selection(F, E2, D2, A2);
    std::cout << "after=" << after << std::endl;
  } else if (mode == "setup_backward") {
    learn_model_setup(0, 0, 0, 5, 0);
    if (learn_model != learn_model_mdl_backward_selection || learn_model_inner != learn_model_traditional) return 1;
    result = learn_model(F, E, D, A);
  } else {
    std::fprintf(stderr, "unknown mode %s\n", mode.c_str());
    return 2;
  }
  std::cout << "atoms=" << D.get_rows() << std::endl << "result=" << result << std::endl;
  if (!store(argv[5], E)) return 1;
  if (D.get_rows() && (!store(argv[6], D) || !store(argv[7], A))) {
    std::fprintf(stderr, "cannot write the outputs\n");
    return 1;
  }
  return 0;
}
