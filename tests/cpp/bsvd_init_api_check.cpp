// bsvd_init_api_check.cpp -- include/bsvd.h's model initialisers through the C++ bridge
// (tests/test_gpu_bsvd_init_host.py; tests/test_capi_bsvd_init.py only compiles it):
//   bsvd_init_api_check E.pbm p outdir rule [rule ...]
// reads the data E (n x m) and, for the t-th rule named (neighbor, partition, centroids, xor, or default for
// whatever the initialize_model pointer holds), makes D (p x m) and A (n x p) with ones in every bit, runs the
// initialiser on the default device and writes outdir/D<t>.pbm and outdir/A<t>.pbm. All calls run in this one
// process, so the rules that draw continue one generator, seeded from random_seed.
#include <cstdio>
#include <cstdlib>
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

static bool store(const std::string& path, binary_matrix& M) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = write_pbm(M, f) == PBM_OK;
  return std::fclose(f) == 0 && ok;
}

static mi_algorithm_t rule(const char* name) {
  if (!std::strcmp(name, "neighbor")) return initialize_model_neighbor;
  if (!std::strcmp(name, "partition")) return initialize_model_partition;
  if (!std::strcmp(name, "centroids")) return initialize_model_random_centroids;
  if (!std::strcmp(name, "xor")) return initialize_model_random_centroids_xor;
  if (!std::strcmp(name, "default")) return initialize_model;
  return nullptr;
}

int main(int argc, char** argv) {
  if (argc < 5) {
    std::fprintf(stderr, "usage: %s E.pbm p outdir rule [rule ...]\n", argv[0]);
    return 2;
  }
  mi_algorithm_t* const selected = &initialize_model;  // the pointer is an object of the library
  if (*selected != initialize_model_neighbor || random_seed != 34503498) {
    std::fprintf(stderr, "unexpected defaults\n");
    return 1;
  }
  binary_matrix E;
  if (!load(argv[1], E)) {
    std::fprintf(stderr, "cannot read the input\n");
    return 1;
  }
  const idx_t p = (idx_t)std::strtoul(argv[2], nullptr, 10);
  for (int t = 0; t + 4 < argc; ++t) {
    const mi_algorithm_t f = rule(argv[4 + t]);
    if (!f) {
      std::fprintf(stderr, "unknown rule %s\n", argv[4 + t]);
      return 2;
    }
    binary_matrix D(p, E.get_cols()), A(E.get_rows(), p);
    D.set();
    A.set();
    f(E, D, A);
    const std::string base = std::string(argv[3]) + "/", idx = std::to_string(t);
    if (!store(base + "D" + idx + ".pbm", D) || !store(base + "A" + idx + ".pbm", A)) {
      std::fprintf(stderr, "cannot write the outputs\n");
      return 1;
    }
    D.destroy();
    A.destroy();
  }
  std::printf("calls=%d\n", argc - 4);
  return 0;
}
