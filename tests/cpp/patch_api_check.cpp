// patch_api_check.cpp -- the image mode through the C++ bridge (libbicpp.so; tests/test_gpu_patch_host.py):
//   patch_api_check I.pbm W p dirty outdir
// reads the image, sets its pad bits when dirty = 1, and writes into outdir, each result twice:
//   X_dev.bin / X_host.bin   bic::Device::patches and the driver's loop over the host binary_matrix (raw words)
//   R_dev.pbm / R_host.pbm   bic::Device::unpatch of those samples into an all-ones image, and the host loop
//   M_dev.pbm / M_host.pbm   bic::Device::mosaic of the samples and render_mosaic's file
//   one_{X,E,D,A}.bin, one_R.pbm   bic::Device::bsvd_learn_image (neighbour rule, traditional learner, steepest rule)
//   sep_{X,E,D,A}.bin, sep_R.pbm   patches, E = X, bsvd_initialize, bsvd_learn and unpatch called one by one
// and prints the iteration counts and generator states of the two runs.
#include <cstdlib>
#include <cstring>

#include "bic.h"
#include "bic_gpu.h"
#include "patch_host_loops.h"
#include "util.h"

#define CHECK(x)                                                            \
  do {                                                                      \
    const int rc_ = (x);                                                    \
    if (rc_) {                                                              \
      std::fprintf(stderr, "%s: %s\n", #x, bic_strerror(rc_));              \
      return 1;                                                             \
    }                                                                       \
  } while (0)
#define WRITE(x)                                    \
  do {                                              \
    if (!(x)) {                                     \
      std::fprintf(stderr, "cannot write: %s\n", #x); \
      return 1;                                     \
    }                                               \
  } while (0)

int main(int argc, char** argv) {
  if (argc < 6) {
    std::fprintf(stderr, "usage: %s I.pbm W p dirty outdir\n", argv[0]);
    return 2;
  }
  binary_matrix I;
  if (!load_pbm(argv[1], I)) {
    std::fprintf(stderr, "cannot read the input\n");
    return 1;
  }
  const unsigned W = (unsigned)std::strtoul(argv[2], nullptr, 10);
  const idx_t p = (idx_t)std::strtoul(argv[3], nullptr, 10);
  if (std::atoi(argv[4])) dirty_padding(I);
  const std::string out = std::string(argv[5]) + "/";
  bic::Device& dev = bic::default_device();

  binary_matrix X, Xh;
  CHECK(dev.patches(I, W, X));
  host_patches(I, W, Xh);
  WRITE(store_words(out + "X_dev.bin", X) && store_words(out + "X_host.bin", Xh));

  binary_matrix R(I.get_rows(), I.get_cols()), Rh(I.get_rows(), I.get_cols());
  R.set();
  Rh.set();
  CHECK(dev.unpatch(X, W, R));
  host_unpatch(Xh, W, Rh);
  WRITE(store_pbm(out + "R_dev.pbm", R) && store_pbm(out + "R_host.pbm", Rh));

  binary_matrix M;
  CHECK(dev.mosaic(X, M));
  WRITE(store_pbm(out + "M_dev.pbm", M));
  render_mosaic(Xh, (out + "M_host.pbm").c_str());

  uint64_t st1 = 0, st2 = 0;
  bic_bsvd_rng_seed(34503498, &st1);
  st2 = st1;
  idx_t it1 = 0, it2 = 0;
  binary_matrix X1, E1, D1, A1, R1;
  CHECK(dev.bsvd_learn_image(BIC_BSVD_MI_NEIGHBOR, BIC_BSVD_LM_TRADITIONAL, BIC_BSVD_DU_STEEPEST, I, W, p, X1, E1, D1, A1,
                             &st1, 0, &it1, &R1));
  binary_matrix X2;
  CHECK(dev.patches(I, W, X2));
  binary_matrix E2(X2), D2(p, X2.get_cols()), A2(X2.get_rows(), p), R2(I.get_rows(), I.get_cols());
  CHECK(dev.bsvd_initialize(BIC_BSVD_MI_NEIGHBOR, E2, D2, A2, &st2));
  CHECK(dev.bsvd_learn(BIC_BSVD_LM_TRADITIONAL, BIC_BSVD_DU_STEEPEST, X2, E2, D2, A2, 0, &it2));
  CHECK(dev.unpatch(E2, W, R2));
  WRITE(store_words(out + "one_X.bin", X1) && store_words(out + "one_E.bin", E1) && store_words(out + "one_D.bin", D1) &&
        store_words(out + "one_A.bin", A1) && store_pbm(out + "one_R.pbm", R1));
  WRITE(store_words(out + "sep_X.bin", X2) && store_words(out + "sep_E.bin", E2) && store_words(out + "sep_D.bin", D2) &&
        store_words(out + "sep_A.bin", A2) && store_pbm(out + "sep_R.pbm", R2));
  std::printf("iters=%lu,%lu states=%llu,%llu n=%lu m=%lu\n", (unsigned long)it1, (unsigned long)it2,
              (unsigned long long)st1, (unsigned long long)st2, (unsigned long)X1.get_rows(),
              (unsigned long)X1.get_cols());
  return 0;
}
