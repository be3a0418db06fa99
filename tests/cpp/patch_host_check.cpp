// patch_host_check.cpp -- the driver's image-mode loops and render_mosaic over the host binary_matrix alone (no
// device code; tests/test_patch_ref.py builds it from include/ + host/binmat.cpp + host/util.cpp + host/pbm.cpp):
//   patch_host_check gather  I.pbm W dirty X.bin       the samples, every word as it lies in memory
//   patch_host_check scatter X.pbm W rows cols I.pbm   the rows of X put back into an all-ones rows x cols image
//   patch_host_check mosaic  D.pbm out.pbm             render_mosaic's file
//   patch_host_check time    I.pbm W                   prints the wall time of the two loops (tools/time_bsvd_image.py)
// dirty = 1 sets every pad bit of the image before the gather (read_pbm_data clears them).
#include <chrono>
#include <cstdlib>
#include <cstring>

#include "patch_host_loops.h"
#include "util.h"

int main(int argc, char** argv) {
  if (argc >= 6 && !std::strcmp(argv[1], "gather")) {
    binary_matrix I, X;
    if (!load_pbm(argv[2], I)) return 1;
    if (std::atoi(argv[4])) dirty_padding(I);
    host_patches(I, (idx_t)std::strtoul(argv[3], nullptr, 10), X);
    return store_words(argv[5], X) ? 0 : 1;
  }
  if (argc >= 7 && !std::strcmp(argv[1], "scatter")) {
    binary_matrix X;
    if (!load_pbm(argv[2], X)) return 1;
    binary_matrix I((idx_t)std::strtoul(argv[4], nullptr, 10), (idx_t)std::strtoul(argv[5], nullptr, 10));
    I.set();
    host_unpatch(X, (idx_t)std::strtoul(argv[3], nullptr, 10), I);
    return store_pbm(argv[6], I) ? 0 : 1;
  }
  if (argc >= 4 && !std::strcmp(argv[1], "mosaic")) {
    binary_matrix D;
    if (!load_pbm(argv[2], D)) return 1;
    render_mosaic(D, argv[3]);
    return 0;
  }
  if (argc >= 4 && !std::strcmp(argv[1], "time")) {
    binary_matrix I, X;
    if (!load_pbm(argv[2], I)) return 1;
    const idx_t W = (idx_t)std::strtoul(argv[3], nullptr, 10);
    const auto t0 = std::chrono::steady_clock::now();
    host_patches(I, W, X);
    const auto t1 = std::chrono::steady_clock::now();
    host_unpatch(X, W, I);
    const auto t2 = std::chrono::steady_clock::now();
    std::printf("gather_ms=%.3f scatter_ms=%.3f weight=%lu\n", std::chrono::duration<double, std::milli>(t1 - t0).count(),
                std::chrono::duration<double, std::milli>(t2 - t1).count(), (unsigned long)I.weight());
    return 0;
  }
  std::fprintf(stderr, "usage: %s gather|scatter|mosaic|time ...\n", argv[0]);
  return 2;
}
