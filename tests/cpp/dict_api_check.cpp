// dict_api_check.cpp -- bic::Device::dict_encode through the C++ bridge (tests/test_gpu_dict_host.py):
//   dict_api_check I.pbm variant W T atom_step
// runs the growing-dictionary loop on the default device with two fresh GolombCoders, then feeds the samples
// the result names (every tile but the first: bestd to golomb_match when 'x', else the weight to
// golomb_nomatch) to two host GolombCoders and requires the same bitcount, samples, accumulated error and k.
// Prints one line per coder and the totals for the caller to compare with the restatement.
#include <cstdio>
#include <cstdlib>

#include "bic_gpu.h"
#include "pbm.h"

static void show(const char* name, const GolombCoder& c) {
  std::printf("%s bitcount=%ld samples=%u accumulated=%u k=%u\n", name, (long)c.bitcount, bic::coder_state::samples(c),
              bic::coder_state::accumulated(c), bic::coder_state::k(c));
}

static bool same(const GolombCoder& a, const GolombCoder& b) {
  return a.bitcount == b.bitcount && bic::coder_state::samples(a) == bic::coder_state::samples(b) &&
         bic::coder_state::accumulated(a) == bic::coder_state::accumulated(b) &&
         bic::coder_state::k(a) == bic::coder_state::k(b);
}

int main(int argc, char** argv) {
  if (argc != 6) {
    std::fprintf(stderr, "usage: %s I.pbm variant W T atom_step\n", argv[0]);
    return 2;
  }
  FILE* f = std::fopen(argv[1], "rb");
  idx_t rows = 0, cols = 0;
  if (!f || read_pbm_header(f, rows, cols) != PBM_OK) {
    std::fprintf(stderr, "cannot read %s\n", argv[1]);
    return 1;
  }
  binary_matrix I(rows, cols);
  const bool ok = read_pbm_data(f, I) == PBM_OK;
  std::fclose(f);
  if (!ok) return 1;
  const int variant = std::atoi(argv[2]);
  const unsigned W = (unsigned)std::atoi(argv[3]), T = (unsigned)std::atoi(argv[4]), step = (unsigned)std::atoi(argv[5]);
  bic::Device& dev = bic::default_device();
  bic::DictResult res;
  GolombCoder gm_gpu, gn_gpu, gm, gn;
  const int rc = dev.dict_encode(I, variant, W, T, step, &res, &gm_gpu, &gn_gpu);
  if (rc != BIC_OK) {
    std::fprintf(stderr, "dict_encode: %s\n", bic_strerror(rc));
    return 1;
  }
  if (variant == 3)
    for (size_t t = 1; t < res.modes.size(); ++t) (res.modes[t] == 'x' ? gm : gn).codeSample(res.weights[t]);
  show("match", gm_gpu);
  show("nomatch", gn_gpu);
  std::printf("tiles=%zu matches=%llu L=%llu D=%zu stream_bits=%llu,%llu\n", res.modes.size(),
              (unsigned long long)res.matches, (unsigned long long)res.L, res.dict_tiles.size(),
              (unsigned long long)res.stream_match.bits, (unsigned long long)res.stream_nomatch.bits);
  if (!same(gm, gm_gpu) || !same(gn, gn_gpu)) {
    show("host_match", gm);
    show("host_nomatch", gn);
    std::fprintf(stderr, "the coders' state differs from codeSample over the same samples\n");
    return 1;
  }
  return 0;
}
