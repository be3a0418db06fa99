// bic_gpu.h -- the reference C++ API's hot path on an MI355X: what bitplane_tool.cpp, pred.cpp
// and GolombCoder / EGCoder do pixel by pixel on the host, done for whole planes by the HIP
// kernels behind bic.h. Host matrices (binmat.h) are copied to the device as they are (their
// storage already is the kernels' plane layout), results are copied back.
//
// Every call returns a bic.h status code (BIC_OK = 0). A Device whose status() is not BIC_OK
// (no gfx950 GPU, no HIP runtime) fails every call with that code; nothing falls back to the CPU.
#ifndef BIC_GPU_H
#define BIC_GPU_H

#include <stdint.h>

#include <vector>

#include "GolombCoder.h"
#include "bic.h"
#include "binmat.h"
#include "eg.h"
#include "pnm.h"

namespace bic {

// One encoded stream: MSB-first bits, zero-padded to a whole byte.
struct Stream {
  std::vector<uint8_t> bytes;
  uint64_t bits = 0;
};

// Reads and advances the protected state of the reference coders (friend of Golomb and EG).
struct coder_state {
  static bool fresh(const GolombCoder& c) { return c.samples == 0 && c.accumulatedError == 0 && c.k == 1; }
  static bool fresh(const EGCoder& e) { return e.g == 1 && e.blockSize == 1 && e.lutIndex == 0; }
  static unsigned samples(const GolombCoder& c) { return c.samples; }
  static unsigned accumulated(const GolombCoder& c) { return c.accumulatedError; }
  static unsigned k(const GolombCoder& c) { return c.k; }
  // the state codeSample leaves after `n` more samples summing to `sum` that cost `bits` bits
  static void advance(GolombCoder& c, uint64_t n, uint64_t sum, uint64_t bits);
  // the state codeRun leaves after a plane: `ones` non-EOL runs, `bits` bits
  static void advance(EGCoder& e, uint64_t ones, uint64_t bits);
};

// Number of planes bitplane_tool.cpp:24 writes for a maxval: #{bi : 2^bi < maxval}.
int planes_for_maxval(int maxval);

// Result of the W x W tile path (compress7_test.cpp:184-275 with R = 0), one entry per tile in
// raster order.
struct TileResult {
  std::vector<uint32_t> weights;    // the weight that was Golomb-coded (w_pred if 'O' else w_nonpred)
  std::vector<uint32_t> w_nonpred;  // P.weight()
  std::vector<uint32_t> w_pred;     // med(P).weight()
  std::vector<uint8_t> modes;       // 'o' or 'O'
  Stream stream;                    // golomb_nomatch's codewords
  uint64_t L = 0;                   // sum of lentab[chosen weight]
};

// Result of compress7_test.cpp's tile loop with a search window (Device::match_encode), per tile
// in raster order, plus the state the driver's two GolombCoders end in.
struct MatchResult {
  std::vector<uint32_t> besti, bestj, bestd;  // the search (:184; bestd = W*W+1: empty region)
  std::vector<uint32_t> weights;              // the coded weight
  std::vector<uint8_t> modes;                 // 'X' 'x' (match) or 'O' 'o'
  Stream stream_match, stream_nomatch;        // golomb_match / golomb_nomatch codewords
  uint64_t matches = 0, L = 0;                // L: sum of the chosen lengths (before the bitcounts)
};

// Result of the growing-dictionary tile loop of compress2_test.cpp / compress3_test.cpp
// (Device::dict_encode), per tile in raster order over ceil(rows/W) x ceil(cols/W).
struct DictResult {
  std::vector<uint32_t> bestk, bestd;   // the search: first atom at least distance; (0, W*W) when none beats W*W
  std::vector<uint32_t> dsize;          // |D| as the tile saw it
  std::vector<uint32_t> weights;        // the coded value: bestd (match) or the tile's weight
  std::vector<uint8_t> modes, joined;   // 'x' (match) or 'o'; 1 iff the tile was pushed
  std::vector<uint32_t> dict_tiles;     // the tile index of every atom, dictionary order (the final |D| entries)
  Stream stream_match, stream_nomatch;  // variant 3: golomb_match / golomb_nomatch codewords
  uint64_t matches = 0, L = 0;          // L: sum of the chosen lengths (before the bitcounts)
};

class Device {
 public:
  explicit Device(int ordinal = 0);
  ~Device();
  Device(const Device&) = delete;
  Device& operator=(const Device&) = delete;

  int status() const { return status_; }
  bic_ctx* ctx() { return ctx_; }

  // bitplane_tool.cpp:24-30: planes[bi](i,j) = (gray[i*cols+j] >> bi) & 1 for bi < nplanes
  // (1..32). Each planes[bi] must be allocated rows x cols.
  int bitplanes(const pixel_t* gray, idx_t rows, idx_t cols, int nplanes, binary_matrix* planes);

  // pred.cpp:3-15 into R (allocated like P); R(0,0) and R's pad bits keep their old values.
  // weight (nullable) receives the number of residual ones in R outside (0,0).
  int med(const binary_matrix& P, binary_matrix& R, idx_t* weight = nullptr);

  // Runs of every plane (one sample per 1-pixel and one end-of-row sample per row, raster
  // order) coded with a fresh coder per plane: GolombCoder::codeSample (golomb != nullptr) and/or
  // EGCoder::codeRun (eg != nullptr), of the med residual (predict) or of the plane itself.
  // golomb / eg point to nplanes coders that must be fresh; on return they hold the state and
  // bitcount the reference coders would have after coding the same runs. Streams are optional.
  int encode(const binary_matrix* planes, int nplanes, bool predict, GolombCoder* golomb,
             std::vector<Stream>* golomb_streams, EGCoder* eg, std::vector<Stream>* eg_streams);

  // GolombCoder::codeSample over samples[0..n), continuing from the coder's current state.
  int code_samples(GolombCoder& coder, const unsigned* samples, size_t n, Stream* stream = nullptr);

  // The tile path over I (rows and cols multiples of W, 1 <= W <= 64). lentab[w] =
  // (idx_t)(2 + enumL(W*W, w)); pass nullptr to use this build's (coding.h). resid (nullable,
  // allocated like I) receives the image after the residual write-back.
  int tiles(const binary_matrix& I, unsigned W, TileResult* out, const uint64_t* lentab = nullptr,
            binary_matrix* resid = nullptr);

  // compress_test.cpp:73-111: per W x W tile (raster order over ceil(rows/W) x ceil(cols/W)) the
  // least-distance window of the causal search region, first in the reference's scan order.
  int patch_search(const binary_matrix& I, unsigned W, std::vector<uint32_t>* besti,
                   std::vector<uint32_t>* bestj, std::vector<uint32_t>* bestd);

  // compress7_test.cpp:117-275 with W, T, R as its argv[2..4] (rows, cols multiples of W): I is
  // replaced by the image after the residual write-back; golomb_match / golomb_nomatch (fresh)
  // end in the state the driver's coders end in. enuml[w] = enumL(W*W, w) (nullptr: this build's).
  int match_encode(binary_matrix& I, unsigned W, unsigned T, unsigned R, MatchResult* out,
                   GolombCoder* golomb_match = nullptr, GolombCoder* golomb_nomatch = nullptr,
                   const double* enuml = nullptr);

  // compress2_test.cpp:79-129 (variant 2) / compress3_test.cpp:87-149 (variant 3, T as its argv[3]) with W
  // as argv[2], any rows and cols (bic.h bic_dict_encode). atom_step 1: the drivers (atom windows at the
  // pixel of the tile's index pair); W: the tile itself. I is only read. Variant 3: golomb_match /
  // golomb_nomatch (fresh) end in the state the driver's coders end in. enuml as for match_encode.
  int dict_encode(const binary_matrix& I, int variant, unsigned W, unsigned T, unsigned atom_step, DictResult* out,
                  GolombCoder* golomb_match = nullptr, GolombCoder* golomb_nomatch = nullptr,
                  const double* enuml = nullptr);

  // bsvd.cpp:399-460 / 463-527 / 1215-1244 (bic.h "binary dictionary learning"): E and X n x m, D p x m,
  // A n x p, 1 <= p <= 4096, 1 <= m <= 1048576: above m = 4096 the steps run the wide-row entries (bic.h "wide
  // rows"), with the same results. The matrices are uploaded, the step runs on the device, and what it
  // may have changed is downloaded: E and A; E and D; E, D and A. changed / iters (nullable) receive the
  // reference functions' return values. max_iter = 0: no cap (the reference's loop).
  int bsvd_update_coefficients(binary_matrix& E, const binary_matrix& D, binary_matrix& A, idx_t* changed = nullptr);
  int bsvd_update_dictionary(binary_matrix& E, binary_matrix& D, const binary_matrix& A, idx_t* changed = nullptr);
  int bsvd_learn(binary_matrix& X, binary_matrix& E, binary_matrix& D, binary_matrix& A, size_t max_iter = 0,
                 idx_t* iters = nullptr);
  // bsvd.cpp:530-735, the second dictionary rule (E, D and A all change; rounds: the rounds run over all
  // atoms), and the loop with the rule chosen: du = BIC_BSVD_DU_STEEPEST (the call above) or BIC_BSVD_DU_PROXIMUS.
  int bsvd_update_dictionary_proximus(binary_matrix& E, binary_matrix& D, binary_matrix& A, idx_t* changed = nullptr,
                                      idx_t* rounds = nullptr);
  int bsvd_learn(binary_matrix& X, binary_matrix& E, binary_matrix& D, binary_matrix& A, int du, size_t max_iter = 0,
                 idx_t* iters = nullptr);
  // bic_bsvd_learn_lm: the learner lm (BIC_BSVD_LM_*: the loop above, or learn_model_alter1 / 2 / 3 of
  // bsvd.cpp:1247-1434, which leave zero padding in E, D and A) with the rule du
  int bsvd_learn(int lm, int du, binary_matrix& X, binary_matrix& E, binary_matrix& D, binary_matrix& A,
                 size_t max_iter = 0, idx_t* iters = nullptr);
  // bsvd.cpp:99-267, the model initialisers (bic.h "model initialisers"): E is uploaded, D and A are made on the
  // device by the rule mi (BIC_BSVD_MI_*) and downloaded. state: the generator's state (bic_bsvd_rng_seed), read
  // and advanced by the rules that draw; may be null for BIC_BSVD_MI_PARTITION. E needs at least one row.
  int bsvd_initialize(int mi, const binary_matrix& E, binary_matrix& D, binary_matrix& A, uint64_t* state);
  // bsvd.cpp:1438-1717, the MDL model order (bic.h "MDL model order"). bsvd_model_codelength: the code length of
  // the model (E, D, A) in bits, with the reference's truncations; D and A may be empty (no atoms). bsvd_learn_mdl:
  // one search (BIC_BSVD_MDL_*) with the inner learner lmi, the rule du and, for the forward and the full search,
  // the initialiser mi drawing from *state. E receives the result's residual, D and A are re-allocated to the
  // result's atoms where the reference does so: always by the forward and the backward search (an empty result
  // destroys both), by the full search only when a candidate was taken. The forward search may grow the model
  // up to p_cap atoms (0: 4096) and returns BIC_ENOSPC beyond, with the best model so far in E, D and A.
  struct MdlResult {
    idx_t atoms = 0;       // the result's atoms
    uint64_t length = 0;   // the reference's return value
    std::vector<bic_bsvd_mdl_step> trace;  // one record per pass (bic.h)
  };
  int bsvd_model_codelength(const binary_matrix& E, const binary_matrix& D, const binary_matrix& A, uint64_t* length);
  int bsvd_learn_mdl(int search, int lmi, int du, int mi, binary_matrix& X, binary_matrix& E, binary_matrix& D,
                     binary_matrix& A, uint64_t* state, MdlResult* out, size_t p_cap = 0);
  // bsvd_test.cpp:78-151, the driver's image mode (bic.h "image mode"). Each call re-allocates its outputs to
  // the geometry they need, uploads, runs on the device and downloads. patches: the W x W tiles of I as the rows
  // of X (ceil(rows/W) ceil(cols/W) x W^2), the loop of :89-97. unpatch: the rows of X back as the tiles of I,
  // which must have its rows x cols on entry and is overwritten, the loop of :130-139 -- with zero padding, where
  // set_submatrix leaves an edge tile's bits in the pad columns. mosaic: render_mosaic's image of D (util.cpp:53-82).
  // bsvd_learn_image: :78-145 as one call (bic_bsvd_learn_image): X and E from I, D and A (p atoms) by the rule
  // mi, the learner lm with the rule du; residual (nullable) receives E put back as an image of I's geometry.
  int patches(const binary_matrix& I, unsigned W, binary_matrix& X);
  int unpatch(const binary_matrix& X, unsigned W, binary_matrix& I);
  int mosaic(const binary_matrix& D, binary_matrix& image);
  int bsvd_learn_image(int mi, int lm, int du, const binary_matrix& I, unsigned W, idx_t p, binary_matrix& X,
                       binary_matrix& E, binary_matrix& D, binary_matrix& A, uint64_t* state, size_t max_iter = 0,
                       idx_t* iters = nullptr, binary_matrix* residual = nullptr);

 private:
  struct Buf {
    void* p = nullptr;
    size_t cap = 0;
  };
  int ensure(Buf& b, size_t bytes);
  int upload(const binary_matrix& M, uint64_t* dst);
  int download(uint64_t* src, binary_matrix& M);
  int fetch_stream(const uint64_t* slot, uint64_t bits, Stream* s);
  // step: 0 coefficients, 1 dictionary, 2 learn (X then non-null) with the rule du, 3 the PROXIMUS dictionary step
  int bsvd_run(int step, const binary_matrix* X, binary_matrix& E, binary_matrix& D, binary_matrix& A,
               size_t max_iter, idx_t* result, int du = 0, idx_t* rounds = nullptr, int lm = 0);

  bic_ctx* ctx_ = nullptr;
  int status_ = BIC_ENODEV;
  Buf in_, out_a_, out_b_, small_, aux_;
};

// The process-wide device used by the free function med() (pred.h): device 0, created on
// first use. Aborts with a message if it is not usable.
Device& default_device();

}  // namespace bic

#endif
