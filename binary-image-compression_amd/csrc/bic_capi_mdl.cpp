// bic_capi_mdl.cpp -- the MDL model-order searches of the reference's learner catalogue (bsvd.cpp:1438-1717)
// over the kernels of bic_bsvd_mdl.hip, bic_bsvd_learn_lm and bic_bsvd_initialize.
#include "bic_ctx.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

constexpr size_t kMdlWide = 1048576, kMdlNarrow = 4096, kMdlAtoms = 4096;

bool mdl_geom(size_t n, size_t m, size_t e_wpr, size_t p, size_t d_wpr, size_t a_wpr) {
  if (m < 1 || m > kMdlWide || p > kMdlAtoms || n < 1 || n > 0x7fffffffu) return false;
  const size_t mw = (m + 63) / 64, pw = (p + 63) / 64;
  return e_wpr >= mw && e_wpr <= 0xffffffffu && (!p || (d_wpr >= mw && d_wpr <= 0xffffffffu && a_wpr >= pw &&
                                                        a_wpr <= 0xffffffffu));
}

// idx_t += double and idx_t -= double: the sum goes through double and is truncated toward zero
inline uint64_t plus(uint64_t s, double d) { return (uint64_t)((double)s + d); }
inline uint64_t minus(uint64_t s, double d) { return (uint64_t)((double)s - d); }
inline uint64_t length_e(size_t n, size_t m, uint64_t we) {  // :1450 (unsigned arguments)
  return (uint64_t)bic_universal_codelength((unsigned)(n * m), (unsigned)we);
}

// the weights of a model on the device: we (u64), then wd and wa (u32 x p each), read back in one copy
struct Weights {
  uint64_t we = 0;
  std::vector<uint32_t> w;  // wd, then wa
  const uint32_t* wd() const { return w.data(); }
  const uint32_t* wa(size_t p) const { return w.data() + p; }
};

int mdl_weights(bic_ctx* ctx, const uint64_t* E, size_t n, size_t m, size_t e_wpr, const uint64_t* D, size_t p,
                size_t d_wpr, const uint64_t* A, size_t a_wpr, uint64_t* we, uint32_t* wd, uint32_t* wa) {
  timed(ctx, "bsvd_mdl_weights", [&] {
    bic::launch_bsvd_mdl_weights(ctx->cur, E, (uint32_t)n, (uint32_t)m, (uint32_t)e_wpr, D, (uint32_t)p, (uint32_t)d_wpr,
                                 A, (uint32_t)a_wpr, we, wd, wa);
  });
  BIC_HIP(hipGetLastError());
  return BIC_OK;
}

// dev: 8 + 8 p bytes of device memory; blocks
int mdl_read_weights(bic_ctx* ctx, const uint64_t* E, size_t n, size_t m, size_t e_wpr, const uint64_t* D, size_t p,
                     size_t d_wpr, const uint64_t* A, size_t a_wpr, uint8_t* dev, Weights* out) {
  uint32_t* wd = reinterpret_cast<uint32_t*>(dev + 8);
  int rc = mdl_weights(ctx, E, n, m, e_wpr, D, p, d_wpr, A, a_wpr, reinterpret_cast<uint64_t*>(dev), wd, wd + p);
  if (rc) return rc;
  std::vector<uint8_t> h(8 + 8 * p);
  BIC_HIP(hipMemcpyAsync(h.data(), dev, h.size(), hipMemcpyDeviceToHost, ctx->cur));
  BIC_HIP(hipStreamSynchronize(ctx->cur));
  std::memcpy(&out->we, h.data(), 8);
  out->w.resize(2 * p);
  if (p) std::memcpy(out->w.data(), h.data() + 8, 8 * p);
  return BIC_OK;
}

// model_codelength (bsvd.cpp:1438-1461) from the weights; ld, la (optional) receive the two running sums
uint64_t mdl_length(size_t n, size_t m, size_t p, const Weights& w, uint64_t* ld = nullptr, uint64_t* la = nullptr) {
  const uint64_t LE = length_e(n, m, w.we);
  uint64_t LD = 0, LA = 0;
  for (size_t k = 0; k < p; ++k) {
    LD = plus(LD, bic_universal_codelength((unsigned)m, w.wd()[k]));
    LA = plus(LA, bic_universal_codelength((unsigned)n, w.wa(p)[k]));
  }
  if (ld) *ld = LD;
  if (la) *la = LA;
  return LE + LD + LA;
}

struct Mat {
  uint64_t* w;
  size_t wpr;
};

// One search's state: the arena's layout and the steps the three searches share
struct Search {
  bic_ctx* ctx;
  int lmi, du, mi;
  const uint64_t* X;
  size_t x_wpr, n, m, mw;
  uint8_t* wts;      // 8 + 8 p_cap bytes: the weights
  uint64_t* score;   // p_cap u64: the removal scores
  void* drop_scratch;
  uint64_t* rng;
  bic_bsvd_mdl_step* trace;
  size_t trace_cap, nrec = 0;

  void note(const bic_bsvd_mdl_step& r) {
    if (trace && nrec < trace_cap) trace[nrec] = r;
    ++nrec;
  }
  void copy(const Mat& dst, const Mat& src, size_t rows, size_t words) {
    timed(ctx, "bsvd_mdl_copy", [&] {
      bic::launch_bsvd_mdl_copy(ctx->cur, dst.w, (uint32_t)dst.wpr, src.w, (uint32_t)src.wpr, (uint32_t)rows,
                                (uint32_t)words);
    });
  }
  // the caller's matrices receive the model (E, D, A) of K atoms
  void copy_out(const Mat& E, const Mat& D, const Mat& A, const Mat& e, const Mat& d, const Mat& a, size_t K) {
    copy(E, e, n, mw);
    copy(D, d, K, mw);
    copy(A, a, n, (K + 63) / 64);
  }
  int learn(const Mat& E, const Mat& D, const Mat& A, size_t K) {
    size_t it = 0;
    return bic_bsvd_learn_lm(ctx, lmi, du, X, x_wpr, E.w, n, m, E.wpr, D.w, K, D.wpr, A.w, A.wpr, 0, &it);
  }
  int init(const uint64_t* from, size_t from_wpr, const Mat& D, const Mat& A, size_t K) {
    return bic_bsvd_initialize(ctx, mi, from, n, m, from_wpr, D.w, K, D.wpr, A.w, A.wpr, rng);
  }
  int length(const Mat& E, const Mat& D, const Mat& A, size_t K, uint64_t* len) {
    Weights w;
    int rc = mdl_read_weights(ctx, E.w, n, m, E.wpr, D.w, K, D.wpr, A.w, A.wpr, wts, &w);
    if (rc) return rc;
    *len = mdl_length(n, m, K, w);
    return BIC_OK;
  }
};

// what the reference prints at the start of a forward or backward pass (:1485-1487, :1572-1574)
struct Stuck {
  uint64_t stuck = 0, sum = 0, all = 0;
  int32_t dev() const { return all > 0 ? (int32_t)(uint32_t)(sum / all) : 0; }
  void reject(uint64_t len, uint64_t best) {
    ++stuck;
    ++all;
    sum += len - best;
  }
};
inline int32_t int_dif(uint64_t a, uint64_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }
inline bool better(uint64_t len, int32_t dev, uint64_t best) { return len + (uint64_t)(int64_t)dev < best; }

#define MDL_TRY(x)            \
  do {                        \
    if ((rc = (x))) return rc; \
  } while (0)

// learn_model_mdl_forward_selection (bsvd.cpp:1463-1546)
int forward(Search& s, const Mat& E, const Mat& D, size_t p, size_t p_cap, const Mat& A, const Mat& cE, const Mat& cD,
            const Mat& cA, const Mat& atom, const Mat& coefs, size_t* p_out, uint64_t* best_len) {
  int rc;
  size_t K = p;
  MDL_TRY(s.learn(E, D, A, K));                                   // :1470
  s.copy(cD, D, K, s.mw);                                         // :1473
  s.copy(cA, A, s.n, (K + 63) / 64);
  s.copy(cE, E, s.n, s.mw);
  uint64_t bestK = K, bestL = 0, currL = 0;
  MDL_TRY(s.length(E, D, A, K, &bestL));                          // :1476
  *p_out = K;
  *best_len = bestL;
  Stuck st;
  do {
    MDL_TRY(s.length(cE, cD, cA, K, &currL));                     // :1484
    const int32_t dif = int_dif(currL, bestL), dev = st.dev();
    s.note({K, currL, bestK, bestL, st.stuck, dif, dev, 0, 0, {0}});
    if (K + 1 > p_cap) return BIC_ENOSPC;
    MDL_TRY(s.init(cE.w, cE.wpr, atom, coefs, 1));                // :1488
    timed(s.ctx, "bsvd_mdl_append", [&] {                         // :1497-1513
      bic::launch_bsvd_mdl_append_atom(s.ctx->cur, cD.w, (uint32_t)K, (uint32_t)s.m, (uint32_t)cD.wpr, cA.w,
                                       (uint32_t)s.n, (uint32_t)cA.wpr, atom.w, coefs.w, (uint32_t)coefs.wpr);
    });
    MDL_TRY(s.learn(cE, cD, cA, K + 1));                          // :1515
    MDL_TRY(s.length(cE, cD, cA, K + 1, &currL));                 // :1516
    if (better(currL, dev, bestL)) {                              // :1517
      st.stuck = 0;
      bestL = currL;
      s.copy_out(E, D, A, cE, cD, cA, K + 1);
      bestK = K + 1;
      *p_out = bestK;
      *best_len = bestL;
    } else {
      st.reject(currL, bestL);
      if (st.stuck >= 10) break;
    }
    ++K;
  } while (st.stuck < 10);
  return BIC_OK;
}

// learn_model_mdl_backward_selection (bsvd.cpp:1548-1663)
int backward(Search& s, const Mat& E, const Mat& D, size_t p, const Mat& A, const Mat& cE, const Mat& cD, const Mat& cA,
             size_t* p_out, uint64_t* best_len) {
  int rc;
  size_t K = p;
  MDL_TRY(s.learn(E, D, A, K));                                   // :1555
  uint64_t bestL = 0;
  MDL_TRY(s.length(E, D, A, K, &bestL));                          // :1558
  uint64_t bestK = K, currL = bestL;
  s.copy(cD, D, K, s.mw);                                         // :1563-1564
  s.copy(cA, A, s.n, (K + 63) / 64);
  *p_out = K;
  *best_len = bestL;
  Stuck st;
  std::vector<uint64_t> score;
  for (; K > 0; --K) {
    const int32_t dif = int_dif(currL, bestL), dev = st.dev();
    // :1577-1590 the K scores from the caller-visible E with the current D and A
    timed(s.ctx, "bsvd_mdl_drop", [&] {
      bic::launch_bsvd_mdl_drop_weights(s.ctx->cur, E.w, (uint32_t)s.n, (uint32_t)s.m, (uint32_t)E.wpr, cD.w, (uint32_t)K,
                                        (uint32_t)cD.wpr, cA.w, (uint32_t)cA.wpr, s.score, s.drop_scratch);
    });
    BIC_HIP(hipGetLastError());
    score.resize(K);
    BIC_HIP(hipMemcpyAsync(score.data(), s.score, K * 8, hipMemcpyDeviceToHost, s.ctx->cur));
    Weights w;
    MDL_TRY(mdl_read_weights(s.ctx, E.w, s.n, s.m, E.wpr, cD.w, K, cD.wpr, cA.w, cA.wpr, s.wts, &w));  // (waits)
    uint64_t LD = 0, LA = 0;
    (void)mdl_length(s.n, s.m, K, w, &LD, &LA);
    size_t nextk = 0;
    uint64_t nextL = ~(1ull << (sizeof(uint64_t) - 1));             // :1576
    for (size_t k = 0; k < K; ++k) {
      uint64_t tmpL = length_e(s.n, s.m, score[k]) + LD + LA;       // :1583
      tmpL = minus(tmpL, bic_universal_codelength((unsigned)s.m, w.wd()[k]));  // :1584
      tmpL = minus(tmpL, bic_universal_codelength((unsigned)s.n, w.wa(K)[k]));  // :1585
      if (tmpL < nextL) {
        nextL = tmpL;
        nextk = k;
      }
    }
    s.note({K, currL, bestK, bestL, st.stuck, dif, dev, (uint32_t)nextk, 0, {0}});
    if (K > 1) {                                                    // :1596-1612
      timed(s.ctx, "bsvd_mdl_drop_atom", [&] {
        bic::launch_bsvd_mdl_drop_atom(s.ctx->cur, cD.w, (uint32_t)K, (uint32_t)s.m, (uint32_t)cD.wpr, cA.w,
                                       (uint32_t)s.n, (uint32_t)cA.wpr, (uint32_t)nextk);
      });
      MDL_TRY(s.learn(cE, cD, cA, K - 1));
      MDL_TRY(s.length(cE, cD, cA, K - 1, &nextL));
    } else {
      nextL = length_e(s.n, s.m, score[0]);                         // :1614 nextE as the k = 0 score left it
    }
    if (better(nextL, dev, bestL)) {                                // :1617
      if (K == 1) {                                                 // :1619-1625 (best_len keeps its value)
        s.copy(E, Mat{const_cast<uint64_t*>(s.X), s.x_wpr}, s.n, s.mw);
        *p_out = 0;
        break;
      }
      st.stuck = 0;
      bestK = K - 1;
      bestL = nextL;
      s.copy_out(E, D, A, cE, cD, cA, K - 1);
      *p_out = bestK;
      *best_len = bestL;
    } else {
      st.reject(nextL, bestL);
      if (st.stuck >= 10) break;
    }
    currL = nextL;                                                  // :1653
  }
  return BIC_OK;
}

// learn_model_mdl_full_search (bsvd.cpp:1665-1717)
int full_search(Search& s, const Mat& E, const Mat& D, size_t p, const Mat& A, const Mat& cE, const Mat& cD,
                const Mat& cA, size_t* p_out, uint64_t* best_len) {
  int rc;
  uint64_t bestL = 1ull << 30, bestk = 0;                           // :1674-1675
  *p_out = 0;
  *best_len = bestL;
  for (size_t k = 20; k <= p; k += 20) {                            // :1676
    MDL_TRY(s.init(s.X, s.x_wpr, cD, cA, k));                       // :1679-1680: thrown away
    MDL_TRY(s.learn(cE, cD, cA, k));
    bic_bsvd_mdl_step r = {k, 0, 0, 0, 0, 0, 0, 0, 0, {0}};
    for (int i = 0; i < 10; ++i) {                                  // :1685-1691
      MDL_TRY(s.init(s.X, s.x_wpr, cD, cA, k));
      MDL_TRY(s.learn(cE, cD, cA, k));
      MDL_TRY(s.length(cE, cD, cA, k, &r.lens[i]));
    }
    const uint64_t candL = *std::min_element(r.lens, r.lens + 10);  // :1692
    if (candL < bestL) {                                            // :1698: the last repetition's model
      bestL = candL;
      bestk = k;
      s.copy_out(E, D, A, cE, cD, cA, k);
      *p_out = k;
      *best_len = bestL;
    }
    r.currL = candL;
    r.bestK = bestk;
    r.bestL = bestL;
    s.note(r);
  }
  return BIC_OK;
}

}  // namespace

extern "C" {

double bic_universal_codelength(unsigned n, unsigned r) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double half_log = 0.5 * std::log2((double)n);
  if (r == 0 || r >= n) return half_log;
  const double p = (double)r / (double)n;
  return double(n) * (-p * std::log2(p) - (1.0 - p) * std::log2(1.0 - p)) + half_log;
}

int bic_bsvd_model_weights(bic_ctx* ctx, const uint64_t* E, size_t n, size_t m, size_t e_wpr, const uint64_t* D,
                           size_t p, size_t d_wpr, const uint64_t* A, size_t a_wpr, uint64_t* we, uint32_t* wd,
                           uint32_t* wa) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (!mdl_geom(n, m, e_wpr, p, d_wpr, a_wpr) || !E || !we || (p && (!D || !A || !wd || !wa))) return BIC_EINVAL;
  return mdl_weights(ctx, E, n, m, e_wpr, D, p, d_wpr, A, a_wpr, we, wd, wa);
}

int bic_bsvd_drop_weights(bic_ctx* ctx, const uint64_t* E, size_t n, size_t m, size_t e_wpr, const uint64_t* D,
                          size_t p, size_t d_wpr, const uint64_t* A, size_t a_wpr, uint64_t* w) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (!mdl_geom(n, m, e_wpr, p, d_wpr, a_wpr) || p < 1 || !E || !D || !A || !w) return BIC_EINVAL;
  if ((rc = ensure_scratch(ctx, bic::bsvd_mdl_drop_scratch_bytes()))) return rc;
  timed(ctx, "bsvd_mdl_drop", [&] {
    bic::launch_bsvd_mdl_drop_weights(ctx->cur, E, (uint32_t)n, (uint32_t)m, (uint32_t)e_wpr, D, (uint32_t)p,
                                      (uint32_t)d_wpr, A, (uint32_t)a_wpr, w, ctx->scratch);
  });
  BIC_HIP(hipGetLastError());
  return BIC_OK;
}

int bic_bsvd_drop_atom(bic_ctx* ctx, uint64_t* D, size_t p, size_t m, size_t d_wpr, uint64_t* A, size_t n,
                       size_t a_wpr, size_t k) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (!mdl_geom(n, m, (m + 63) / 64, p, d_wpr, a_wpr) || p < 1 || k >= p || !D || !A) return BIC_EINVAL;
  timed(ctx, "bsvd_mdl_drop_atom", [&] {
    bic::launch_bsvd_mdl_drop_atom(ctx->cur, D, (uint32_t)p, (uint32_t)m, (uint32_t)d_wpr, A, (uint32_t)n,
                                   (uint32_t)a_wpr, (uint32_t)k);
  });
  BIC_HIP(hipGetLastError());
  return BIC_OK;
}

int bic_bsvd_append_atom(bic_ctx* ctx, uint64_t* D, size_t p, size_t m, size_t d_wpr, uint64_t* A, size_t n,
                         size_t a_wpr, const uint64_t* atom, size_t atom_wpr, const uint64_t* coefs, size_t c_wpr) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (p >= kMdlAtoms || !mdl_geom(n, m, (m + 63) / 64, p + 1, d_wpr, a_wpr) || atom_wpr < (m + 63) / 64 || c_wpr < 1 ||
      c_wpr > 0xffffffffu || !D || !A || !atom || !coefs)
    return BIC_EINVAL;
  timed(ctx, "bsvd_mdl_append", [&] {
    bic::launch_bsvd_mdl_append_atom(ctx->cur, D, (uint32_t)p, (uint32_t)m, (uint32_t)d_wpr, A, (uint32_t)n,
                                     (uint32_t)a_wpr, atom, coefs, (uint32_t)c_wpr);
  });
  BIC_HIP(hipGetLastError());
  return BIC_OK;
}

int bic_bsvd_model_codelength(bic_ctx* ctx, const uint64_t* E, size_t n, size_t m, size_t e_wpr, const uint64_t* D,
                              size_t p, size_t d_wpr, const uint64_t* A, size_t a_wpr, uint64_t* len) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (!mdl_geom(n, m, e_wpr, p, d_wpr, a_wpr) || (unsigned)(n * m) == 0 || !E || !len || (p && (!D || !A)))
    return BIC_EINVAL;
  if ((rc = ensure_scratch(ctx, 8 + 8 * p))) return rc;
  Weights w;
  if ((rc = mdl_read_weights(ctx, E, n, m, e_wpr, D, p, d_wpr, A, a_wpr, static_cast<uint8_t*>(ctx->scratch), &w)))
    return rc;
  *len = mdl_length(n, m, p, w);
  return BIC_OK;
}

int bic_bsvd_learn_mdl(bic_ctx* ctx, int search, int lmi, int du, int mi, const uint64_t* X, size_t x_wpr,
                       uint64_t* E, size_t n, size_t m, size_t e_wpr, uint64_t* D, size_t p, size_t p_cap,
                       size_t d_wpr, uint64_t* A, size_t a_wpr, uint64_t* rng_state, size_t* p_out,
                       uint64_t* best_len, bic_bsvd_mdl_step* trace, size_t trace_cap, size_t* trace_len) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (trace_len) *trace_len = 0;
  const bool inits = search == BIC_BSVD_MDL_FORWARD || search == BIC_BSVD_MDL_FULL;
  if (search < BIC_BSVD_MDL_FORWARD || search > BIC_BSVD_MDL_FULL || lmi < BIC_BSVD_LM_TRADITIONAL ||
      lmi > BIC_BSVD_LM_ALTER3 || (du != BIC_BSVD_DU_STEEPEST && du != BIC_BSVD_DU_PROXIMUS) || p < 1 || p > p_cap ||
      !mdl_geom(n, m, e_wpr, p_cap, d_wpr, a_wpr) || (unsigned)(n * m) == 0 || x_wpr < (m + 63) / 64 ||
      x_wpr > 0xffffffffu || !X || !E || !D || !A || !p_out || !best_len || (trace_cap && !trace))
    return BIC_EINVAL;
  if (lmi != BIC_BSVD_LM_TRADITIONAL && n > kMdlWide) return BIC_EINVAL;
  if (inits && (m > kMdlNarrow || mi < BIC_BSVD_MI_NEIGHBOR || mi > BIC_BSVD_MI_CENTROIDS_XOR ||
                (mi != BIC_BSVD_MI_PARTITION && !rng_state)))
    return BIC_EINVAL;
  // The arena: what the inner learner and the initialiser take from its start for any model of the call, then the
  // weights, the scores and the working copies. Sized once, so that no step's own ensure_scratch moves it.
  const size_t mw = (m + 63) / 64, pwc = (p_cap + 63) / 64;
  size_t head = 0;
  for (size_t K = 1; K <= p_cap; ++K) {
    head = std::max(head, bsvd_learn_arena_bytes(lmi, n, m, K));
    if (search == BIC_BSVD_MDL_FULL || K == 1)
      head = std::max(head, bic::bsvd_init_scratch_bytes((uint32_t)n, (uint32_t)m, (uint32_t)K));
  }
  head = (head + 255) & ~(size_t)255;
  const size_t wts_bytes = (8 + 8 * p_cap + 255) & ~(size_t)255, score_bytes = (8 * p_cap + 255) & ~(size_t)255;
  const size_t words = p_cap * mw + n * pwc + n * mw + mw + n;
  if ((rc = ensure_scratch(ctx, head + wts_bytes + score_bytes + 256 + words * 8))) return rc;
  uint8_t* base = static_cast<uint8_t*>(ctx->scratch) + head;
  Search s{ctx, lmi, du, mi, X, x_wpr, n, m, mw, base, reinterpret_cast<uint64_t*>(base + wts_bytes),
           base + wts_bytes + score_bytes, rng_state, trace, trace_cap};
  uint64_t* wk = reinterpret_cast<uint64_t*>(base + wts_bytes + score_bytes + 256);
  const Mat Em{E, e_wpr}, Dm{D, d_wpr}, Am{A, a_wpr};
  const Mat cD{wk, mw}, cA{wk + p_cap * mw, pwc}, cE{cA.w + n * pwc, mw}, atom{cE.w + n * mw, mw}, coefs{atom.w + mw, 1};
  if (search == BIC_BSVD_MDL_FORWARD)
    rc = forward(s, Em, Dm, p, p_cap, Am, cE, cD, cA, atom, coefs, p_out, best_len);
  else if (search == BIC_BSVD_MDL_BACKWARD)
    rc = backward(s, Em, Dm, p, Am, cE, cD, cA, p_out, best_len);
  else
    rc = full_search(s, Em, Dm, p, Am, cE, cD, cA, p_out, best_len);
  if (trace_len) *trace_len = s.nrec;
  if (rc == BIC_EDEVICE) return rc;
  BIC_HIP(hipGetLastError());
  BIC_HIP(hipStreamSynchronize(ctx->cur));  // (the copies out)
  return rc;
}

}  // extern "C"
