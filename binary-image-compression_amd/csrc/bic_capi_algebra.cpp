// bic_capi_algebra.cpp -- GF(2) algebra (bic_gf2.hip) and binary dictionary learning (bic_bsvd.hip).
#include "bic_ctx.h"

#include <algorithm>
#include <cstring>

namespace {

bool gf2_geom(size_t rows, size_t cols, size_t wpr) {
  return rows <= 0x7fffffffu && cols <= 0x7fffff00u && wpr >= (cols + 63) / 64 && wpr <= 0xffffffffu;
}

// E (n x m), D (p x m), A (n x p): the domain and the pitches. A row of the narrow kernels (bic_bsvd.hip) has at
// most kBsvdNarrow bits, one of the wide ones (bic_bsvd_wide.hip) at most kBsvdWide.
constexpr size_t kBsvdNarrow = 4096, kBsvdWide = 1048576;
bool bsvd_geom(size_t n, size_t m, size_t e_wpr, size_t p, size_t d_wpr, size_t a_wpr, size_t max_m = kBsvdNarrow) {
  if (m < 1 || m > max_m || p < 1 || p > 4096 || n > 0x7fffffffu) return false;
  const size_t mw = (m + 63) / 64, pw = (p + 63) / 64;
  return e_wpr >= mw && d_wpr >= mw && a_wpr >= pw && e_wpr <= 0xffffffffu && d_wpr <= 0xffffffffu &&
         a_wpr <= 0xffffffffu;
}

// the two steps without their argument checks; `changed` a device u64 that is written; wide: the kernels of
// bic_bsvd_wide.hip (any m of the wide domain), otherwise those of bic_bsvd.hip (m <= kBsvdNarrow)
int bsvd_coef(bic_ctx* ctx, uint64_t* E, size_t n, size_t m, size_t e_wpr, const uint64_t* D, size_t p, size_t d_wpr,
              uint64_t* A, size_t a_wpr, uint64_t* changed, bool wide = false) {
  timed(ctx, wide ? "bsvd_wide_coef" : "bsvd_coef", [&] {
    if (changed) bic::launch_fill(ctx->cur, changed, 0, 8);
    if (n)
      (wide ? bic::launch_bsvd_wide_coef : bic::launch_bsvd_coef)(ctx->cur, E, (uint32_t)n, (uint32_t)m,
                                                                  (uint32_t)e_wpr, D, (uint32_t)p, (uint32_t)d_wpr, A,
                                                                  (uint32_t)a_wpr, changed);
  });
  BIC_HIP(hipGetLastError());
  return BIC_OK;
}

int bsvd_dict(bic_ctx* ctx, uint64_t* E, size_t n, size_t m, size_t e_wpr, uint64_t* D, size_t p, size_t d_wpr,
              const uint64_t* A, size_t a_wpr, uint64_t* changed, bool wide = false) {
  if (!n) {
    if (changed) bic::launch_fill(ctx->cur, changed, 0, 8);
    BIC_HIP(hipGetLastError());
    return BIC_OK;
  }
  int rc = ensure_scratch(ctx, bic::bsvd_wide_scratch_bytes((uint32_t)n, (uint32_t)p));
  if (rc) return rc;
  uint8_t* arena = static_cast<uint8_t*>(ctx->scratch);
  if (!changed) changed = reinterpret_cast<uint64_t*>(arena + bic::kBsvdDictCounts + 16);
  if (wide) {  // every column chunk walks the p atoms by itself: one launch, and one that counts the flags
    timed(ctx, "bsvd_dict_prepare", [&] {
      bic::launch_fill(ctx->cur, changed, 0, 8);
      bic::launch_bsvd_wide_prepare(ctx->cur, (uint32_t)n, (uint32_t)p, A, (uint32_t)a_wpr, ctx->scratch);
    });
    BIC_HIP(hipGetLastError());
    timed(ctx, "bsvd_wide_dict", [&] {
      bic::launch_bsvd_wide_dict(ctx->cur, E, (uint32_t)n, (uint32_t)m, (uint32_t)e_wpr, D, (uint32_t)p,
                                 (uint32_t)d_wpr, ctx->scratch, changed);
    });
    BIC_HIP(hipGetLastError());
    return BIC_OK;
  }
  timed(ctx, "bsvd_dict_prepare", [&] {
    bic::launch_fill(ctx->cur, changed, 0, 8);
    bic::launch_bsvd_dict_prepare(ctx->cur, (uint32_t)n, (uint32_t)p, A, (uint32_t)a_wpr, ctx->scratch);
  });
  // (the atom launches trust the transpose for which rows exist: none is enqueued after a refused launch)
  BIC_HIP(hipGetLastError());
  auto atoms = [&](uint32_t k_lo, uint32_t k_hi) {
    timed(ctx, "bsvd_dict", [&] {
      bic::launch_bsvd_dict_atoms(ctx->cur, E, (uint32_t)n, (uint32_t)m, (uint32_t)e_wpr, D, (uint32_t)p,
                                  (uint32_t)d_wpr, ctx->scratch, k_lo, k_hi, changed);
    });
  };
  // one workgroup that owns every row walks the atoms in one launch; otherwise one launch per atom and
  // one for the last atom's change, ordered by the stream (no workgroup ever waits for another)
  if (bic::bsvd_dict_blocks((uint32_t)n) == 1) {
    atoms(0, (uint32_t)p);
  } else {
    for (uint32_t k = 0; k <= (uint32_t)p; ++k) atoms(k, k);
  }
  BIC_HIP(hipGetLastError());
  return BIC_OK;
}

// update_dictionary_proximus (bsvd.cpp:530-735). All p atoms are enqueued up front, `budget` rounds of
// (atom half, coefficient half) each; the launches of the rounds an atom does not need leave at once, and an
// atom that needs more than its budget stops the batch (every later launch leaves), is read back here and is
// enqueued again with everything after it. One read-back per batch: the call blocks. The automatic budget
// is the one of 1, 2, 4, 8 that was fastest from a sparse-coding step's output, where nearly every atom takes
// two rounds (DESIGN.md §3 "PROXIMUS"): a launch that leaves at once still costs 1.7 us.
constexpr unsigned kBsvdProxAutoRounds = 2;

int bsvd_prox(bic_ctx* ctx, uint64_t* E, size_t n, size_t m, size_t e_wpr, uint64_t* D, size_t p, size_t d_wpr,
              uint64_t* A, size_t a_wpr, uint64_t* changed, uint64_t* h_changed, size_t* rounds, bool wide = false) {
  if (h_changed) *h_changed = 0;
  if (rounds) *rounds = 0;
  if (!n) {
    if (changed) bic::launch_fill(ctx->cur, changed, 0, 8);
    BIC_HIP(hipGetLastError());
    BIC_HIP(hipStreamSynchronize(ctx->cur));
    return BIC_OK;
  }
  int rc = ensure_scratch(ctx, bic::bsvd_wide_scratch_bytes((uint32_t)n, (uint32_t)p));
  if (rc) return rc;
  timed(ctx, "bsvd_dict_prepare",
        [&] { bic::launch_bsvd_dict_prepare(ctx->cur, (uint32_t)n, (uint32_t)p, A, (uint32_t)a_wpr, ctx->scratch); });
  BIC_HIP(hipGetLastError());
  const uint32_t budget = ctx->bsvd_rounds ? ctx->bsvd_rounds : kBsvdProxAutoRounds, np = (uint32_t)p;
  auto atom = [&](uint32_t k, uint32_t r, bool check_prev, bool fresh) {
    timed(ctx, wide ? "bsvd_wide_prox_atom" : "bsvd_prox_atom", [&] {
      (wide ? bic::launch_bsvd_wide_prox_atom : bic::launch_bsvd_prox_atom)(
          ctx->cur, E, (uint32_t)n, (uint32_t)m, (uint32_t)e_wpr, D, np, (uint32_t)d_wpr, ctx->scratch, k, r, budget,
          check_prev, fresh);
    });
  };
  uint8_t* arena = static_cast<uint8_t*>(ctx->scratch);
  uint32_t words[16] = {0};
  for (uint32_t k0 = 0, resumed = 0;; resumed = 1) {
    for (uint32_t k = k0; k < np; ++k)
      for (uint32_t r = 0; r < budget; ++r) {
        atom(k, r, r == 0 && k > k0, r == 0 && !(resumed && k == k0));
        timed(ctx, wide ? "bsvd_wide_prox_coef" : "bsvd_prox_coef", [&] {
          (wide ? bic::launch_bsvd_wide_prox_coef : bic::launch_bsvd_prox_coef)(
              ctx->cur, E, (uint32_t)n, (uint32_t)m, (uint32_t)e_wpr, D, (uint32_t)d_wpr, A, (uint32_t)a_wpr,
              ctx->scratch, k, r);
        });
      }
    atom(np, 0, true, false);  // the last atom's stall
    BIC_HIP(hipGetLastError());
    BIC_HIP(hipMemcpyAsync(words, arena, sizeof(words), hipMemcpyDeviceToHost, ctx->cur));
    BIC_HIP(hipStreamSynchronize(ctx->cur));
    const uint32_t stalled = words[bic::kBsvdProxStalled / 4];
    if (!stalled) break;
    k0 = stalled - 1;
    bic::launch_bsvd_prox_clear_stall(ctx->cur, ctx->scratch);
  }
  uint64_t h[2];
  std::memcpy(&h[0], &words[bic::kBsvdProxChanged / 4], 8);
  std::memcpy(&h[1], &words[bic::kBsvdProxRounds / 4], 8);
  if (changed) {
    BIC_HIP(hipMemcpyAsync(changed, arena + bic::kBsvdProxChanged, 8, hipMemcpyDeviceToDevice, ctx->cur));
    BIC_HIP(hipStreamSynchronize(ctx->cur));
  }
  if (h_changed) *h_changed = h[0];
  if (rounds) *rounds = (size_t)h[1];
  return BIC_OK;
}

// What the learners share. The arena's head is the dictionary step's (sized once for the largest step of
// the call, so that no step's own ensure_scratch moves it); the counts live in it at kBsvdDictCounts.
struct BsvdMat {
  uint64_t* w;
  size_t rows, cols, wpr;
};

// mul(A, false, D, false, E); add(E, X, E) (bsvd.cpp:1219-1220): mul_AB as bic_gf2_mul launches it, in chunks of
// the rows one launch's grid can hold
int bsvd_residual(bic_ctx* ctx, const uint64_t* X, size_t x_wpr, uint64_t* E, size_t n, size_t m, size_t e_wpr,
                  const uint64_t* D, size_t p, size_t d_wpr, const uint64_t* A, size_t a_wpr) {
  const uint32_t mw = (uint32_t)((m + 63) / 64);
  timed(ctx, "gf2_mul", [&] {
    for (size_t r0 = 0; r0 < n; r0 += bic::kGf2MaxRows)
      bic::launch_gf2_ab(ctx->cur, A + r0 * a_wpr, (uint32_t)std::min<size_t>(n - r0, bic::kGf2MaxRows), (uint32_t)a_wpr,
                         (uint32_t)p, D, (uint32_t)d_wpr, mw, E + r0 * e_wpr, (uint32_t)e_wpr, mw * 64u);
  });
  timed(ctx, "bsvd_xor", [&] {
    bic::launch_bsvd_xor(ctx->cur, E, (uint32_t)n, (uint32_t)m, (uint32_t)e_wpr, X, (uint32_t)x_wpr);
  });
  BIC_HIP(hipGetLastError());
  return BIC_OK;
}

// update_coefficients(E, D, A) if `coef`, then update_dictionary(E, D, A) by the rule du; each by the narrow
// kernels where E's rows have at most kBsvdNarrow bits, by the wide ones above. The two counts are read back:
// the call blocks.
int bsvd_pass(bic_ctx* ctx, int du, bool coef, const BsvdMat& E, const BsvdMat& D, const BsvdMat& A, uint64_t* h_coef,
              uint64_t* h_dict) {
  const size_t n = E.rows, m = E.cols, p = D.rows;
  const bool wide = m > kBsvdNarrow;
  uint64_t* counts = reinterpret_cast<uint64_t*>(static_cast<uint8_t*>(ctx->scratch) + bic::kBsvdDictCounts);
  int rc;
  uint64_t h[2] = {0, 0};
  if (coef && (rc = bsvd_coef(ctx, E.w, n, m, E.wpr, D.w, p, D.wpr, A.w, A.wpr, counts, wide))) return rc;
  if (du == BIC_BSVD_DU_PROXIMUS) {  // (blocks itself; the sparse-coding count is read after it)
    if ((rc = bsvd_prox(ctx, E.w, n, m, E.wpr, D.w, p, D.wpr, A.w, A.wpr, nullptr, &h[1], nullptr, wide))) return rc;
    if (coef) BIC_HIP(hipMemcpyAsync(h, counts, 8, hipMemcpyDeviceToHost, ctx->cur));
  } else {
    if ((rc = bsvd_dict(ctx, E.w, n, m, E.wpr, D.w, p, D.wpr, A.w, A.wpr, counts + 1, wide))) return rc;
    if (coef) BIC_HIP(hipMemcpyAsync(h, counts, sizeof(h), hipMemcpyDeviceToHost, ctx->cur));
    else BIC_HIP(hipMemcpyAsync(h + 1, counts + 1, 8, hipMemcpyDeviceToHost, ctx->cur));
  }
  BIC_HIP(hipStreamSynchronize(ctx->cur));
  *h_coef = h[0];
  *h_dict = h[1];
  return BIC_OK;
}

// learn_model_traditional (bsvd.cpp:1215-1244) with either dictionary rule: E = A D ^ X, then the two steps
// until neither changes anything. The counts are read back every iteration: the call blocks.
int bsvd_learn(bic_ctx* ctx, int du, const uint64_t* X, size_t x_wpr, uint64_t* E, size_t n, size_t m, size_t e_wpr,
               uint64_t* D, size_t p, size_t d_wpr, uint64_t* A, size_t a_wpr, size_t max_iter, size_t* iters,
               size_t max_m = kBsvdNarrow) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (!bsvd_geom(n, m, e_wpr, p, d_wpr, a_wpr, max_m) || x_wpr < (m + 63) / 64 || x_wpr > 0xffffffffu ||
      (n && (!X || !E || !D || !A)))
    return BIC_EINVAL;
  if (iters) *iters = 0;
  if ((rc = bsvd_residual(ctx, X, x_wpr, E, n, m, e_wpr, D, p, d_wpr, A, a_wpr))) return rc;
  // the counts live in the dictionary step's arena, which is sized here once (n = 0 still needs them)
  if ((rc = ensure_scratch(ctx, bic::bsvd_wide_scratch_bytes((uint32_t)n, (uint32_t)p)))) return rc;
  const BsvdMat Em{E, n, m, e_wpr}, Dm{D, p, m, d_wpr}, Am{A, n, p, a_wpr};
  size_t it = 0;
  for (;;) {
    ++it;
    uint64_t hc = 0, hd = 0;
    if ((rc = bsvd_pass(ctx, du, true, Em, Dm, Am, &hc, &hd))) return rc;
    if (hc + hd == 0 || (max_iter && it >= max_iter)) break;
  }
  if (iters) *iters = it;
  return BIC_OK;
}

// B (rows x cols) -> T (cols x rows), T's padding bits zero (transpose_to, binmat.cpp:199-208); words of T past
// ceil(rows / 64) are not touched
void bsvd_transpose(bic_ctx* ctx, const BsvdMat& B, const BsvdMat& T) {
  timed(ctx, "gf2_transpose", [&] {
    bic::launch_gf2_transpose(ctx->cur, B.w, (uint32_t)B.rows, (uint32_t)B.wpr, (uint32_t)((B.cols + 63) / 64),
                              (uint32_t)B.cols, T.w, (uint32_t)T.wpr, (uint32_t)((B.rows + 63) / 64));
  });
}

// the role-switching learners' arena: the steps' own part for either role, then Et, At and Dt
size_t bsvd_alter_head_bytes(size_t n, size_t m, size_t p) {
  return (std::max(bic::bsvd_wide_scratch_bytes((uint32_t)n, (uint32_t)p),
                   bic::bsvd_wide_scratch_bytes((uint32_t)m, (uint32_t)p)) + 255) & ~(size_t)255;
}

}  // namespace

// The arena bytes bic_bsvd_learn_lm takes for the learner lm (bic_ctx.h: a caller that keeps data of its own in the
// arena across such calls sizes the arena for them first and puts its data after these bytes)
size_t bsvd_learn_arena_bytes(int lm, size_t n, size_t m, size_t p) {
  if (lm == BIC_BSVD_LM_TRADITIONAL) return bic::bsvd_wide_scratch_bytes((uint32_t)n, (uint32_t)p);
  const size_t nw = (n + 63) / 64, pw = (p + 63) / 64;
  return bsvd_alter_head_bytes(n, m, p) + (m * nw + p * nw + m * pw) * 8;
}

namespace {

// learn_model_alter1 / 2 / 3 (bsvd.cpp:1247-1434) as written. In the exchanged role the calls are
// update_coefficients(Et, At, Dt) and update_dictionary(Et, At, Dt): Et (m x n) the residual, At's p rows of n
// bits the atoms, Dt (m x p) the coefficients. Et, At and Dt live in the arena after the steps' own part.
// max_iter counts every iter++ of the text over the whole call; a pass that reaches it is finished (with its
// transposes back) and the call returns.
int bsvd_learn_alter(bic_ctx* ctx, int lm, int du, const uint64_t* X, size_t x_wpr, uint64_t* E, size_t n, size_t m,
                     size_t e_wpr, uint64_t* D, size_t p, size_t d_wpr, uint64_t* A, size_t a_wpr, size_t max_iter,
                     size_t* iters) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (!bsvd_geom(n, m, e_wpr, p, d_wpr, a_wpr, kBsvdWide) || n < 1 || n > kBsvdWide || x_wpr < (m + 63) / 64 ||
      x_wpr > 0xffffffffu || !X || !E || !D || !A)
    return BIC_EINVAL;
  if (iters) *iters = 0;
  const size_t nw = (n + 63) / 64, pw = (p + 63) / 64;
  const size_t head = bsvd_alter_head_bytes(n, m, p);
  if ((rc = ensure_scratch(ctx, bsvd_learn_arena_bytes(lm, n, m, p)))) return rc;
  uint64_t* tw = reinterpret_cast<uint64_t*>(static_cast<uint8_t*>(ctx->scratch) + head);
  const BsvdMat Em{E, n, m, e_wpr}, Dm{D, p, m, d_wpr}, Am{A, n, p, a_wpr};
  const BsvdMat Et{tw, m, n, nw}, At{tw + m * nw, p, n, nw}, Dt{tw + m * nw + p * nw, m, p, pw};
  auto there = [&] {  // A.transpose_to(At); D.transpose_to(Dt); E.transpose_to(Et)
    bsvd_transpose(ctx, Am, At);
    bsvd_transpose(ctx, Dm, Dt);
    bsvd_transpose(ctx, Em, Et);
  };
  auto back = [&] {
    bsvd_transpose(ctx, At, Am);
    bsvd_transpose(ctx, Dt, Dm);
    bsvd_transpose(ctx, Et, Em);
  };
  if ((rc = bsvd_residual(ctx, X, x_wpr, E, n, m, e_wpr, D, p, d_wpr, A, a_wpr))) return rc;
  size_t total = 0, iter = 0;
  uint64_t hc = 0, hd = 0, changed = 1;
  auto capped = [&] { return max_iter && total >= max_iter; };
  if (lm == BIC_BSVD_LM_ALTER1) {
    while (changed > 0) {  // :1271
      ++iter, ++total;
      if ((rc = bsvd_pass(ctx, du, true, Em, Dm, Am, &hc, &hd))) return rc;  // (its sum is overwritten below)
      there();
      if ((rc = bsvd_pass(ctx, du, true, Et, At, Dt, &hc, &hd))) return rc;
      changed = hd;  // :1297: the transposed dictionary step alone
      back();
      if (capped()) break;
    }
  } else if (lm == BIC_BSVD_LM_ALTER2) {
    uint64_t outer = 1;
    bool stop = false;
    while (outer > 0 && !stop) {  // :1337
      outer = 0;
      while (changed > 0) {  // :1339 (not reset for a second outer pass: skipped there)
        ++iter, ++total;
        if ((rc = bsvd_pass(ctx, du, true, Em, Dm, Am, &hc, &hd))) return rc;
        changed = hc + hd;
        outer += changed;
        if ((stop = capped())) break;
      }
      if (stop) break;
      there();
      changed = 1;
      iter = 0;  // :1359
      while (changed > 0) {  // :1360
        ++iter, ++total;
        if ((rc = bsvd_pass(ctx, du, true, Et, At, Dt, &hc, &hd))) return rc;
        changed = hc + hd;
        outer += changed;
        if ((stop = capped())) break;
      }
      back();
    }
  } else {
    while (changed > 0) {  // :1408
      ++iter, ++total;
      there();
      if ((rc = bsvd_pass(ctx, du, false, Et, At, Dt, &hc, &hd))) return rc;
      back();
      if ((rc = bsvd_pass(ctx, du, false, Em, Dm, Am, &hc, &hd))) return rc;
      changed = hd;  // :1423: only the direct step decides
      if (capped()) break;
    }
  }
  BIC_HIP(hipGetLastError());
  BIC_HIP(hipStreamSynchronize(ctx->cur));
  if (iters) *iters = iter;
  return BIC_OK;
}

// ---- the model initialisers (bsvd.cpp:99-267) ----
// gsl_rng_rand48: x = (0x5DEECE66D x + 0xB) mod 2^48, the output its upper 32 bits
constexpr uint64_t kRand48Mask = (1ull << 48) - 1;
inline uint32_t rand48_next(uint64_t& x) {
  x = (0x5DEECE66Dull * x + 0xBull) & kRand48Mask;
  return (uint32_t)(x >> 16);
}
// gsl_rng_uniform_int: scale = range / bound, draw until output / scale < bound (a rejected output is used up)
inline uint32_t rand48_uniform(uint64_t& x, uint32_t bound) {
  const uint32_t scale = 0xFFFFFFFFu / bound;
  uint32_t k;
  do k = rand48_next(x) / scale;
  while (k >= bound);
  return k;
}

// the initialisers' domain: n = 0 is refused (nothing can be initialised from no data)
bool bsvd_init_geom(const uint64_t* E, size_t n, size_t m, size_t e_wpr, const uint64_t* D, size_t p, size_t d_wpr,
                    const uint64_t* A, size_t a_wpr) {
  return n >= 1 && bsvd_geom(n, m, e_wpr, p, d_wpr, a_wpr) && E && D && A;
}

// one explicit entry: the arena, then the launches (no host synchronisation)
int bsvd_init(bic_ctx* ctx, int mi, const uint64_t* E, size_t n, size_t m, size_t e_wpr, uint64_t* D, size_t p,
              size_t d_wpr, uint64_t* A, size_t a_wpr, const uint32_t* sel) {
  int rc = ensure_scratch(ctx, bic::bsvd_init_scratch_bytes((uint32_t)n, (uint32_t)m, (uint32_t)p));
  if (rc) return rc;
  timed(ctx, "bsvd_init", [&] {
    bic::launch_bsvd_init(ctx->cur, mi, E, (uint32_t)n, (uint32_t)m, (uint32_t)e_wpr, D, (uint32_t)p, (uint32_t)d_wpr, A,
                          (uint32_t)a_wpr, sel, ctx->scratch);
  });
  BIC_HIP(hipGetLastError());
  return BIC_OK;
}

}  // namespace

extern "C" {

int bic_gf2_transpose(bic_ctx* ctx, const uint64_t* src, size_t rows, size_t cols, size_t wpr, uint64_t* dst,
                      size_t dst_wpr) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (!gf2_geom(rows, cols, wpr) || !gf2_geom(cols, rows, dst_wpr)) return BIC_EINVAL;
  if (!rows || !cols) return BIC_OK;
  if (!src || !dst) return BIC_EINVAL;
  timed(ctx, "gf2_transpose", [&] {
    bic::launch_gf2_transpose(ctx->cur, src, (uint32_t)rows, (uint32_t)wpr, (uint32_t)((cols + 63) / 64),
                              (uint32_t)cols, dst, (uint32_t)dst_wpr, (uint32_t)((rows + 63) / 64));
  });
  BIC_HIP(hipGetLastError());
  return BIC_OK;
}

// mul_AB as the kernel; mul_AtB = transpose(A) then mul_AB; mul_ABt = A times the transpose of B's
// whole words (its loop runs over A's blocks, binmat.cpp:586-588), stored for j < B.cols.
int bic_gf2_mul(bic_ctx* ctx, int op, const uint64_t* A, size_t a_rows, size_t a_cols, size_t a_wpr,
                const uint64_t* B, size_t b_rows, size_t b_cols, size_t b_wpr, uint64_t* C, size_t c_rows,
                size_t c_cols, size_t c_wpr) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (!gf2_geom(a_rows, a_cols, a_wpr) || !gf2_geom(b_rows, b_cols, b_wpr) || !gf2_geom(c_rows, c_cols, c_wpr))
    return BIC_EINVAL;
  const uint32_t cw = (uint32_t)((c_cols + 63) / 64);
  switch (op) {
    case BIC_GF2_AB:
      if (c_rows != a_rows || c_cols != b_cols || a_cols != b_rows) return BIC_EINVAL;
      break;
    case BIC_GF2_ATB:
      if (c_rows != a_cols || c_cols != b_cols || a_rows != b_rows) return BIC_EINVAL;
      break;
    case BIC_GF2_ABT:
      if (c_rows != a_rows || c_cols != b_rows || a_cols != b_cols) return BIC_EINVAL;
      break;
    case BIC_GF2_ATBT:
      if (c_rows != a_cols || c_cols != b_rows || a_rows != b_cols) return BIC_EINVAL;
      return BIC_OK;  // binmat.cpp:596-604: "FALTA!" -- C is returned unchanged
    default:
      return BIC_EINVAL;
  }
  if (!c_rows || !cw) return BIC_OK;
  if (!A || !B || !C) return BIC_EINVAL;
  if (op == BIC_GF2_AB) {
    timed(ctx, "gf2_mul", [&] {
      bic::launch_gf2_ab(ctx->cur, A, (uint32_t)a_rows, (uint32_t)a_wpr, (uint32_t)a_cols, B, (uint32_t)b_wpr, cw, C,
                         (uint32_t)c_wpr, cw * 64u);
    });
    BIC_HIP(hipGetLastError());
    return BIC_OK;
  }
  // the transposed operand: At (a_cols x a_rows) or B's whole words transposed (64 aw x b_rows)
  const bool atb = op == BIC_GF2_ATB;
  const uint32_t aw = (uint32_t)((a_cols + 63) / 64);
  const uint64_t t_rows = atb ? a_cols : 64ull * aw, t_src_rows = atb ? a_rows : b_rows;
  const uint32_t t_words = (uint32_t)((t_src_rows + 63) / 64);
  uint64_t* T = nullptr;
  if (t_rows && t_words) {
    BIC_HIP(hipMallocAsync(reinterpret_cast<void**>(&T), (size_t)t_rows * t_words * 8, ctx->cur));
    timed(ctx, "gf2_transpose", [&] {
      if (atb)
        bic::launch_gf2_transpose(ctx->cur, A, (uint32_t)a_rows, (uint32_t)a_wpr, aw, (uint32_t)a_cols, T, t_words,
                                  t_words);
      else
        bic::launch_gf2_transpose(ctx->cur, B, (uint32_t)b_rows, (uint32_t)b_wpr, aw, (uint32_t)t_rows, T, t_words,
                                  t_words);
    });
  }
  timed(ctx, "gf2_mul", [&] {
    if (atb)
      bic::launch_gf2_ab(ctx->cur, T, (uint32_t)a_cols, t_words, (uint32_t)a_rows, B, (uint32_t)b_wpr, cw, C,
                         (uint32_t)c_wpr, cw * 64u);
    else  // cw == t_words (c_cols == b_rows); bits j >= b_rows of the product are 0
      bic::launch_gf2_ab(ctx->cur, A, (uint32_t)a_rows, (uint32_t)a_wpr, (uint32_t)t_rows, T, t_words, cw, C,
                         (uint32_t)c_wpr, (uint32_t)std::min<size_t>(b_cols, 64ull * cw));
  });
  if (T) (void)hipFreeAsync(T, ctx->cur);
  BIC_HIP(hipGetLastError());
  return BIC_OK;
}

int bic_bsvd_update_coefficients(bic_ctx* ctx, uint64_t* E, size_t n, size_t m, size_t e_wpr, const uint64_t* D,
                                 size_t p, size_t d_wpr, uint64_t* A, size_t a_wpr, uint64_t* changed) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (!bsvd_geom(n, m, e_wpr, p, d_wpr, a_wpr) || (n && (!E || !D || !A))) return BIC_EINVAL;
  return bsvd_coef(ctx, E, n, m, e_wpr, D, p, d_wpr, A, a_wpr, changed);
}

int bic_bsvd_update_dictionary(bic_ctx* ctx, uint64_t* E, size_t n, size_t m, size_t e_wpr, uint64_t* D, size_t p,
                               size_t d_wpr, const uint64_t* A, size_t a_wpr, uint64_t* changed) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (!bsvd_geom(n, m, e_wpr, p, d_wpr, a_wpr) || (n && (!E || !D || !A))) return BIC_EINVAL;
  return bsvd_dict(ctx, E, n, m, e_wpr, D, p, d_wpr, A, a_wpr, changed);
}

int bic_bsvd_learn(bic_ctx* ctx, const uint64_t* X, size_t x_wpr, uint64_t* E, size_t n, size_t m, size_t e_wpr,
                   uint64_t* D, size_t p, size_t d_wpr, uint64_t* A, size_t a_wpr, size_t max_iter, size_t* iters) {
  return bsvd_learn(ctx, BIC_BSVD_DU_STEEPEST, X, x_wpr, E, n, m, e_wpr, D, p, d_wpr, A, a_wpr, max_iter, iters);
}

int bic_bsvd_learn_du(bic_ctx* ctx, int du, const uint64_t* X, size_t x_wpr, uint64_t* E, size_t n, size_t m,
                      size_t e_wpr, uint64_t* D, size_t p, size_t d_wpr, uint64_t* A, size_t a_wpr, size_t max_iter,
                      size_t* iters) {
  if (du != BIC_BSVD_DU_STEEPEST && du != BIC_BSVD_DU_PROXIMUS) return BIC_EINVAL;
  return bsvd_learn(ctx, du, X, x_wpr, E, n, m, e_wpr, D, p, d_wpr, A, a_wpr, max_iter, iters);
}

int bic_bsvd_update_dictionary_proximus(bic_ctx* ctx, uint64_t* E, size_t n, size_t m, size_t e_wpr, uint64_t* D,
                                        size_t p, size_t d_wpr, uint64_t* A, size_t a_wpr, uint64_t* changed,
                                        size_t* rounds) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (!bsvd_geom(n, m, e_wpr, p, d_wpr, a_wpr) || (n && (!E || !D || !A))) return BIC_EINVAL;
  return bsvd_prox(ctx, E, n, m, e_wpr, D, p, d_wpr, A, a_wpr, changed, nullptr, rounds);
}

int bic_bsvd_update_coefficients_wide(bic_ctx* ctx, uint64_t* E, size_t n, size_t m, size_t e_wpr, const uint64_t* D,
                                      size_t p, size_t d_wpr, uint64_t* A, size_t a_wpr, uint64_t* changed) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (!bsvd_geom(n, m, e_wpr, p, d_wpr, a_wpr, kBsvdWide) || (n && (!E || !D || !A))) return BIC_EINVAL;
  return bsvd_coef(ctx, E, n, m, e_wpr, D, p, d_wpr, A, a_wpr, changed, true);
}

int bic_bsvd_update_dictionary_wide(bic_ctx* ctx, int du, uint64_t* E, size_t n, size_t m, size_t e_wpr, uint64_t* D,
                                    size_t p, size_t d_wpr, uint64_t* A, size_t a_wpr, uint64_t* changed,
                                    size_t* rounds) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((du != BIC_BSVD_DU_STEEPEST && du != BIC_BSVD_DU_PROXIMUS) ||
      !bsvd_geom(n, m, e_wpr, p, d_wpr, a_wpr, kBsvdWide) || (n && (!E || !D || !A)))
    return BIC_EINVAL;
  if (du == BIC_BSVD_DU_PROXIMUS)
    return bsvd_prox(ctx, E, n, m, e_wpr, D, p, d_wpr, A, a_wpr, changed, nullptr, rounds, true);
  if (!n && rounds) *rounds = 0;
  return bsvd_dict(ctx, E, n, m, e_wpr, D, p, d_wpr, A, a_wpr, changed, true);
}

int bic_bsvd_learn_lm(bic_ctx* ctx, int lm, int du, const uint64_t* X, size_t x_wpr, uint64_t* E, size_t n, size_t m,
                      size_t e_wpr, uint64_t* D, size_t p, size_t d_wpr, uint64_t* A, size_t a_wpr, size_t max_iter,
                      size_t* iters) {
  if (du != BIC_BSVD_DU_STEEPEST && du != BIC_BSVD_DU_PROXIMUS) return BIC_EINVAL;
  if (lm == BIC_BSVD_LM_TRADITIONAL)
    return bsvd_learn(ctx, du, X, x_wpr, E, n, m, e_wpr, D, p, d_wpr, A, a_wpr, max_iter, iters, kBsvdWide);
  if (lm != BIC_BSVD_LM_ALTER1 && lm != BIC_BSVD_LM_ALTER2 && lm != BIC_BSVD_LM_ALTER3) return BIC_EINVAL;
  return bsvd_learn_alter(ctx, lm, du, X, x_wpr, E, n, m, e_wpr, D, p, d_wpr, A, a_wpr, max_iter, iters);
}

int bic_bsvd_rng_seed(uint64_t seed, uint64_t* state) {
  if (!state) return BIC_EINVAL;
  const uint64_t s = seed & 0xFFFFFFFFull;  // gsl_rng_set takes an unsigned long, rand48_set its low 32 bits
  *state = s ? (s << 16) | 0x330Eull : 0x1234ABCD330Eull;
  return BIC_OK;
}

int bic_bsvd_rng_uniform(uint64_t* state, uint32_t bound, size_t count, uint32_t* out) {
  if (!state || !bound || (count && !out)) return BIC_EINVAL;
  uint64_t x = *state & kRand48Mask;
  for (size_t i = 0; i < count; ++i) out[i] = rand48_uniform(x, bound);
  *state = x;
  return BIC_OK;
}

int bic_bsvd_init_neighbor(bic_ctx* ctx, const uint64_t* E, size_t n, size_t m, size_t e_wpr, uint64_t* D, size_t p,
                           size_t d_wpr, uint64_t* A, size_t a_wpr, const uint32_t* rows) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (!bsvd_init_geom(E, n, m, e_wpr, D, p, d_wpr, A, a_wpr) || !rows) return BIC_EINVAL;
  return bsvd_init(ctx, BIC_BSVD_MI_NEIGHBOR, E, n, m, e_wpr, D, p, d_wpr, A, a_wpr, rows);
}

int bic_bsvd_init_partition(bic_ctx* ctx, const uint64_t* E, size_t n, size_t m, size_t e_wpr, uint64_t* D, size_t p,
                            size_t d_wpr, uint64_t* A, size_t a_wpr) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (!bsvd_init_geom(E, n, m, e_wpr, D, p, d_wpr, A, a_wpr)) return BIC_EINVAL;
  return bsvd_init(ctx, BIC_BSVD_MI_PARTITION, E, n, m, e_wpr, D, p, d_wpr, A, a_wpr, nullptr);
}

int bic_bsvd_init_centroids(bic_ctx* ctx, int mi, const uint64_t* E, size_t n, size_t m, size_t e_wpr, uint64_t* D,
                            size_t p, size_t d_wpr, uint64_t* A, size_t a_wpr, const uint32_t* atom_of_row) {
  int rc = bind(ctx);
  if (rc) return rc;
  if ((mi != BIC_BSVD_MI_CENTROIDS && mi != BIC_BSVD_MI_CENTROIDS_XOR) ||
      !bsvd_init_geom(E, n, m, e_wpr, D, p, d_wpr, A, a_wpr) || !atom_of_row)
    return BIC_EINVAL;
  return bsvd_init(ctx, mi, E, n, m, e_wpr, D, p, d_wpr, A, a_wpr, atom_of_row);
}

int bic_bsvd_initialize(bic_ctx* ctx, int mi, const uint64_t* E, size_t n, size_t m, size_t e_wpr, uint64_t* D,
                        size_t p, size_t d_wpr, uint64_t* A, size_t a_wpr, uint64_t* state) {
  int rc = bind(ctx);
  if (rc) return rc;
  if (mi < BIC_BSVD_MI_NEIGHBOR || mi > BIC_BSVD_MI_CENTROIDS_XOR ||
      !bsvd_init_geom(E, n, m, e_wpr, D, p, d_wpr, A, a_wpr) || (mi != BIC_BSVD_MI_PARTITION && !state))
    return BIC_EINVAL;
  if (mi == BIC_BSVD_MI_PARTITION) return bsvd_init(ctx, mi, E, n, m, e_wpr, D, p, d_wpr, A, a_wpr, nullptr);
  // the drawn indices travel through the arena's tail, which the explicit entry leaves alone
  if ((rc = ensure_scratch(ctx, bic::bsvd_init_scratch_bytes((uint32_t)n, (uint32_t)m, (uint32_t)p)))) return rc;
  void* tail = bic::bsvd_init_scratch_tail(ctx->scratch, (uint32_t)m, (uint32_t)p);
  uint64_t x = *state & kRand48Mask;
  std::vector<uint32_t> sel;
  if (mi == BIC_BSVD_MI_NEIGHBOR) {
    std::vector<uint64_t> nz((n + 63) / 64);
    timed(ctx, "bsvd_init_nonzero", [&] {
      bic::launch_bsvd_init_nonzero(ctx->cur, E, (uint32_t)n, (uint32_t)m, (uint32_t)e_wpr,
                                    static_cast<uint64_t*>(tail));
    });
    BIC_HIP(hipGetLastError());
    BIC_HIP(hipMemcpyAsync(nz.data(), tail, nz.size() * 8, hipMemcpyDeviceToHost, ctx->cur));
    BIC_HIP(hipStreamSynchronize(ctx->cur));
    if (std::all_of(nz.begin(), nz.end(), [](uint64_t w) { return w == 0; })) return BIC_EINVAL;  // (:243 would spin)
    sel.resize(p);
    for (size_t k = 0; k < p;) {  // :239-243: a zero row is drawn again and uses up its draw
      const uint32_t i = rand48_uniform(x, (uint32_t)n);
      if ((nz[i >> 6] >> (63u - (i & 63u))) & 1ull) sel[k++] = i;
    }
  } else {
    sel.resize(n);
    for (size_t i = 0; i < n; ++i) sel[i] = rand48_uniform(x, (uint32_t)p);  // :117, :151
  }
  *state = x;
  BIC_HIP(hipMemcpyAsync(tail, sel.data(), sel.size() * 4, hipMemcpyHostToDevice, ctx->cur));
  if ((rc = bsvd_init(ctx, mi, E, n, m, e_wpr, D, p, d_wpr, A, a_wpr, static_cast<const uint32_t*>(tail)))) return rc;
  BIC_HIP(hipStreamSynchronize(ctx->cur));  // (sel leaves scope: the call blocks)
  return BIC_OK;
}

int bic_set_bsvd_rounds(bic_ctx* ctx, unsigned rounds) {
  if (!ctx || rounds > 64) return BIC_EINVAL;
  ctx->bsvd_rounds = rounds;
  return BIC_OK;
}

}  // extern "C"
