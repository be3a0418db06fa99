// bic_ctx.h -- the per-device context behind the C ABI (bic_capi*.cpp): its stream, scratch arena,
// deferred-error flags and kernel timing, and what every family's entry points do with them. Not
// installed; the public surface is include/bic.h.
#pragma once
#include "bic.h"
#include "bic_internal.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

// A failing HIP call returns BIC_EDEVICE; with BIC_VERBOSE set in the environment it is also named on
// stderr (source file and line, call, HIP's error string)
inline void hip_fail(hipError_t e, const char* file, int line, const char* what) {
  static const bool verbose = std::getenv("BIC_VERBOSE") != nullptr;
  if (verbose) std::fprintf(stderr, "%s:%d: %s: %s\n", file, line, what, hipGetErrorString(e));
}
#define BIC_HIP(x)                                       \
  do {                                                   \
    const hipError_t bic_e_ = (x);                       \
    if (bic_e_ != hipSuccess) {                          \
      hip_fail(bic_e_, __FILE_NAME__, __LINE__, #x);     \
      return BIC_EDEVICE;                                \
    }                                                    \
  } while (0)

// A host table the kernels read from device memory (the tile length table, the match loop's enumL):
// kept on the device until the caller passes another one.
template <class T>
struct DeviceTable {
  T* dev = nullptr;
  T* pinned = nullptr;  // host staging of `cap` entries, as dev
  size_t cap = 0;
  std::vector<T> host;  // what dev holds

  // A table equal to the one on the device is not re-sent, so repeated calls do not synchronise the
  // host with the stream. Otherwise: wait for `s` (the previous copy out of the staging buffer, and
  // the kernels that read the old table), grow, copy through the staging buffer, remember.
  int upload(hipStream_t s, const T* src, size_t n) {
    if (host.size() == n && std::memcmp(host.data(), src, n * sizeof(T)) == 0) return BIC_OK;
    BIC_HIP(hipStreamSynchronize(s));
    if (cap < n) {
      release();
      if (hipHostMalloc(reinterpret_cast<void**>(&pinned), n * sizeof(T)) != hipSuccess ||
          hipMalloc(reinterpret_cast<void**>(&dev), n * sizeof(T)) != hipSuccess) {
        release();
        return BIC_ENOMEM;
      }
      cap = n;
    }
    host.clear();  // (a failed copy leaves no table remembered)
    std::memcpy(pinned, src, n * sizeof(T));
    BIC_HIP(hipMemcpyAsync(dev, pinned, n * sizeof(T), hipMemcpyHostToDevice, s));
    host.assign(src, src + n);
    return BIC_OK;
  }
  void release() {
    if (pinned) (void)hipHostFree(pinned);
    if (dev) (void)hipFree(dev);
    pinned = dev = nullptr;
    cap = 0;
    host.clear();
  }
};

struct bic_ctx {
  int device = 0;
  hipStream_t own = nullptr;
  hipStream_t cur = nullptr;
  hipStream_t aux = nullptr;      // the staged encoder's second stream (REST emit launch), made on first use
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  void* scratch = nullptr;
  size_t scratch_bytes = 0;
  // bytes at the arena's start left zero by the last call (the single / two-pass encoder's k_fixup
  // clears its counter and look-back records for the next call); ensure_scratch hands the value to
  // its caller (scratch_zero_prev) and resets it, since any other user may dirty the arena
  size_t scratch_zero = 0, scratch_zero_prev = 0;
  // a call that took the arena was enqueued under stream capture: graph replays then run work this
  // bookkeeping never sees (a captured call leaves nothing zeroed when enqueued, and a replay may dirty
  // the arena between two eager calls), so from then on every single / two-pass call clears the records
  // itself. The rule: whoever takes the arena passes ensure_scratch, and ensure_scratch notes capture.
  bool captured = false;
  uint64_t* lut = nullptr;        // device [3][256] byte table of the fused encoder
  uint32_t* flags = nullptr;      // device [4]: overflow, domain, look-back timeout, internal length check
  DeviceTable<uint64_t> lentab;   // the tile length table (bic_patch_encode)
  DeviceTable<double> enuml;      // the match loop's enumL table (bic_match_encode*)
  uint64_t* rbuf = nullptr;       // bic_encode_gray* without planes: the count pass's residual planes
  size_t rbuf_bytes = 0;
  unsigned match_parts = 0;       // bic_set_match_parts: workgroups per tile (0 = by region size)
  unsigned dict_block = 0;        // bic_set_dict_block: tiles resolved per block (0 = automatic)
  unsigned bsvd_rounds = 0;       // bic_set_bsvd_rounds: PROXIMUS rounds enqueued per atom (0 = automatic)
  // kernel timing (bic_prof_*): HIP events recorded on the launch stream around each kernel
  bool prof_on = false;
  std::string prof_only;  // bic_prof_only: bracket only launches of this name ("" = all)
  bool force_multipass = false;
  bool two_pass = false;       // BIC_OPT_TWO_PASS: the two-pass row encoder instead of the staged one
  bool single_kernel = false;  // BIC_OPT_SINGLE_KERNEL: the single kernel with decoupled look-backs
  bool force_staged = false;   // BIC_OPT_STAGED: the staged encoder whatever the batch size
  bool one_stream = false;     // BIC_OPT_ONE_STREAM: no second stream for the staged encoder's emission
  bool eg_src_off = false;     // BIC_OPT_EG_SOURCE = 0: bic_encode_gray* stores R instead of writing EG
  bool eg_src_one = false;     // BIC_OPT_EG_SOURCE = 2: one emission kernel for every row class
  bool gray_code = false;      // BIC_OPT_GRAY_CODE: samples <-> planes go through G(v) = v ^ (v >> 1)
  int color_transform = 0;     // BIC_OPT_COLOR_TRANSFORM: the RGB calls' per-pixel transform in front of G
  int sample_predict = 0;      // BIC_OPT_SAMPLE_PREDICT: one-byte gray samples minus their left neighbour, in front of G
  int rgb_predict = 0;         // BIC_OPT_RGB_PREDICT: the same on each channel of the RGB calls, behind the colour transform
  struct Rec { std::string name; hipEvent_t a, b; };
  std::vector<Rec> recs;
  std::vector<hipEvent_t> pool;
};

#ifndef BIC_PROF_EVENT_FLAGS
#define BIC_PROF_EVENT_FLAGS hipEventDisableSystemFence
#endif

inline hipEvent_t take_event(bic_ctx* ctx) {
  if (!ctx->pool.empty()) {
    hipEvent_t e = ctx->pool.back();
    ctx->pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  // device-scope timing events: a system-scope release at every record would write back L2 between
  // the launches it brackets
  if (hipEventCreateWithFlags(&e, BIC_PROF_EVENT_FLAGS) != hipSuccess) (void)hipEventCreate(&e);
  return e;
}

inline bool prof_wants(bic_ctx* ctx, const char* name) {
  return ctx->prof_on && (ctx->prof_only.empty() || ctx->prof_only == name);
}

// The row encoders' emission stage: `name` times the staged encoder's main kernel alone (events the
// launch records on its own stream right around that kernel, EmitStreams::main*: the roofline
// kernel's launch duration), "<name>_stage" the whole stage, the second stream's fork and join included.
template <typename F>
void timed_rows(bic_ctx* ctx, bic::EmitStreams& es, const char* name, F&& launch) {
  if (!ctx->prof_on) return launch();
  const std::string stage_name = std::string(name) + "_stage";
  const bool k = prof_wants(ctx, name), st = prof_wants(ctx, stage_name.c_str());
  hipEvent_t a = nullptr, b = nullptr, sa = nullptr, sb = nullptr;
  bool main_rec = false;
  if (k) {
    a = take_event(ctx);
    b = take_event(ctx);
    // (recorded here too: a path without a separate main kernel -- the single and two-pass encoders --
    // then times the whole stage, b recorded below)
    (void)hipEventRecord(a, ctx->cur);
    es.main0 = a;
    es.main1 = b;
    es.main_rec = &main_rec;
  }
  if (st) {
    sa = take_event(ctx);
    sb = take_event(ctx);
    (void)hipEventRecord(sa, ctx->cur);
  }
  launch();
  // (an event never recorded would fail hipEventElapsedTime, and that error would stay pending for
  // the next call's hipGetLastError)
  if (k && !main_rec) (void)hipEventRecord(b, ctx->cur);
  if (st) {
    (void)hipEventRecord(sb, ctx->cur);
    ctx->recs.push_back({stage_name, sa, sb});
  }
  if (k) ctx->recs.push_back({name, a, b});
}

// Runs one launch, bracketed by events when profiling is on.
template <typename F>
void timed(bic_ctx* ctx, const char* name, F&& launch) {
  if (!ctx->prof_on || (!ctx->prof_only.empty() && ctx->prof_only != name)) {
    launch();
    return;
  }
  hipEvent_t a = take_event(ctx), b = take_event(ctx);
  (void)hipEventRecord(a, ctx->cur);
  launch();
  (void)hipEventRecord(b, ctx->cur);
  ctx->recs.push_back({name, a, b});
}

inline int bind(bic_ctx* ctx) {
  if (!ctx) return BIC_EINVAL;
  BIC_HIP(hipSetDevice(ctx->device));
  return BIC_OK;
}

// The arena's one gate: every call that uses ctx->scratch takes it here, on ctx->cur.
inline int ensure_scratch(bic_ctx* ctx, size_t bytes) {
  hipStreamCaptureStatus cst = hipStreamCaptureStatusNone;
  if (!ctx->captured && hipStreamIsCapturing(ctx->cur, &cst) == hipSuccess && cst != hipStreamCaptureStatusNone)
    ctx->captured = true;
  ctx->scratch_zero_prev = ctx->scratch_zero;
  ctx->scratch_zero = 0;
  if (bytes <= ctx->scratch_bytes) return BIC_OK;
  ctx->scratch_zero_prev = 0;
  BIC_HIP(hipStreamSynchronize(ctx->cur));  // earlier calls may still use the old arena
  if (ctx->scratch) (void)hipFree(ctx->scratch);
  ctx->scratch = nullptr;
  ctx->scratch_bytes = 0;
  const size_t want = bytes + bytes / 4 + 4096;
  if (hipMalloc(&ctx->scratch, want) != hipSuccess) {
    ctx->scratch = nullptr;
    return BIC_ENOMEM;
  }
  ctx->scratch_bytes = want;
  return BIC_OK;
}

// The context's residual buffer (bic_encode_gray*, bic_encode_pbm* without planes), grown to `need` bytes
inline int ensure_rbuf(bic_ctx* ctx, size_t need) {
  if (ctx->rbuf_bytes >= need) return BIC_OK;
  BIC_HIP(hipStreamSynchronize(ctx->cur));  // earlier calls may still use the old buffer
  if (ctx->rbuf) (void)hipFree(ctx->rbuf);
  ctx->rbuf = nullptr;
  ctx->rbuf_bytes = 0;
  if (hipMalloc(&ctx->rbuf, need) != hipSuccess) return BIC_ENOMEM;
  ctx->rbuf_bytes = need;
  return BIC_OK;
}

// bic_capi_algebra.cpp: the arena bytes one bic_bsvd_learn_lm call takes (from the arena's start)
size_t bsvd_learn_arena_bytes(int lm, size_t n, size_t m, size_t p);

inline bool geom_ok(size_t rows, size_t cols, size_t wpr) {
  if (cols == 0 || rows > 0x7fffffffu || cols > 0x7ffffffeu) return false;
  if (wpr < (cols + 63) / 64 || wpr > 0xffffffffu) return false;
  // the reference's 32-bit coder state (Golomb.h:21-24) is only defined while the sample
  // count and accumulated error stay below 2^31: both are bounded by rows*(cols+1).
  return (unsigned long long)rows * (cols + 1) < 0x80000000ull;
}
