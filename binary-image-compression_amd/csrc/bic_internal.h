// bic_internal.h -- shared between the HIP kernels (bic_kernels.hip) and the C ABI
// (bic_capi*.cpp; the context they share is bic_ctx.h). Not installed; the public surface is include/bic.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace bic {

// Geometry of one batch of planes as the chunk kernels see it. A "chunk" is the unit
// one wavefront processes: up to 64*WPL consecutive words of ONE row (lane l handles
// words c0 + 64*t + l for t < WPL, so every load instruction is 512 contiguous bytes).
struct Geom {
  uint32_t rows, cols, wpr;
  uint32_t used;  // ceil(cols/64): words that hold pixels
  uint32_t wpl;   // words per lane (1, 2 or 4)
  uint32_t wpc;   // words per chunk = 64*wpl
  uint32_t cpr;   // chunks per row = ceil(used/wpc)
  uint32_t nplanes;
  uint64_t trail;             // valid-bit mask of word used-1 (binmat.cpp:146-147)
  uint64_t plane_words;       // rows*wpr
  uint64_t chunks_per_plane;  // rows*cpr
  uint64_t nchunks;           // nplanes*chunks_per_plane
  uint64_t words_used;        // rows*used per plane (word_bits stride)
};

Geom make_geom(size_t rows, size_t cols, size_t wpr, int nplanes);

// Per-call device scratch carved from the context arena.
struct ChunkScratch {
  uint32_t* ones;      // [nchunks]
  int32_t* last;       // [nchunks] last 1-column in the chunk, -1 if none
  int32_t* first;      // [nchunks] first 1-column in the chunk, INT32_MAX if none
  uint32_t* nbase;     // [nchunks] global sample index of the chunk's first 1
  int32_t* jprev;      // [nchunks] column of the last 1 before the chunk in its row, -1
  uint64_t* bits;      // [nchunks] Golomb bits of the chunk
  uint64_t* boff;      // [nchunks] absolute bit offset of the chunk in `out`
  uint32_t* word_bits; // [nplanes*rows*used]
  uint64_t* plane_F;   // [nplanes] raster index of the plane's first residual 1 (~0 if none)
  uint64_t* plane_ones;// [nplanes]
};
size_t chunk_scratch_bytes(const Geom& g);
ChunkScratch carve_chunk_scratch(void* base, const Geom& g);

// Launchers (all asynchronous on `s`). flags[0] = overflow, flags[1] = domain error.
void launch_bitplanes_u8(hipStream_t s, const uint8_t* gray, size_t pitch, uint32_t rows,
                         uint32_t cols, int plane0, int nplanes, uint64_t* planes, uint32_t wpr,
                         bool gray_code = false, int sample_predict = 0);
void launch_count(hipStream_t s, const Geom& g, const uint64_t* planes, int predict,
                  const ChunkScratch& cs, uint64_t* resid, uint64_t* weight_out);
void launch_scan_rows(hipStream_t s, const Geom& g, const ChunkScratch& cs);
// bic_med_residual for rows of <= 256 words: RPW rows per wave, 16-byte loads; part = one u32 per
// wave (scratch, ceil(rows/8) per plane)
bool med_rows_supported(const Geom& g, const void* planes, const void* resid);
// a9 adaptive EG (bic_egad.hip)
size_t egad_scratch_bytes(uint64_t nrows);
// out null: no emission (index only); index (nullable): per row its first bit in the plane's stream and
// the coder state there (bic_egad_row_index)
// nib: egad_build_nib's table in device memory (the context's byte-table buffer, kLutEgadNib)
void launch_egad(hipStream_t s, const uint64_t* planes, uint32_t rows, uint32_t cols, uint32_t wpr, uint32_t nplanes,
                 int predict, uint64_t* out, uint64_t slot, uint64_t* bits, void* scratch, uint32_t* flags,
                 uint64_t* index, const uint64_t* nib);
// the adaptive EG coder's nibble table (976 u64 entries), built on the host
void egad_build_nib(uint64_t* T);
constexpr size_t kLutEgadNib = 3 * 256;         // its offset in the context's byte-table buffer (u64 words)
constexpr size_t kLutEgadDec = kLutEgadNib + 976;  // the decoder's table (992 u64 words)
constexpr size_t kLutWords = kLutEgadDec + 992;    // the whole buffer
// f1 decoders (bic_decode.hip)
bool decode_supported(uint32_t cols);
// bic_decode_gray: the samples the decoded planes (plane b = bit plane0 + b) go to
struct GrayOut {
  uint8_t* gray;
  uint64_t pitch;
  int plane0, bps, big_endian;
  int gray_code = 0;  // BIC_OPT_GRAY_CODE: the planes are G(v)'s, the samples stored are v's
  // bic_decode_gray_frames: the call's planes are nframes groups, group f those of the image at gray + f * frame_stride
  uint32_t nframes = 1;
  uint64_t frame_stride = 0;
  // BIC_OPT_SAMPLE_PREDICT (bps 1): the planes are T(row)'s; the sink stores the z samples and the entry point
  // turns them into v's in place with launch_sample_unpredict, a pass of its own after the decode
  int sample_predict = 0;
};
// bic_decode_rgb: the interleaved R G B samples (one byte each) the decoded planes go to; plane c * np + b
// (np = the call's planes / 3) is bit plane0 + b of channel c
struct RgbOut {
  uint8_t* rgb;
  uint64_t pitch;
  int plane0;
  int gray_code = 0;
  int color_transform = 0;  // BIC_OPT_COLOR_TRANSFORM: the planes are T(pixel)'s, the samples stored the pixel's
  // bic_decode_rgb_frames: the call's planes are nframes groups of 3 np, group f those of the image at rgb + f * frame_stride
  uint32_t nframes = 1;
  uint64_t frame_stride = 0;
  // BIC_OPT_RGB_PREDICT: the planes are T_sp(T_ct(row))'s per channel; the sink then runs with color_transform 0 and
  // stores the z bytes, and the entry point turns them into the pixels in place with launch_rgb_unpredict (the
  // scan and ct_inverse, the transform kept here), a pass of its own after the decode
  int rgb_predict = 0;
  int ct_inverse = 0;
};
// bic_decode_pbm: the P4 rasters the decoded planes go to (plane f = frame f at raster + f * stride)
struct PbmOut {
  uint8_t* raster;
  uint64_t stride;
};
// One decode: the streams, the geometry, and the sink the decoded planes go to.
struct DecodeCall {
  int coder;  // 0 Golomb, 1 EG, 2 adaptive EG
  const uint64_t* streams;
  uint64_t slot;  // > 0: plane p at streams + p * slot; 0: packed, plane p at word_off[p]
  const uint64_t *word_off, *plane_bits, *index;
  const uint8_t* p00;
  uint32_t rows, cols, wpr, nplanes;
  int predict;
  enum { kPlanes, kGray, kPbm, kRgb } sink;
  // the one `sink` names
  uint64_t* planes;
  GrayOut gray;
  PbmOut pbm;
  RgbOut rgb;
  // the context's: its arena (decode_scratch_bytes of this call), its error flags, and egad_build_dec_nib's
  // table in device memory (the context's byte-table buffer, kLutEgadDec)
  void* scratch;
  uint32_t* flags;
  const uint64_t* egnib;
};
// the column totals and the EG first rows; for kGray, kRgb and kPbm also the D buffer (nplanes * rows * wpr
// words) the row kernels write instead of the caller's planes
size_t decode_scratch_bytes(const DecodeCall& c);
void launch_decode(hipStream_t s, const DecodeCall& c);
// the adaptive EG decoder's nibble table (62 states x 16 nibbles, u64), built on the host
void egad_build_dec_nib(uint64_t* T);
void launch_med_rows(hipStream_t s, const Geom& g, const uint64_t* planes, int predict, uint64_t* resid,
                     uint32_t* part, uint64_t* weight_out);
void launch_golomb_bits(hipStream_t s, const Geom& g, const uint64_t* planes, int predict,
                        const ChunkScratch& cs);
void launch_golomb_offsets(hipStream_t s, const Geom& g, const ChunkScratch& cs, uint64_t* out,
                           uint64_t slot_words, uint64_t* plane_bits, uint32_t* flags);
void launch_golomb_emit(hipStream_t s, const Geom& g, const uint64_t* planes, int predict,
                        const ChunkScratch& cs, uint64_t* out, uint64_t slot_words);
void launch_eg_emit(hipStream_t s, const Geom& g, const uint64_t* planes, int predict,
                    const ChunkScratch& cs, uint64_t* out, uint64_t slot_words,
                    uint64_t* plane_bits, uint32_t* flags);

// Sample coder (GolombCoder::codeSample over an array).
struct SampleScratch {
  uint32_t* counter;   // block tickets
  uint64_t* a_rec;     // [nblk] look-back records: sums of samples
  uint64_t* b_rec;     // [nblk] look-back records: codeword bits
  uint64_t* blk_A;     // [nblk] accumulated error before the block
  uint64_t* blk_off;   // [nblk] absolute bit offset of the block
  size_t zero_bytes;   // counter + records, zeroed per launch
};
size_t sample_scratch_bytes(size_t n);
SampleScratch carve_sample_scratch(void* base, size_t n);
// prezeroed: the scratch's counter and records are already 0 (k_tiles_split zeroes them); lpart
// (nullable): nlpart per-block sums added into *lout by the emit launch
void launch_golomb_samples(hipStream_t s, const uint32_t* samples, size_t n, uint64_t n0,
                           uint64_t a0, unsigned bit0, uint64_t* out, size_t cap_words,
                           uint64_t* bits_out, const SampleScratch& ss, uint32_t* flags, bool prezeroed = false,
                           const uint64_t* lpart = nullptr, uint32_t nlpart = 0, uint64_t* lout = nullptr);
// the aligned tile path split over 4 waves per strip (W in 8, 16, 32, 64; else 0 blocks)
uint32_t tiles_split_blocks(uint32_t rows, uint32_t cols, uint32_t W);
void launch_tiles_split(hipStream_t s, const uint64_t* plane, uint32_t rows, uint32_t cols, uint32_t wpr, uint32_t W,
                        const uint64_t* lentab_dev, uint32_t* weights, uint32_t* w_nonpred, uint32_t* w_pred,
                        uint8_t* modes, uint64_t* resid, uint64_t* lpart, uint32_t* zero, uint32_t nzero);

// Tiles (compress7 R = 0 path).
void launch_tiles(hipStream_t s, const uint64_t* plane, uint32_t rows, uint32_t cols,
                  uint32_t wpr, uint32_t W, const uint64_t* lentab_dev, uint32_t* weights,
                  uint32_t* w_nonpred, uint32_t* w_pred, uint8_t* modes, uint64_t* resid,
                  uint64_t* stats);

// Row encoders for rows of at most 256 words: the staged encoder (bic_fused.hip) and the look-back
// encoders (bic_fused_lookback.hip). One encode is a FusedCall handed to the launch functions below.

// The device arena of one call, carved from the context's scratch (n = rows * planes). Its layout is
// fused_layout's walk in bic_fused.hip: the size and the carving both come from it.
struct FusedArena {
  // counter: kZeroWords u32 words in 256 bytes. [0] the look-back encoders' tile ticket, [1] slow_n,
  // [2] the walk list's length, [3] rest_ids', [4] and [5] the k = 0 and k = 1 class lists'; the words from
  // [6] on are unused ([6..10] served experiments whose code was removed)
  uint32_t* counter;
  uint64_t *ones_rec, *bits_rec;  // the look-back records
  uint64_t *gboff, *glen, *gfrag, *gslow, *eboff, *elen, *efrag;
  uint64_t* slow_ids;  // rows k_rows_global must write; their number in *slow_n
  // staged encoder's count pass: per (plane, row, strip) the residual 1-count and the Golomb k
  // statistics record (bic_kstat.h)
  int4* krec;
  uint32_t *kpos, *sones;
  uint32_t* row_o;     // ones of the plane before each row (two-pass / staged encoders)
  uint32_t* walk_ids;  // rows whose Golomb length is walked (k_row_walk)
  uint32_t* rest_ids;  // rows the REST emit launch writes (mixed k, the plane's first 1; counter[3])
  uint32_t* walk_o;    // the walked rows' ones before (row_o), beside the id: the walk loads both at once
  // per plane: packed output's totals of residual 1s and start words / bits, the EG source's one bit to
  // clear after the emission (found by the ONES scan; bic_fused.h eg_fix_bit)
  uint64_t *pones, *gbase, *ebase, *efix;
  // EG source: the LEN scan lists the rows whose codewords all have k = 0 (entries [0 .. counter[4]))
  // and all k = 1 (entries [n ..], counter[5]) for the two class emission kernels, each entry two u64
  // words: the row id | its Golomb length << 32, then its slot-relative Golomb bit offset (gboff's
  // value): 2 n entries in all. The rows of mixed k stay k_emit_rest's
  uint64_t* cls;
  uint64_t* sink;      // 64 words the class kernels' idle lanes store to (a fixed store count)
  uint32_t* slow_n;    // counter + 1: zeroed with the counter
  size_t zero_bytes;   // counter + look-back records: what a look-back encoder needs zero at its start
};
size_t fused_scratch_bytes(const Geom& g);
FusedArena carve_fused_arena(void* base, const Geom& g);
bool fused_supported(const Geom& g);

// One coder's output: nplanes slots of `slot` words from `out`, the planes' bit counts in bits.
// off (packed output, staged encoder): the streams are written word-aligned back to back from word 0
// of `out` (what bic_pack_streams makes of slots) and off[0..nplanes] receive their word offsets.
struct CoderOut {
  uint64_t* out = nullptr;
  uint64_t slot = 0;
  uint64_t *bits = nullptr, *off = nullptr;
};

// What one call asks of the row encoders.
struct FusedRequest {
  CoderOut g, e;  // Golomb, EG; out null: that coder is not wanted
  // row index for the decoders: per row, the bit offset of its first Golomb codeword in its plane's
  // stream and the residual 1s of the plane before it; null: not written. Without g.out
  // (bic_row_index: the staged prefix alone) g.slot still gives the slot the offsets are relative to
  uint64_t* index = nullptr;
  // EG source (bic_encode_gray without planes, slot output): the count pass (launch_gray_rows with
  // out_e) wrote the EG stream in its uniform layout (row r at bit r (cols + 1) + 1) instead of the
  // residual planes; the Golomb kernels read the residual rows back from the stream, and one bit per
  // plane (FusedArena::efix) is cleared after them
  bool eg_src = false;
  bool eg_src_one = false;  // (A/B: the one emission kernel k_emit_known for every class instead)
  bool counted = false;     // the count pass already ran (bic_encode_gray's fused bitplane kernel) ...
  uint32_t ns = 1;          // ... with ns statistics records per row
  bool zero_ready = false;  // (look-back encoders) the previous call's k_fixup left zero_bytes cleared
};

// the staged encoder (prefix kernels, then independent rows; planes 16-byte aligned with an even row
// pitch), the single kernel with decoupled look-backs, the two-pass one
constexpr int kEncStaged = 0, kEncSingle = 1, kEncTwoPass = 2;

struct FusedCall {
  Geom g;
  const uint64_t* planes;
  int predict;
  int mode;  // kEnc*
  FusedRequest rq;
  // the context's: its byte tables (build_byte_lut), its error flags, the arena carved from its scratch
  const uint64_t* lut;
  uint32_t* flags;
  FusedArena ar;
};

// The staged emission's second stream (k_emit_rest then runs beside the main kernel) with its fork /
// join events, null: one stream; and (bic_prof_*) the events recorded on the launch stream around the
// main kernel alone, null: not timed. *main_rec is set when main1 was recorded.
struct EmitStreams {
  hipStream_t aux = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
  hipEvent_t main0 = nullptr, main1 = nullptr;
  bool* main_rec = nullptr;
};

// host: the fused encoder's byte tables -- lut[0..255] 64-bit entries for k = 3, then (as u32)
// [2][256] packed entries for k = 1, 2 (bic_fused.h encode_word); 4 KiB
void build_byte_lut(uint64_t* lut);
// The launches of one encode, in order (all asynchronous on `s`):
// look-back encoders: zero the tile ticket and the records, unless rq.zero_ready
void launch_lookback_clear(hipStream_t s, const FusedCall& c);
// staged: the count pass unless rq.counted, the ONES scan, then -- with golomb_lengths -- the walk of
// the mixed-k rows and the LEN scan (+ the row index), and the packed planes' bases
void launch_staged_prefix(hipStream_t s, const FusedCall& c, bool golomb_lengths);
// staged: k_emit_rest (on es.aux, forked from and joined back into s) and the main emission kernel
void launch_staged_emit(hipStream_t s, const FusedCall& c, const EmitStreams& es);
// look-back encoders: the single kernel (kEncSingle) or the length and emission passes (kEncTwoPass)
void launch_lookback_rows(hipStream_t s, const FusedCall& c);
// every encoder: the LDS-overflow rows (k_rows_global) and the words adjacent rows share (k_fixup)
void launch_fused_finish(hipStream_t s, const FusedCall& c);
// the staged encoder's count passes also zero its kZeroWords counters (no separate fill launch)
constexpr uint32_t kZeroWords = 64;
void launch_row_ones(hipStream_t s, const Geom& g, const uint64_t* planes, int predict, uint32_t* sones,
                     int4* krec, uint32_t* kpos, uint32_t* zero);
// P4 rasters -> planes + the count pass in one read (bic_encode_pbm): frame f (g.rows x ceil(cols/8) bytes at
// raster + f * stride, any alignment) is plane f; one record per row (ns = 1). dst (med_rows_supported)
// receives the planes, or with store_resid and predict their med residual
void launch_pbm_rows(hipStream_t s, const uint8_t* raster, uint64_t stride, const Geom& g, int predict, uint64_t* dst,
                     bool store_resid, uint32_t* sones, int4* krec, uint32_t* kpos, uint32_t* zero);
// bitplanes + the count pass in one read of the gray image (bic_encode_gray); gray_strips(g)
// k statistics records per row (one per 64-word strip)
bool gray_rows_supported(const Geom& g, const void* gray, size_t pitch, const void* planes, int bps = 1);
uint32_t gray_strips(const Geom& g);
// store_resid: the words stored are the med residual R (planes = the caller's bitplanes are not
// wanted; the encoder then reads R with predict off), not the bitplanes P. out_e (with predict, the
// bitplanes not wanted): the EG stream instead of R (FusedRequest::eg_src; slots of eg_stride
// words); planes is then unused. bps = 2 (bic_encode_gray16): samples of two bytes, big-endian
// (pnm.cpp:71-74) or the host's order, planes plane0 .. of 16 (k_gray_strips16). bps = 3 (bic_encode_rgb):
// interleaved RGB pixels of one-byte samples; g.nplanes = 3 np, output plane c * np + k is plane plane0 + k
// of channel c (k_gray_strips_rgb; color_transform: BIC_OPT_COLOR_TRANSFORM, bps = 3 only).
// sample_predict: BIC_OPT_SAMPLE_PREDICT (bps = 1), BIC_OPT_RGB_PREDICT (bps = 3: per channel, behind color_transform)
void launch_gray_rows(hipStream_t s, const uint8_t* gray, size_t pitch, const Geom& g, int predict, int plane0,
                      uint64_t* planes, uint32_t* sones, int4* krec, uint32_t* kpos, uint32_t* zero,
                      bool store_resid = false, uint64_t* out_e = nullptr, uint64_t eg_stride = 0, int bps = 1,
                      int big_endian = 0, bool gray_code = false, int color_transform = 0, int sample_predict = 0);
// the count pass can write the EG stream (FusedRequest::eg_src): rows of whole 64-word strips only
bool gray_eg_supported(const Geom& g);
// launch_gray_rows for nframes images of one-byte samples in one launch (bic_encode_gray_frames): frame f at
// gray + f * frame_stride, g.nplanes = nframes x one frame's planes, output plane f * (g.nplanes / nframes) + k
// = plane plane0 + k of frame f (k_gray_strips_frames). gray_frames_supported: its grid fits 31 bits
bool gray_frames_supported(const Geom& g, uint64_t nframes, int predict, bool store_resid);
void launch_gray_frames(hipStream_t s, const uint8_t* gray, size_t pitch, uint64_t frame_stride, uint32_t nframes,
                        const Geom& g, int predict, int plane0, uint64_t* planes, uint32_t* sones, int4* krec,
                        uint32_t* kpos, uint32_t* zero, bool store_resid, uint64_t* out_e, uint64_t eg_stride,
                        bool gray_code, int sample_predict = 0);
// launch_gray_rows' bps = 3 form for nframes interleaved RGB images in one launch (bic_encode_rgb_frames): frame f at
// rgb + f * frame_stride, g.nplanes = nframes x 3 x one channel's planes np, output plane (f * 3 + c) * np + k = plane
// plane0 + k of channel c of frame f (k_gray_strips_rgb_frames). rgb_frames_supported: its grid fits 31 bits
bool rgb_frames_supported(const Geom& g, uint64_t nframes, int predict, bool store_resid);
void launch_rgb_frames(hipStream_t s, const uint8_t* rgb, size_t pitch, uint64_t frame_stride, uint32_t nframes,
                       const Geom& g, int predict, int plane0, uint64_t* planes, uint32_t* sones, int4* krec,
                       uint32_t* kpos, uint32_t* zero, bool store_resid, uint64_t* out_e, uint64_t eg_stride,
                       bool gray_code, int color_transform, int rgb_predict = 0);

void launch_patch_search(hipStream_t s, const uint64_t* plane, uint32_t rows, uint32_t cols, uint32_t wpr,
                         uint32_t W, uint32_t* besti, uint32_t* bestj, uint32_t* bestd);

// compress7_test.cpp:117-275 with a search window (bic_match.hip). The plane I is modified in
// place. Per-tile outputs left null are carved from the scratch by launch_match_tiles.
struct MatchArgs {
  uint64_t* I;
  uint32_t rows, cols, wpr, used, W, nx, ny, T;
  int R;
  uint32_t G;                       // tile schedule: workgroups per tile
  uint32_t H, K;                    // team schedule: helpers per tile row; tiles of slack
  const double* enuml;              // device, W*W+1
  uint32_t* counter;                // scratch: ticket
  unsigned long long* key;          // scratch: per tile min key
  uint32_t* done;                   // scratch: per tile
  uint32_t* arrive;                 // scratch: per tile
  uint32_t* lens;                   // scratch: per tile chosen length
  uint32_t *besti, *bestj, *bestd, *weights;
  uint8_t* modes;
  uint32_t* flags;
  uint32_t inv;                     // compress8_test.cpp's patch inversion (0: compress7_test.cpp)
  uint8_t* inverted;                // per tile: the patch was flipped (nullable)
  // the loop of compress4_test.cpp (4), compress5_test.cpp (5), compress6_test.cpp (6); 0: compress7/8
  // (per-tile schedule only)
  uint32_t var;
  unsigned long long* key2;         // scratch, variant 5: per tile the first window with d < W*W/2
};
constexpr uint32_t kSchedTiles = 0, kSchedRows = 1, kSchedTeam = 2;
struct MatchSched {
  uint32_t kind, G, H, K;
};
// code: 0 auto; 1..256 workgroups per tile; 0x10000 | H a team of 1 + H workgroups per tile row;
// anything else: per-tile workgroups, count from W and R
// var (MatchArgs::var) != 0: per-tile workgroups only; rows bounds the region for the automatic count
MatchSched match_schedule(uint32_t W, uint32_t R, uint32_t cols, uint32_t code, uint32_t var = 0, uint32_t rows = 0);
size_t match_scratch_bytes(size_t ntiles, const MatchSched& m);
void launch_match_tiles(hipStream_t s, MatchArgs& a, const MatchSched& m, void* scratch);
void launch_match_code(hipStream_t s, const MatchArgs& a, unsigned long long* out_m, unsigned long long* out_n,
                       size_t cap_words, uint64_t* stats);
void launch_pbm(hipStream_t s, bool pack, const uint8_t* raster_in, uint8_t* raster_out, const uint64_t* plane_in,
                uint64_t* plane_out, uint32_t rows, uint32_t cols, uint32_t wpr);
// P5 samples (1 or 2 bytes, any alignment) -> planes plane0.. (bic_raster.hip); pitch: bytes per row
// (0: cols * bpp, a P5 raster); big_endian: the order of two-byte samples (1: pnm.cpp:73);
// color_transform: BIC_OPT_COLOR_TRANSFORM (bpp / bps = 3 only)
void launch_raster_planes(hipStream_t s, const uint8_t* raster, int bpp, uint32_t rows, uint32_t cols, int plane0,
                          int nplanes, uint64_t* planes, uint32_t wpr, uint64_t pitch = 0, int big_endian = 1,
                          bool gray_code = false, int color_transform = 0, int sample_predict = 0);
void launch_planes_gray(hipStream_t s, const uint64_t* planes, uint32_t rows, uint32_t cols, uint32_t wpr, int plane0,
                        int nplanes, int bps, uint8_t* gray, uint64_t pitch, bool gray_code = false,
                        int color_transform = 0);
// BIC_OPT_SAMPLE_PREDICT on the way back, in place on the one-byte z samples launch_planes_gray or the gray
// decoder sink stored (k_sample_unpredict: a wave per row of each frame; 0: no launch). Only the rows' first
// `cols` bytes are touched.
void launch_sample_unpredict(hipStream_t s, int sample_predict, uint8_t* gray, uint64_t pitch, uint64_t frame_stride,
                             uint32_t nframes, uint32_t rows, uint32_t cols);
// BIC_OPT_RGB_PREDICT on the way back, in place on the interleaved z bytes launch_planes_gray (bps 3) or the RGB
// decoder sink stored with color_transform 0 (k_rgb_unpredict: the per-channel scan, then the inverse colour
// transform; 0: no launch). Only the rows' first 3 * cols bytes are touched.
void launch_rgb_unpredict(hipStream_t s, int rgb_predict, int color_transform, uint8_t* rgb, uint64_t pitch,
                          uint64_t frame_stride, uint32_t nframes, uint32_t rows, uint32_t cols);

// GF(2) algebra (bic_gf2.hip). Both launches spread their rows over gridDim.y (at most 65,535): the transpose
// four 64-row blocks per unit, the product 256 rows per unit, so either takes at most kGf2MaxRows source rows
// (rows of A for the product); a caller with more rows launches them in chunks of that many (a multiple of 64)
constexpr uint32_t kGf2MaxRows = 65535u * 256u;
void launch_gf2_transpose(hipStream_t s, const uint64_t* src, uint32_t s_rows, uint32_t s_stride, uint32_t s_words,
                          uint32_t ncols_out, uint64_t* dst, uint32_t d_stride, uint32_t d_words);
void launch_gf2_ab(hipStream_t s, const uint64_t* A, uint32_t M, uint32_t a_stride, uint32_t kbits, const uint64_t* B,
                   uint32_t b_stride, uint32_t nw, uint64_t* C, uint32_t c_stride, uint32_t nset);

// Binary dictionary learning (bic_bsvd.hip). All matrices in the plane layout; m, p in 1 .. 4096.
// changed (device u64) is added to, not written: the caller zeroes it. launch_bsvd_coef takes a null one;
// launch_bsvd_dict_atoms does not (k_bsvd_dict adds to it unconditionally: bsvd_dict in bic_capi_algebra.cpp puts a
// word of the arena in a null pointer's place).
void launch_bsvd_coef(hipStream_t s, uint64_t* E, uint32_t n, uint32_t m, uint32_t e_wpr, const uint64_t* D,
                      uint32_t p, uint32_t d_wpr, uint64_t* A, uint32_t a_wpr, uint64_t* changed);
// the dictionary update's arena: kBsvdDictHead bytes (u32 U, ticket, flag at 0; the 4,096 column counts
// at 64; delta's 64 words after them; at kBsvdDictCounts three u64: the learn loop's two counts and the
// stand-in for a null `changed`), then the transpose of A
constexpr size_t kBsvdDictCounts = 64 + 64 * 64 * 4 + 64 * 8, kBsvdDictHead = 17408;
size_t bsvd_dict_scratch_bytes(uint32_t n, uint32_t p);
uint32_t bsvd_dict_blocks(uint32_t n);  // 1: one workgroup walks the atoms in one launch
// the zeroed counters and the transpose of A (in row chunks of kGf2MaxRows); then the atoms k_lo .. k_hi
// (k = p: the last atom's change alone) in one launch: 0 .. p when bsvd_dict_blocks(n) is 1, else one atom per launch, in order; n >= 1
void launch_bsvd_dict_prepare(hipStream_t s, uint32_t n, uint32_t p, const uint64_t* A, uint32_t a_wpr, void* scratch);
void launch_bsvd_dict_atoms(hipStream_t s, uint64_t* E, uint32_t n, uint32_t m, uint32_t e_wpr, uint64_t* D,
                            uint32_t p, uint32_t d_wpr, void* scratch, uint32_t k_lo, uint32_t k_hi,
                            uint64_t* changed);
void launch_bsvd_xor(hipStream_t s, uint64_t* E, uint32_t n, uint32_t m, uint32_t e_wpr, const uint64_t* X,
                     uint32_t x_wpr);
// PROXIMUS (bsvd.cpp:530-735) after launch_bsvd_dict_prepare: round r of atom k's budget is the atom-half
// launch and then the coefficient-half launch. check_prev: atom k - 1 was enqueued before with `budget`
// rounds (its stall is noted here); fresh: atom k's first round of this call (false when a stalled atom is
// enqueued again). k = p in launch_bsvd_prox_atom only notes atom p - 1's stall. The schedule's words are the
// u32 of the arena's first 64 bytes: kBsvdProxStalled (atom + 1, or 0), u64 rounds at kBsvdProxRounds, u64
// atoms changed at kBsvdProxChanged (byte offsets).
constexpr size_t kBsvdProxStalled = 20, kBsvdProxRounds = 32, kBsvdProxChanged = 48;
void launch_bsvd_prox_atom(hipStream_t s, uint64_t* E, uint32_t n, uint32_t m, uint32_t e_wpr, uint64_t* D,
                           uint32_t p, uint32_t d_wpr, void* scratch, uint32_t k, uint32_t r, uint32_t budget,
                           bool check_prev, bool fresh);
void launch_bsvd_prox_coef(hipStream_t s, uint64_t* E, uint32_t n, uint32_t m, uint32_t e_wpr, const uint64_t* D,
                           uint32_t d_wpr, uint64_t* A, uint32_t a_wpr, void* scratch, uint32_t k, uint32_t r);
void launch_bsvd_prox_clear_stall(hipStream_t s, void* scratch);
// The model initialisers (bsvd.cpp:99-267), mi one of BIC_BSVD_MI_*: A cleared (and set from sel for the two
// centroid rules), every atom's first ceil(m/64) words written. sel (device): p pick rows (NEIGHBOR), n atom
// indices (CENTROIDS, CENTROIDS_XOR), unused for PARTITION; an index out of range is skipped, never
// dereferenced. n >= 1. The arena holds bsvd_init_scratch_bytes: the counters, which the call clears first, and
// after them (bsvd_init_scratch_tail) room for max(n, p) u32 that bic_bsvd_initialize fills: the indices it
// draws, before that the bitmap of launch_bsvd_init_nonzero (bit 63 - i % 64 of word i / 64: row i != 0 over j < m).
size_t bsvd_init_scratch_bytes(uint32_t n, uint32_t m, uint32_t p);
void* bsvd_init_scratch_tail(void* scratch, uint32_t m, uint32_t p);
void launch_bsvd_init(hipStream_t s, int mi, const uint64_t* E, uint32_t n, uint32_t m, uint32_t e_wpr, uint64_t* D,
                      uint32_t p, uint32_t d_wpr, uint64_t* A, uint32_t a_wpr, const uint32_t* sel, void* scratch);
void launch_bsvd_init_nonzero(hipStream_t s, const uint64_t* E, uint32_t n, uint32_t m, uint32_t e_wpr,
                              uint64_t* bitmap);
// The same three steps for rows of any width, m in 1 .. 1,048,576 (bic_bsvd_wide.hip), with the narrow
// launchers' arguments. The arena is the narrow dictionary update's plus a flag per atom
// (bsvd_wide_scratch_bytes); launch_bsvd_wide_prepare stands for launch_bsvd_dict_prepare, and
// launch_bsvd_wide_dict walks all p atoms and adds the atoms changed to *changed (not null). n >= 1.
size_t bsvd_wide_scratch_bytes(uint32_t n, uint32_t p);
void launch_bsvd_wide_coef(hipStream_t s, uint64_t* E, uint32_t n, uint32_t m, uint32_t e_wpr, const uint64_t* D,
                           uint32_t p, uint32_t d_wpr, uint64_t* A, uint32_t a_wpr, uint64_t* changed);
void launch_bsvd_wide_prepare(hipStream_t s, uint32_t n, uint32_t p, const uint64_t* A, uint32_t a_wpr,
                              void* scratch);
void launch_bsvd_wide_dict(hipStream_t s, uint64_t* E, uint32_t n, uint32_t m, uint32_t e_wpr, uint64_t* D,
                           uint32_t p, uint32_t d_wpr, void* scratch, uint64_t* changed);
void launch_bsvd_wide_prox_atom(hipStream_t s, uint64_t* E, uint32_t n, uint32_t m, uint32_t e_wpr, uint64_t* D,
                                uint32_t p, uint32_t d_wpr, void* scratch, uint32_t k, uint32_t r, uint32_t budget,
                                bool check_prev, bool fresh);
void launch_bsvd_wide_prox_coef(hipStream_t s, uint64_t* E, uint32_t n, uint32_t m, uint32_t e_wpr, const uint64_t* D,
                                uint32_t d_wpr, uint64_t* A, uint32_t a_wpr, void* scratch, uint32_t k, uint32_t r);
// The MDL model-order searches' device side (bic_bsvd_mdl.hip), m in 1 .. 1,048,576, p <= 4096, n >= 1. Every read
// of E, D and A is masked at the row's last word. launch_bsvd_mdl_weights: *we = |E|, wd[k] = |D_k|, wa[k] = the
// users of atom k (p = 0: we alone, D and A not dereferenced). launch_bsvd_mdl_drop_weights: score[k] =
// |E ^ A_k^t D_k| for k < p, p >= 1; scratch holds bsvd_mdl_drop_scratch_bytes. launch_bsvd_mdl_drop_atom takes row k
// out of D and column k out of A in place (k < p), launch_bsvd_mdl_append_atom adds row p and column p (the caller
// has room for them). launch_bsvd_mdl_copy: dst = src, rows x words.
void launch_bsvd_mdl_weights(hipStream_t s, const uint64_t* E, uint32_t n, uint32_t m, uint32_t e_wpr, const uint64_t* D,
                             uint32_t p, uint32_t d_wpr, const uint64_t* A, uint32_t a_wpr, uint64_t* we, uint32_t* wd,
                             uint32_t* wa);
size_t bsvd_mdl_drop_scratch_bytes();
void launch_bsvd_mdl_drop_weights(hipStream_t s, const uint64_t* E, uint32_t n, uint32_t m, uint32_t e_wpr,
                                  const uint64_t* D, uint32_t p, uint32_t d_wpr, const uint64_t* A, uint32_t a_wpr,
                                  uint64_t* score, void* scratch);
void launch_bsvd_mdl_drop_atom(hipStream_t s, uint64_t* D, uint32_t p, uint32_t m, uint32_t d_wpr, uint64_t* A,
                               uint32_t n, uint32_t a_wpr, uint32_t k);
void launch_bsvd_mdl_append_atom(hipStream_t s, uint64_t* D, uint32_t p, uint32_t m, uint32_t d_wpr, uint64_t* A,
                                 uint32_t n, uint32_t a_wpr, const uint64_t* atom, const uint64_t* coefs,
                                 uint32_t c_wpr);
void launch_bsvd_mdl_copy(hipStream_t s, uint64_t* dst, uint32_t d_wpr, const uint64_t* src, uint32_t s_wpr,
                          uint32_t rows, uint32_t words);

// The driver's image mode (bic_patch.hip), one launch each: the W x W tiles of a plane as the rows of X (the plane
// read with get_submatrix's flat word indexing, 1 <= W <= 1024), the rows of X back as tiles (every own word of
// the plane written, zero padding), and render_mosaic's image of D (n rows as w x w tiles, gn tiles across, a
// one-pixel gutter; every own word of the irows x icols image written).
void launch_patches_gather(hipStream_t s, const uint64_t* plane, uint32_t rows, uint32_t cols, uint32_t wpr, uint32_t W,
                           uint64_t* X, uint32_t x_wpr);
void launch_patches_scatter(hipStream_t s, const uint64_t* X, uint32_t x_wpr, uint32_t W, uint64_t* plane,
                            uint32_t rows, uint32_t cols, uint32_t wpr);
void launch_mosaic(hipStream_t s, const uint64_t* D, uint32_t n, uint32_t d_wpr, uint32_t w, uint32_t gn, uint32_t irows,
                   uint32_t icols, uint64_t* image, uint32_t i_wpr);

// The growing-dictionary tile coder of compress2_test.cpp:79-129 / compress3_test.cpp:87-149 (bic_dict.hip).
// The plane is only read. Everything below `arena` is carved from the scratch by dict_carve, which also
// puts arena arrays in the place of null per-tile outputs.
struct DictArgs {
  const uint64_t* I;
  uint32_t rows, cols, wpr, used, W, nx, ny, T;
  uint32_t step;                    // atom k's window is at pixel (i * step, j * step) of its tile (i, j)
  uint32_t variant;                 // 2 or 3
  double h;                         // 0.5 log2(W*W) (variant 2) or 0 (variant 3)
  const double* enuml;              // device, W*W+1
  uint32_t *bestk, *bestd, *dsize, *weights;
  uint8_t *modes, *joined;
  uint32_t* dict_tiles;
  // arena
  uint64_t* state;                  // [0] |D|, [1] L, [2] matches
  unsigned long long* keys;         // per tile (distance << 32) | atom: the running first argmin
  uint64_t *P, *Q;                  // per tile W words: its rows, its atom window's rows (Q = P when step = W)
  uint32_t* wt;                     // per tile weight
  uint64_t* nml;                    // per tile nomatch_len
  uint32_t* lens;                   // per tile chosen length (the sample coder's input)
  uint32_t* noflags;                // stand-in for the context's flags when no stream is written
};
size_t dict_scratch_bytes(size_t ntiles, uint32_t W);
void dict_carve(DictArgs& a, void* scratch);
// tiles resolved per block: code 0 = automatic, else code, at most what the resolve kernel's LDS holds
uint32_t dict_block_tiles(uint32_t W, uint32_t code);
void launch_dict_gather(hipStream_t s, const DictArgs& a);
// the block's tiles t0 .. t0 + bn against the atoms in the dictionary (none when t0 = 0: no launch)
void launch_dict_dist(hipStream_t s, const DictArgs& a, uint32_t t0, uint32_t bn);
void launch_dict_resolve(hipStream_t s, const DictArgs& a, uint32_t t0, uint32_t bn);
void launch_dict_finish(hipStream_t s, const DictArgs& a, uint64_t* stats);

// Byte fill by a kernel (every device-side memset of the library): hipMemsetAsync enqueued under stream
// capture replays wrongly on this ROCm (the first captured memset of a process zeroed 800 of 1,280 bytes,
// tools/capture_memset_probe.py), and the encoders' calls are meant to be capturable
void launch_fill(hipStream_t s, void* dst, int value, size_t bytes);
void launch_pack(hipStream_t s, const uint64_t* slots, int nplanes, size_t slot_words,
                 const uint64_t* plane_bits, uint64_t* dst, uint64_t* word_off);

}  // namespace bic
