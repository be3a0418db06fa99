/*
 * bic.h -- C ABI of the MI355X (gfx950) hot path of nacho-pancho/binary-image-compression:
 *          bitplane extraction -> med (3-neighbour XOR) prediction -> per-row zero runs
 *          -> adaptive Golomb (GolombCoder) / "EG" run-length (EGCoder) coding.
 *
 * Plain pointers and sizes only; no C++ or torch types. Every bulk pointer is a DEVICE
 * pointer (hipMalloc'd or any device allocation of the caller); the caller allocates every
 * output (the reference's convention "C is assumed to have been allocated",
 * binmat.cpp:462). Calls enqueue on the context's stream and return immediately;
 * bic_sync() waits and reports deferred errors (e.g. an output slot that was too small).
 *
 * Plane layout = the reference's binary_matrix storage (binmat.h:8-19, 114-141): rows x wpr
 * uint64 words, row-major, column j in word j/64 at bit 63 - j%64 (MSB = leftmost pixel),
 * wpr >= ceil(cols/64). Bits past `cols` are ignored on input and written 0 on output.
 * Several planes are stored back to back (plane p at planes + p*rows*wpr).
 *
 * Encoded streams (build-defined container): one stream per plane, MSB-first
 * bit order, stored as big-endian 64-bit words (so the bytes in memory ARE the bit stream),
 * zero-padded to a 64-bit boundary. Plane p's stream starts at out + p*slot_words.
 *
 * Reference interface each entry replaces is cited per function (file:line under /root/reference/src).
 * Error codes: 0 = OK; never exceptions (style of pbm.h:8-16 ErrorCode).
 */
#ifndef BIC_H
#define BIC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BIC_OK 0
#define BIC_EINVAL 1   /* bad argument (the reference asserts, e.g. binmat.cpp:465-469, GolombCoder.cpp:14) */
#define BIC_ENOMEM 2   /* device allocation failed */
#define BIC_EDEVICE 3  /* HIP runtime error */
#define BIC_ENOSPC 4   /* an output slot was too small (reported by bic_sync) */
#define BIC_ENODEV 5   /* no usable gfx950 device */
#define BIC_EDATA 6    /* a decoder met a malformed stream (reported by bic_sync) */

#define BIC_CODER_GOLOMB 0 /* GolombCoder::codeSample over the run samples (GolombCoder.cpp:29-34) */
#define BIC_CODER_EG 1     /* EGCoder::codeRun as written: incBlockSize disabled (eg.cpp:20-37) */
/* EGCoder::codeRun as intended: incBlockSize() per full block (eg.cpp:25 uncommented) -- the JPEG-LS
 * run mode the #if 0 decoder (eg.cpp:41-55) reads; EGLUT's index saturates at 31. bic_encode_planes
 * only (slots as for Golomb: bic_encode_slot_words). */
#define BIC_CODER_EG_ADAPTIVE 2

typedef struct bic_ctx bic_ctx;

/* ---- context ----------------------------------------------------------------------------- */
int bic_ctx_create(int device, bic_ctx** out);
int bic_ctx_destroy(bic_ctx* ctx);
/* Enqueue on an external hipStream_t (e.g. torch's current stream); NULL is the HIP null
 * (legacy default) stream. A new ctx enqueues on its own non-blocking stream, which
 * bic_ctx_own_stream returns. A ctx's scratch arena and residual buffer (bic_encode_gray) are
 * shared by all its calls, whatever stream is bound: calls enqueued on two different streams must
 * not run concurrently (use one ctx per stream). */
int bic_ctx_set_stream(bic_ctx* ctx, void* hip_stream);
void* bic_ctx_get_stream(bic_ctx* ctx);
void* bic_ctx_own_stream(bic_ctx* ctx);
/* Wait for all work enqueued by this ctx; returns BIC_ENOSPC if an encode since the last
 * sync overflowed its slot (that plane's stream is then incomplete), else BIC_OK/BIC_EDEVICE. */
int bic_sync(bic_ctx* ctx);
const char* bic_strerror(int code);
int bic_device_count(int* n);
/* Device memory for callers without a runtime of their own (the C++ reference-API layer,
 * ctypes/cgo bindings). bic_malloc/bic_free act on the ctx's device; the copies are ordered
 * on the ctx stream and return after the copy has completed (host buffers are pageable). */
int bic_malloc(bic_ctx* ctx, size_t bytes, void** dptr);
int bic_free(bic_ctx* ctx, void* dptr);
int bic_memcpy_h2d(bic_ctx* ctx, void* dst, const void* src, size_t bytes);
int bic_memcpy_d2h(bic_ctx* ctx, void* dst, const void* src, size_t bytes);
int bic_memset(bic_ctx* ctx, void* dst, int value, size_t bytes);
/* Pre-grow the ctx scratch so later calls do not allocate (needed before stream capture). */
int bic_reserve(bic_ctx* ctx, int nplanes, size_t rows, size_t cols);
/* Options: BIC_OPT_MULTIPASS = 1 forces the multi-pass chunk kernels for every geometry
 * (cross-checking the row encoders); 0 (default) picks a row encoder where it applies. */
#define BIC_OPT_MULTIPASS 1
/* Row encoders (same output; the alternatives are kept as cross-checks and for comparison).
 * Default: the staged encoder -- per-row sample counts, per-plane scans and per-row Golomb
 * lengths first, then every row written independently -- for batches of >= 32768 rows (all
 * planes; planes 16-byte aligned, even row pitch), the single kernel below that (fewer launches).
 * BIC_OPT_STAGED = 1: the staged encoder for every batch size. BIC_OPT_TWO_PASS = 1: lengths and
 * offsets found by decoupled look-backs, then every row written. BIC_OPT_SINGLE_KERNEL = 1: one
 * kernel, rows staged in LDS until decoupled look-backs give their offsets. */
#define BIC_OPT_TWO_PASS 2
#define BIC_OPT_SINGLE_KERNEL 3
#define BIC_OPT_STAGED 4
/* BIC_OPT_ONE_STREAM = 1: the staged encoder's two emission launches run one after the other on
 * the ctx stream instead of side by side on a second stream (same output; a test hook for the
 * launch ordering). */
#define BIC_OPT_ONE_STREAM 5
/* BIC_OPT_EG_SOURCE = 0: bic_encode_gray* without planes stores the med residual planes in a ctx
 * buffer for the encoder (the round-3 path) instead of writing the EG stream from the count pass
 * and reading the residual rows back from it (default 1, slot output with the EG coder; same
 * streams: a cross-check and A/B hook); 2: the EG source with one emission kernel for every row
 * class instead of one per class (A/B hook). */
#define BIC_OPT_EG_SOURCE 6
/* BIC_OPT_GRAY_CODE = 1: binary-reflected Gray coding of the samples before they are split into
 * planes, G(v) = v ^ (v >> 1) on the whole sample (8 or 16 bits): a smooth ramp crossing 127 -> 128
 * flips one plane instead of eight. 0 (default): the natural binary code, every call as it was. Any
 * other value is BIC_EINVAL and leaves the setting as it was.
 *  - Samples to planes (bic_bitplanes_u8, _u8_range, _u16, bic_pgm_bitplanes, bic_encode_gray, _range,
 *    _packed, bic_encode_gray16, _packed): output plane b is bit plane0 + b of G(v); planes, streams,
 *    bit counts, offsets and the row index equal those of the same call with the option off on an image
 *    whose samples are G(v). For 16-bit samples bit 7 of G is v7 ^ v8, whatever the range.
 *  - Planes to samples (bic_planes_to_gray, bic_decode_gray): the sample assembled from the given
 *    planes (bits no plane covers taken as 0) goes through the inverse, v_b = XOR of g_k over k >= b,
 *    and is then masked to the bits the planes cover. The covered bits are the image's own exactly when
 *    the range reaches up to the highest non-zero plane of G: dropping low planes is allowed, dropping
 *    high ones is not invertible.
 * Calls that take or return planes only (bic_encode_planes*, bic_decode_planes, the PBM calls) are
 * untouched. */
#define BIC_OPT_GRAY_CODE 7
/* BIC_OPT_COLOR_TRANSFORM: a reversible per-pixel colour transform T in front of the RGB bitplane split,
 * on one-byte samples. BIC_CT_NONE (0, default): none, every call as it was. BIC_CT_SUBTRACT_GREEN (1):
 * R' = (R - G) mod 256, G' = G, B' = (B - G) mod 256. BIC_CT_SUBTRACT_GREEN_FOLDED (2): the same
 * differences, each read as a signed 8-bit d and folded with z = ((d << 1) ^ (d >> 7)) & 0xFF (arithmetic
 * shift: 0 -> 0, -1 -> 1, 1 -> 2, -128 -> 255; inverse d = (z >> 1) ^ -(z & 1)), so that a difference
 * hovering around 0 stays in the low planes. Both are bijections on (R, G); G is never changed. Any other
 * value is BIC_EINVAL and leaves the setting as it was.
 *  - Samples to planes (bic_encode_rgb, bic_encode_rgb_packed, bic_bitplanes_rgb): T, then the Gray code
 *    if BIC_OPT_GRAY_CODE is on (per channel), then the plane0 shift and the split. Planes, streams, bit
 *    counts, offsets and the row index equal those of the same call with the option off on the image T(img).
 *  - Planes to samples (bic_planes_to_rgb, bic_decode_rgb): the three channel samples R', G', B' are
 *    assembled from the given planes (bits no plane covers count as 0, after the un-Gray step and its
 *    mask); then R = (unfold(R') + G') & 0xFF and B likewise (unfold = identity in mode 1), G = G' as
 *    assembled, and all eight bits of the result are written. The result is the image exactly when
 *    plane0 = 0 and nplanes = 8; for any other range it is this formula.
 * The gray, 16-bit, PBM and planes-only calls ignore the option. */
#define BIC_OPT_COLOR_TRANSFORM 8
#define BIC_CT_NONE 0
#define BIC_CT_SUBTRACT_GREEN 1
#define BIC_CT_SUBTRACT_GREEN_FOLDED 2
/* BIC_OPT_SAMPLE_PREDICT: left-neighbour prediction T of one-byte gray samples in front of the bitplane split, so
 * that a smooth row leaves its high planes empty. BIC_SP_NONE (0, default): none, every call as it was.
 * BIC_SP_LEFT (1): d(i,j) = (v(i,j) - v(i,j-1)) mod 256, with v(i,-1) = 0 in every row of every frame.
 * BIC_SP_LEFT_FOLDED (2): the same d, read as a signed 8-bit value and folded as BIC_CT_SUBTRACT_GREEN_FOLDED
 * folds its differences, z = ((d << 1) ^ (d >> 7)) & 0xFF (0 -> 0, -1 -> 1, 1 -> 2, -128 -> 255; inverse
 * d = (z >> 1) ^ -(z & 1)). Both are bijections on a row. Any other value is BIC_EINVAL and leaves the setting
 * as it was.
 *  - Samples to planes, one-byte samples only (bic_bitplanes_u8, _u8_range, bic_pgm_bitplanes with maxval < 256,
 *    bic_encode_gray, _range, _packed, bic_encode_gray_frames, _packed with sample_bytes = 1): T, then the Gray
 *    code if BIC_OPT_GRAY_CODE is on, then the plane0 shift and the split. Planes, streams, bit counts, packed
 *    offsets and the row index equal those of the same call with the option off on the image T(img).
 *  - Planes to samples (bic_planes_to_gray, bic_decode_gray, bic_decode_gray_frames, each with sample_bytes = 1):
 *    the sample z is assembled from the given planes as with the option off (bits no plane covers count as 0,
 *    then the un-Gray step and its mask), unfolded in mode 2 to d, then v(j) = (v(j-1) + d(j)) & 0xFF along the
 *    row from v(-1) = 0, and all eight bits of the result are written (a pass of its own over the stored rows'
 *    first cols bytes; pitch padding and the gap between frames keep the caller's bytes). The result is the
 *    image exactly when plane0 = 0 and nplanes = 8; for any other range it is this formula.
 * Two-byte samples (bic_bitplanes_u16, bic_encode_gray16*, sample_bytes = 2, bic_pgm_bitplanes with maxval >= 256),
 * the RGB calls, the PBM calls and the planes-only calls ignore the option. */
#define BIC_OPT_SAMPLE_PREDICT 9
#define BIC_SP_NONE 0
#define BIC_SP_LEFT 1
#define BIC_SP_LEFT_FOLDED 2
/* BIC_OPT_RGB_PREDICT: the same left-neighbour prediction T_sp on each channel of the RGB calls, behind the colour
 * transform T_ct of BIC_OPT_COLOR_TRANSFORM and in front of the Gray code. Values BIC_SP_NONE (0, default: every
 * call as it was), BIC_SP_LEFT (1), BIC_SP_LEFT_FOLDED (2); any other value is BIC_EINVAL and leaves the setting as
 * it was. An option of its own: the RGB calls go on ignoring BIC_OPT_SAMPLE_PREDICT, and a context that sets only
 * that one produces the streams it always did.
 *  - Samples to planes (bic_encode_rgb, bic_encode_rgb_packed, bic_bitplanes_rgb, bic_encode_rgb_frames,
 *    bic_encode_rgb_frames_packed): per pixel T_ct, giving R', G', B'; then on each of the three channels
 *    separately d_c(i,j) = (c'(i,j) - c'(i,j-1)) mod 256 with c'(i,-1) = 0 in every row of every frame (G is
 *    differenced too), folded in mode 2 with z = ((d << 1) ^ (d >> 7)) & 0xFF; then the Gray code per channel if
 *    BIC_OPT_GRAY_CODE is on, then the plane0 shift and the split. Planes, streams, bit counts, packed offsets and
 *    the row index equal those of the same call with options 8 and 10 both off on the image U(img) = T_sp(T_ct(img)).
 *  - Planes to samples (bic_planes_to_rgb, bic_decode_rgb, bic_decode_rgb_frames): each channel's z is assembled
 *    from the given planes as with the option off (bits no plane covers count as 0, then the un-Gray step and its
 *    mask), unfolded in mode 2 to d, then c'(j) = (c'(j-1) + d(j)) & 0xFF along the row from c'(-1) = 0 per channel,
 *    then the inverse colour transform on (R', G', B'), and all eight bits of the result are written (a pass of its
 *    own over the stored rows' first 3 * cols bytes; pitch padding and the gap between frames keep the caller's
 *    bytes). The result is the image exactly when plane0 = 0 and nplanes = 8; for any other range it is this formula.
 * Use mode 2 with BIC_CT_NONE or BIC_CT_SUBTRACT_GREEN. BIC_CT_SUBTRACT_GREEN_FOLDED folds before the difference:
 * allowed and exact, and a poor choice. The decoder's first-pixel bytes are bic_rgb_p00_predict's.
 * The gray, 16-bit, PBM and planes-only calls ignore option 10; the RGB calls ignore option 9. */
#define BIC_OPT_RGB_PREDICT 10
int bic_ctx_set_option(bic_ctx* ctx, int option, long value);

/* ---- a2: bitplane extraction (bitplane_tool.cpp:24-30) -----------------------------------
 * gray: rows x cols bytes with row pitch `pitch` (>= cols). Plane bi receives bit bi of every
 * pixel, LSB plane first; nplanes in 1..8 (bitplane_tool extracts #{bi : 2^bi < maxval}). */
int bic_bitplanes_u8(bic_ctx* ctx, const uint8_t* gray, size_t pitch, size_t rows, size_t cols,
                     int nplanes, uint64_t* planes, size_t wpr);
/* The planes plane0 .. plane0 + nplanes - 1 (plane0 + nplanes <= 8) only: output plane b is bit
 * plane0 + b of each pixel (bitplane_tool.cpp:24-30's plane index bi = plane0 + b). A rank of a
 * plane-sharded encode extracts its own share of one image this way. */
int bic_bitplanes_u8_range(bic_ctx* ctx, const uint8_t* gray, size_t pitch, size_t rows, size_t cols, int plane0,
                           int nplanes, uint64_t* planes, size_t wpr);
/* The same for samples of two bytes (pnm.cpp:71-74: a P5 sample with maxval >= 256 is (hi << 8) + lo,
 * high byte first; bitplane_tool.cpp:24-30 then extracts up to 16 planes): gray = rows of cols samples
 * with row pitch `pitch` in BYTES (>= 2 * cols), device memory of any byte alignment (pitch too).
 * big_endian = 1: the P5 order; 0: the host's uint16_t. Output plane b is bit plane0 + b of each
 * sample, plane0 + nplanes <= 16. bic_pgm_bitplanes with a row pitch and a choice of byte order. */
int bic_bitplanes_u16(bic_ctx* ctx, const void* gray, size_t pitch, size_t rows, size_t cols, int big_endian,
                      int plane0, int nplanes, uint64_t* planes, size_t wpr);

/* ---- a5/a6: med residual + weight (pred.cpp:3-15, binmat.cpp:57-67) -----------------------
 * resid (nullable): the med residual of each plane (R(0,0) = 0 and pad bits 0, which is what
 * the reference leaves/observes). weight_out (nullable, device, nplanes entries): popcount of the
 * residual (predict = 1) or of the plane itself (predict = 0). */
int bic_med_residual(bic_ctx* ctx, const uint64_t* planes, int nplanes, size_t rows, size_t cols,
                     size_t wpr, int predict, uint64_t* resid, uint64_t* weight_out);

/* ---- a7-a10: plane encoder ------------------------------------------------------------------
 * Runs per row in raster order: one sample per 1-pixel (zeros since the previous 1 or the row
 * start) and one EOL sample per row (the trailing zeros, also when 0); one coder per plane,
 * fresh state (Golomb.h:14-19 / eg.h:9). predict = 1 codes the med residual, 0 the plane.
 * out: nplanes slots of slot_words 64-bit words; plane_bits (device, nplanes): stream length
 * in bits. Domain: rows*(cols+1) < 2^31 (the reference's 32-bit coder state never wraps). */
int bic_encode_planes(bic_ctx* ctx, const uint64_t* planes, int nplanes, size_t rows, size_t cols,
                      size_t wpr, int predict, int coder, uint64_t* out, size_t slot_words,
                      uint64_t* plane_bits);
/* Both streams of the same planes in one pass (either output may be NULL, not both):
 * Golomb into out_golomb/slot_golomb/bits_golomb, EG into out_eg/slot_eg/bits_eg. Same layout
 * and semantics as two bic_encode_planes calls; rows of up to 16384 columns run as a single
 * fused kernel (plus a fixup of the words adjacent rows share). */
int bic_encode_planes2(bic_ctx* ctx, const uint64_t* planes, int nplanes, size_t rows, size_t cols,
                       size_t wpr, int predict, uint64_t* out_golomb, size_t slot_golomb,
                       uint64_t* bits_golomb, uint64_t* out_eg, size_t slot_eg, uint64_t* bits_eg);
/* a2 + a5-a10 in one call: bitplane_tool.cpp:24-30's planes of a gray image (as
 * bic_bitplanes_u8, into `planes`) and both streams of every plane (as bic_encode_planes2). Rows of
 * up to 16384 columns whose gray rows hold ceil(cols/64)*64 readable bytes (pitch >= that; any
 * alignment of gray and pitch, e.g. a P5 raster where it lies in its file's bytes) read the image
 * once: the bitplane kernel also produces the encoder's per-row counts. Otherwise the same result
 * through the two separate calls.
 * planes may be NULL (also in the _range / _packed forms below): the bitplanes are then formed in
 * registers only and not returned. With the EG stream requested into slots (out_eg, no packed EG
 * offsets) and predict = 1, the count pass writes the EG stream itself and the Golomb emission
 * reads each residual row back out of it (no further buffer). Otherwise the count pass stores each
 * plane's med residual in a buffer the context keeps (nplanes * rows * wpr words; it grows to the
 * largest call and lives until bic_ctx_destroy), from which the encoder writes the same streams
 * without recomputing med (no row above, no prediction in the emission).
 * Reads of a gray row whose address or pitch is not 16-byte aligned round out to the enclosing
 * aligned 16-byte chunks (never a chunk without one of the row's readable bytes, so never past the
 * last page of the buffer, but up to 15 bytes beyond the readable range). */
int bic_encode_gray(bic_ctx* ctx, const uint8_t* gray, size_t pitch, size_t rows, size_t cols, int nplanes,
                    uint64_t* planes, size_t wpr, int predict, uint64_t* out_golomb, size_t slot_golomb,
                    uint64_t* bits_golomb, uint64_t* out_eg, size_t slot_eg, uint64_t* bits_eg);
/* bic_encode_gray for the planes plane0 .. plane0 + nplanes - 1 of the image (plane0 + nplanes <= 8):
 * `planes`, the slots and bit counts hold those planes in order (plane0 first). The streams are
 * the ones bic_encode_gray produces for the same planes: each plane has its own coders. */
int bic_encode_gray_range(bic_ctx* ctx, const uint8_t* gray, size_t pitch, size_t rows, size_t cols, int plane0,
                          int nplanes, uint64_t* planes, size_t wpr, int predict, uint64_t* out_golomb,
                          size_t slot_golomb, uint64_t* bits_golomb, uint64_t* out_eg, size_t slot_eg,
                          uint64_t* bits_eg);
/* Packed output (what bic_pack_streams makes of the slots, without the copy): each coder's streams
 * are written word-aligned back to back from word 0 of out_golomb / out_eg (capacity nplanes *
 * slot words each, as for the slots), and off_golomb / off_eg (device, nplanes + 1 u64) receive
 * every plane's start word and the total. The multi-GPU gather sends these buffers as they are.
 * The staged encoder writes the packed positions directly; the other encoders go through slots
 * in a temporary and the pack kernel. off_* must be given for every coder that is written. */
int bic_encode_planes_packed(bic_ctx* ctx, const uint64_t* planes, int nplanes, size_t rows, size_t cols,
                             size_t wpr, int predict, uint64_t* out_golomb, size_t slot_golomb,
                             uint64_t* bits_golomb, uint64_t* off_golomb, uint64_t* out_eg, size_t slot_eg,
                             uint64_t* bits_eg, uint64_t* off_eg, uint64_t* row_index);
int bic_encode_gray_packed(bic_ctx* ctx, const uint8_t* gray, size_t pitch, size_t rows, size_t cols, int plane0,
                           int nplanes, uint64_t* planes, size_t wpr, int predict, uint64_t* out_golomb,
                           size_t slot_golomb, uint64_t* bits_golomb, uint64_t* off_golomb, uint64_t* out_eg,
                           size_t slot_eg, uint64_t* bits_eg, uint64_t* off_eg, uint64_t* row_index);
/* bic_encode_gray_range / bic_encode_gray_packed for samples of two bytes (pnm.cpp:71-74; the planes
 * bitplane_tool.cpp:24-30 extracts from a P5 file with maxval >= 256): gray = rows of cols samples, row
 * pitch `pitch` in BYTES (>= 2 * cols), any byte alignment of gray and pitch (odd included: a P5 raster
 * where it lies in its file's bytes). big_endian = 1: the P5 order, high byte first; 0: the host's
 * uint16_t. Planes plane0 .. plane0 + nplanes - 1 of the 16 (plane0 + nplanes <= 16; a range may cross
 * the byte boundary); outputs, nullable arguments, errors and domain as for the 8-bit calls, the
 * results bit-identical to bic_bitplanes_u16 (bic_pgm_bitplanes) followed by bic_encode_planes2 /
 * bic_encode_planes_packed. Bitplane extraction and med are linear over XOR, so planes 0-7 are the
 * 8-bit pipeline on the samples' low bytes and planes 8-15 the same on their high bytes: rows of up to
 * 16384 columns whose gray rows hold ceil(cols/64)*128 readable bytes read the image once (with planes
 * NULL, predict and the EG stream into slots the count pass writes the EG stream itself, as for
 * bic_encode_gray); otherwise the same result through the two separate calls. The device round trip of
 * a 16-bit image is gray -> bic_encode_gray16_packed -> bic_decode_gray (sample_bytes = 2, the same
 * big_endian). */
int bic_encode_gray16(bic_ctx* ctx, const void* gray, size_t pitch, size_t rows, size_t cols, int big_endian,
                      int plane0, int nplanes, uint64_t* planes, size_t wpr, int predict, uint64_t* out_golomb,
                      size_t slot_golomb, uint64_t* bits_golomb, uint64_t* out_eg, size_t slot_eg, uint64_t* bits_eg);
int bic_encode_gray16_packed(bic_ctx* ctx, const void* gray, size_t pitch, size_t rows, size_t cols, int big_endian,
                             int plane0, int nplanes, uint64_t* planes, size_t wpr, int predict, uint64_t* out_golomb,
                             size_t slot_golomb, uint64_t* bits_golomb, uint64_t* off_golomb, uint64_t* out_eg,
                             size_t slot_eg, uint64_t* bits_eg, uint64_t* off_eg, uint64_t* row_index);
/* Interleaved RGB (P6 with maxval < 256, pnm.cpp:194-239) -> streams in one call. rgb = rows of cols
 * pixels of three one-byte samples R, G, B; row pitch `pitch` in BYTES (>= 3 * cols); any byte alignment
 * of rgb and pitch (odd included: a P6 raster where it lies in its file's bytes, at
 * bic_pnm_parse_header's data_offset). plane0, nplanes: the range within each channel (plane0 + nplanes
 * <= 8). There are 3 * nplanes outputs: plane, stream, bit count, offset and row-index entry
 * c * nplanes + k belongs to plane plane0 + k of channel c (0 = R, 1 = G, 2 = B); slots, bits_*, off_*
 * (3 * nplanes + 1 entries), row_index and planes (3 * nplanes * rows * wpr words) are sized for them.
 * The results are bit for bit those of bic_encode_gray_range / bic_encode_gray_packed on channel c's
 * samples taken as a gray image (with BIC_OPT_GRAY_CODE: each channel's samples Gray-coded on their
 * own). Nullable planes, BIC_ENOSPC, rows = 0, the domain and the argument errors as for
 * bic_encode_gray_packed. Bitplane extraction and med are linear over XOR and no step couples the
 * channels, so plane 8 c + b of the image is the 8-bit pipeline on channel c's bytes: with the staged
 * encoder, an even wpr and rows of up to 16384 columns that hold ceil(cols/64)*192 readable bytes, one
 * count kernel reads the image once (with planes NULL, predict and the EG stream into slots the count pass writes the EG stream
 * itself, as for bic_encode_gray); otherwise the same result through bic_bitplanes_rgb followed by
 * bic_encode_planes2 / bic_encode_planes_packed. Samples of two bytes (P6 with maxval >= 256) are out of
 * scope: these calls have no way to express them. The device round trip is rgb -> bic_encode_rgb_packed
 * -> bic_decode_rgb. */
int bic_encode_rgb(bic_ctx* ctx, const uint8_t* rgb, size_t pitch, size_t rows, size_t cols, int plane0, int nplanes,
                   uint64_t* planes, size_t wpr, int predict, uint64_t* out_golomb, size_t slot_golomb,
                   uint64_t* bits_golomb, uint64_t* out_eg, size_t slot_eg, uint64_t* bits_eg);
int bic_encode_rgb_packed(bic_ctx* ctx, const uint8_t* rgb, size_t pitch, size_t rows, size_t cols, int plane0,
                          int nplanes, uint64_t* planes, size_t wpr, int predict, uint64_t* out_golomb,
                          size_t slot_golomb, uint64_t* bits_golomb, uint64_t* off_golomb, uint64_t* out_eg,
                          size_t slot_eg, uint64_t* bits_eg, uint64_t* off_eg, uint64_t* row_index);
/* The extraction alone and its inverse, in the same plane order (plane c * nplanes + k = plane plane0 + k
 * of channel c; planes = 3 * nplanes * rows * wpr words, pad bits and pad words 0). bic_planes_to_rgb
 * writes only the first 3 * cols bytes of each row; sample bits no plane covers are written 0. rgb and
 * pitch of any byte alignment; with BIC_OPT_GRAY_CODE the planes are those of each channel's Gray-coded
 * samples, as for the gray calls. */
int bic_bitplanes_rgb(bic_ctx* ctx, const uint8_t* rgb, size_t pitch, size_t rows, size_t cols, int plane0, int nplanes,
                      uint64_t* planes, size_t wpr);
int bic_planes_to_rgb(bic_ctx* ctx, const uint64_t* planes, int plane0, int nplanes, size_t rows, size_t cols,
                      size_t wpr, uint8_t* rgb, size_t pitch);
/* The p00 bytes bic_decode_rgb needs for an image whose first pixel is `pixel` (R, G, B), under the given
 * BIC_OPT_COLOR_TRANSFORM and BIC_OPT_GRAY_CODE values: p00[c * nplanes + k] = bit plane0 + k of channel c
 * of the transformed, then Gray-coded, pixel. Host code, no context. p00: host, 3 * nplanes bytes.
 * BIC_EINVAL: a mode outside 0..2, gray_code outside 0..1, a NULL pointer, plane0 < 0, nplanes < 1 or
 * plane0 + nplanes > 8. */
int bic_rgb_p00(int color_transform, int gray_code, const uint8_t pixel[3], int plane0, int nplanes, uint8_t* p00);
/* The gray twin: the p00 bytes bic_decode_gray / bic_decode_gray_frames need for a one-byte image (or frame) whose
 * first sample is `sample`, under the given BIC_OPT_SAMPLE_PREDICT and BIC_OPT_GRAY_CODE values. The first sample
 * has no left neighbour, so it is its own difference: p00[k] = bit plane0 + k of fold(sample) in mode 2, of the
 * sample in modes 0 and 1, after the Gray code. Host code, no context. p00: host, nplanes bytes. BIC_EINVAL: a
 * mode outside 0..2, gray_code outside 0..1, a NULL p00, plane0 < 0, nplanes < 1 or plane0 + nplanes > 8. */
int bic_gray_p00(int sample_predict, int gray_code, uint8_t sample, int plane0, int nplanes, uint8_t* p00);
/* bic_rgb_p00 under BIC_OPT_RGB_PREDICT as well: the first pixel has no left neighbour, so its bytes are
 * T_ct(pixel), folded on all three channels in mode 2 and unchanged in modes 0 and 1; then the Gray code, then the
 * bits plane0 + k. With rgb_predict = 0 the result is bic_rgb_p00's. Host code, no context. p00: host, 3 * nplanes
 * bytes. BIC_EINVAL: as for bic_rgb_p00, or rgb_predict outside 0..2. */
int bic_rgb_p00_predict(int color_transform, int rgb_predict, int gray_code, const uint8_t pixel[3], int plane0,
                        int nplanes, uint8_t* p00);
/* P4 rasters -> streams in one call: bic_pbm_unpack per frame followed by bic_encode_planes2 /
 * bic_encode_planes_packed, bit-identical streams, bit counts, offsets and row index. Frame f's raster
 * (pbm.cpp:29-77: rows x ceil(cols/8) bytes, MSB = leftmost pixel) lies at raster + f * frame_stride:
 * device memory of any byte alignment, e.g. a buffer of concatenated P4 files + data_offset;
 * frame_stride >= rows * ceil(cols/8) (ignored when nframes = 1). Frame f is plane f of every output:
 * slots, bits_*, off_*, row_index and planes + f * rows * wpr. The pad bits of a row's last byte are
 * ignored, whatever they hold. planes may be NULL; given, it receives the unpacked planes (pad bits 0).
 * Arguments, nullable outputs, BIC_ENOSPC, the domain and rows = 0 as for bic_encode_gray_packed.
 * With the staged encoder (>= 32768 rows in all frames, or BIC_OPT_STAGED), cols <= 16384, an even wpr
 * and 16-byte aligned planes, one count kernel reads every raster byte once and writes the encoder's
 * per-row records together with the planes or, with planes NULL, their med residual into the context's
 * residual buffer (nframes * rows * wpr words; it grows to the largest call and lives until
 * bic_ctx_destroy), which the emission codes with prediction off. Otherwise the same result through
 * the separate calls (with planes NULL, unpacked into that buffer).
 * Reads of a raster round out to the enclosing aligned 8-byte chunks (never a chunk without one of the
 * frame's raster bytes, so never past the last page of the buffer, but up to 7 bytes before a frame's
 * first byte and beyond its last). */
int bic_encode_pbm(bic_ctx* ctx, const uint8_t* raster, size_t frame_stride, int nframes, size_t rows, size_t cols,
                   uint64_t* planes, size_t wpr, int predict, uint64_t* out_golomb, size_t slot_golomb,
                   uint64_t* bits_golomb, uint64_t* out_eg, size_t slot_eg, uint64_t* bits_eg);
int bic_encode_pbm_packed(bic_ctx* ctx, const uint8_t* raster, size_t frame_stride, int nframes, size_t rows,
                          size_t cols, uint64_t* planes, size_t wpr, int predict, uint64_t* out_golomb,
                          size_t slot_golomb, uint64_t* bits_golomb, uint64_t* off_golomb, uint64_t* out_eg,
                          size_t slot_eg, uint64_t* bits_eg, uint64_t* off_eg, uint64_t* row_index);
/* A batch of gray frames -> streams in one call: nframes images of one geometry (tiles of a scan, video
 * frames, a queue of small images), each coded as bic_encode_gray_range / bic_encode_gray_packed (sample_bytes
 * = 1) or bic_encode_gray16 / bic_encode_gray16_packed (sample_bytes = 2, big_endian as there; ignored for
 * one-byte samples) codes it alone -- fresh coders per plane, no row above a frame's row 0, R(0,0) = 0 in
 * every frame -- bit for bit. Frame f is rows x cols samples at (const uint8_t*)gray + f * frame_stride, row
 * pitch `pitch` bytes (>= cols * sample_bytes); gray, pitch and frame_stride of any byte alignment (a buffer
 * of concatenated P5 files + data_offset works as it lies); frame_stride >= rows * pitch (ignored when
 * nframes = 1). plane0, nplanes: the plane range within a sample (plane0 + nplanes <= 8 * sample_bytes).
 * There are nframes * nplanes outputs: plane, slot, bit count, offset and row-index entry f * nplanes + k
 * belongs to plane plane0 + k of frame f; off_* have nframes * nplanes + 1 entries and run through all
 * streams as bic_pack_streams would lay them out; planes, when given, holds nframes * nplanes * rows * wpr
 * words. BIC_OPT_GRAY_CODE as in the single-image calls. Nullable planes and coders, BIC_ENOSPC, the domain
 * rows * (cols + 1) < 2^31 per plane, the 15-byte read round-out and rows = 0 as for bic_encode_gray_packed.
 * BIC_EINVAL also for nframes < 1, nframes * nplanes > 65535 and a frame_stride below rows * pitch.
 * One-byte samples, the staged encoder (>= 32768 rows in all planes, or BIC_OPT_STAGED), an even wpr, cols
 * <= 16384 and rows that hold ceil(cols/64)*64 readable bytes: one count kernel reads every frame once
 * (with planes NULL, predict and the EG stream into slots it writes the EG streams itself); otherwise, and
 * for two-byte samples, the same result through bic_bitplanes_u8_range / bic_bitplanes_u16 per frame and
 * one bic_encode_planes2 / bic_encode_planes_packed. The device round trip is gray frames ->
 * bic_encode_gray_frames_packed -> bic_decode_gray_frames. */
int bic_encode_gray_frames(bic_ctx* ctx, const void* gray, size_t frame_stride, int nframes, size_t pitch, size_t rows,
                           size_t cols, int sample_bytes, int big_endian, int plane0, int nplanes, uint64_t* planes,
                           size_t wpr, int predict, uint64_t* out_golomb, size_t slot_golomb, uint64_t* bits_golomb,
                           uint64_t* out_eg, size_t slot_eg, uint64_t* bits_eg);
int bic_encode_gray_frames_packed(bic_ctx* ctx, const void* gray, size_t frame_stride, int nframes, size_t pitch,
                                  size_t rows, size_t cols, int sample_bytes, int big_endian, int plane0, int nplanes,
                                  uint64_t* planes, size_t wpr, int predict, uint64_t* out_golomb, size_t slot_golomb,
                                  uint64_t* bits_golomb, uint64_t* off_golomb, uint64_t* out_eg, size_t slot_eg,
                                  uint64_t* bits_eg, uint64_t* off_eg, uint64_t* row_index);
/* A batch of RGB frames -> streams in one call: nframes interleaved RGB images of one geometry (video frames,
 * tiles of a colour scan), each coded as bic_encode_rgb / bic_encode_rgb_packed codes it alone -- fresh coders
 * per plane, no row above a frame's row 0, R(0,0) = 0 in every frame -- bit for bit. Frame f is rows rows of cols
 * pixels of three one-byte samples R, G, B at rgb + f * frame_stride, row pitch `pitch` bytes (>= 3 * cols);
 * rgb, pitch and frame_stride of any byte alignment (a buffer of concatenated P6 files + data_offset works as it
 * lies); frame_stride >= rows * pitch (ignored when nframes = 1). plane0, nplanes: the range within each channel
 * (plane0 + nplanes <= 8). There are nframes * 3 * nplanes outputs: plane, slot, bit count, offset and row-index
 * entry (f * 3 + c) * nplanes + k belongs to plane plane0 + k of channel c of frame f, so frame f's block of
 * 3 * nplanes entries is what bic_encode_rgb* returns for that frame; off_* have nframes * 3 * nplanes + 1 entries
 * and run through all streams as bic_pack_streams would lay them out; planes, when given, holds nframes * 3 *
 * nplanes * rows * wpr words. BIC_OPT_GRAY_CODE and BIC_OPT_COLOR_TRANSFORM as in the single-image RGB calls
 * (a pixel's green is its own frame's); BIC_OPT_SAMPLE_PREDICT is ignored, as in every RGB call. Nullable planes
 * and coders, BIC_ENOSPC, the domain rows * (cols + 1) < 2^31 per plane, the 15-byte read round-out, rows = 0 and
 * the argument errors as for bic_encode_gray_frames_packed. BIC_EINVAL also for nframes < 1, nframes * 3 *
 * nplanes > 65535 and a frame_stride below rows * pitch. nframes = 1 is the single-image call itself.
 * The staged encoder (>= 32768 rows in all planes, or BIC_OPT_STAGED), an even wpr, cols <= 16384 and rows that
 * hold ceil(cols/64)*192 readable bytes: one count kernel reads every frame once (with planes NULL, predict and
 * the EG stream into slots it writes the EG streams itself); otherwise the same result through bic_bitplanes_rgb
 * per frame and one bic_encode_planes2 / bic_encode_planes_packed. The device round trip is RGB frames ->
 * bic_encode_rgb_frames_packed -> bic_decode_rgb_frames. */
int bic_encode_rgb_frames(bic_ctx* ctx, const uint8_t* rgb, size_t frame_stride, int nframes, size_t pitch,
                          size_t rows, size_t cols, int plane0, int nplanes, uint64_t* planes, size_t wpr,
                          int predict, uint64_t* out_golomb, size_t slot_golomb, uint64_t* bits_golomb,
                          uint64_t* out_eg, size_t slot_eg, uint64_t* bits_eg);
int bic_encode_rgb_frames_packed(bic_ctx* ctx, const uint8_t* rgb, size_t frame_stride, int nframes, size_t pitch,
                                 size_t rows, size_t cols, int plane0, int nplanes, uint64_t* planes, size_t wpr,
                                 int predict, uint64_t* out_golomb, size_t slot_golomb, uint64_t* bits_golomb,
                                 uint64_t* off_golomb, uint64_t* out_eg, size_t slot_eg, uint64_t* bits_eg,
                                 uint64_t* off_eg, uint64_t* row_index);

/* ---- f1: decoders on the device (GolombDecoder.cpp:15-23 read order, eg.cpp:20-37 as written) --
 * row_index (device, nplanes * rows * 2 u64; nullable in the encoders above): per row of each plane,
 * [2 (p rows + r)] = the bit offset of the row's first Golomb codeword in plane p's stream and
 * [2 (p rows + r) + 1] = the residual 1s of plane p before row r (the coder state at the row start:
 * N = ones + r, A = r cols - ones, Golomb.h:21-24). The staged encoder writes it from its scans;
 * bic_row_index computes it from planes (the encoder's prefix kernels alone; cols <= 16384, planes
 * 16-byte aligned). */
int bic_row_index(bic_ctx* ctx, const uint64_t* planes, int nplanes, size_t rows, size_t cols, size_t wpr,
                  int predict, uint64_t* index);
/* The row index of the adaptive EG coder (BIC_CODER_EG_ADAPTIVE; eg.cpp:20-37 with incBlockSize):
 * [2 (p rows + r)] = the bit offset of row r's first codeword in plane p's stream, [2 (p rows + r) + 1]
 * = the coder state there (eg.h's lutIndex, 0..31; 32 = a fresh coder, row 0: index 0, g = 1). From
 * the planes (the encoder's map / resolve / length passes, no stream written). */
int bic_egad_row_index(bic_ctx* ctx, const uint64_t* planes, int nplanes, size_t rows, size_t cols, size_t wpr,
                       int predict, uint64_t* index);
/* streams -> planes (device): slot_words > 0: plane p's stream at streams + p * slot_words;
 * slot_words == 0: packed, at streams + word_off[p], word_off[0..nplanes] as the packed encoders write
 * it (plane p owns words word_off[p] .. word_off[p + 1]). plane_bits: each stream's length; a length
 * past the plane's slot or packed words is malformed (nothing beyond them is read). Golomb needs
 * row_index (rows decode independently); EG finds the row of the plane's first 1 itself;
 * BIC_CODER_EG_ADAPTIVE needs bic_egad_row_index's index (eg.cpp:41-55's read order). predict:
 * the streams code the med residual; P(0, 0), which med discards, comes from p00 (device, one byte
 * per plane; nullable: 0). cols <= 16384. A malformed stream (bad codeword, wrong length, missing
 * end-of-row bit) is reported by bic_sync as BIC_EDATA; the planes are then undefined. */
int bic_decode_planes(bic_ctx* ctx, int coder, const uint64_t* streams, size_t slot_words, const uint64_t* word_off,
                      const uint64_t* plane_bits, const uint64_t* row_index, int nplanes, size_t rows, size_t cols,
                      size_t wpr, int predict, const uint8_t* p00, uint64_t* planes);
/* streams -> gray samples in one call: bic_decode_planes followed by bic_planes_to_gray, without the
 * planes. coder, streams, slot_words, word_off, plane_bits, row_index, predict, p00, the limit
 * cols <= 16384 and BIC_EDATA from bic_sync for a malformed stream (the samples are then undefined) as
 * for bic_decode_planes; the samples as bic_planes_to_gray writes them: stream b sets bit plane0 + b
 * of each sample, bits no plane covers are 0, sample_bytes 1 (plane0 + nplanes <= 8) or 2 (<= 16),
 * gray = rows of `pitch` bytes (device, any byte alignment of pointer and pitch), of which only the
 * first cols * sample_bytes are written. big_endian (sample_bytes 2 only): 1 = the P5 order
 * bic_planes_to_gray writes, 0 = the host's uint16_t (what bic_encode_gray16 reads with big_endian = 0).
 * The row decoders write D (the planes XORed with the row above; the planes themselves without
 * prediction) into a buffer the context keeps -- nplanes * rows * ceil(cols/64) words in the scratch
 * arena, which grows to the largest call and lives until bic_ctx_destroy -- and unmed's last kernel
 * forms the samples as it sums D down the columns: the planes are never written. rows = 0: BIC_OK,
 * nothing written. */
int bic_decode_gray(bic_ctx* ctx, int coder, const uint64_t* streams, size_t slot_words,
                    const uint64_t* word_off, const uint64_t* plane_bits, const uint64_t* row_index,
                    int plane0, int nplanes, size_t rows, size_t cols, int predict, const uint8_t* p00,
                    int sample_bytes, int big_endian, void* gray, size_t pitch);
/* bic_decode_gray for every frame of a batch in one call: the nframes * nplanes streams in
 * bic_encode_gray_frames' order (stream f * nplanes + k sets bit plane0 + k of frame f's samples; p00 one
 * byte per stream), frame f written at (uint8_t*)gray + f * frame_stride (>= rows * pitch, ignored when
 * nframes = 1; any byte alignment). Only the first cols * sample_bytes bytes of each row of each frame are
 * written: pitch padding and the gap between frames keep the caller's bytes. Coders, row_index, BIC_EDATA,
 * cols <= 16384 and rows = 0 as for bic_decode_gray; BIC_EINVAL also for nframes < 1 and nframes * nplanes >
 * 65535. */
int bic_decode_gray_frames(bic_ctx* ctx, int coder, const uint64_t* streams, size_t slot_words,
                           const uint64_t* word_off, const uint64_t* plane_bits, const uint64_t* row_index,
                           int nframes, int plane0, int nplanes, size_t rows, size_t cols, int predict,
                           const uint8_t* p00, int sample_bytes, int big_endian, void* gray, size_t pitch,
                           size_t frame_stride);
/* streams -> interleaved RGB samples in one call: bic_decode_planes followed by bic_planes_to_rgb,
 * without the planes, as bic_decode_gray does for gray. The 3 * nplanes streams in bic_encode_rgb's
 * order (stream c * nplanes + k sets bit plane0 + k of channel c); coder, streams, slot_words, word_off,
 * plane_bits, row_index, predict, the limit cols <= 16384 and BIC_EDATA from bic_sync as for
 * bic_decode_gray; p00 (device, one byte per stream; nullable: 0). rgb = rows of `pitch` bytes (>= 3 *
 * cols; any byte alignment of pointer and pitch), of which only the first 3 * cols are written; bits
 * no plane covers are written 0. rows = 0: BIC_OK, nothing written. */
int bic_decode_rgb(bic_ctx* ctx, int coder, const uint64_t* streams, size_t slot_words, const uint64_t* word_off,
                   const uint64_t* plane_bits, const uint64_t* row_index, int plane0, int nplanes, size_t rows,
                   size_t cols, int predict, const uint8_t* p00, uint8_t* rgb, size_t pitch);
/* bic_decode_rgb for every frame of a batch in one call: the nframes * 3 * nplanes streams in
 * bic_encode_rgb_frames' order (stream (f * 3 + c) * nplanes + k sets bit plane0 + k of channel c of frame f;
 * p00 one byte per stream, frame f's 3 * nplanes bytes being bic_rgb_p00 of its first pixel), frame f written at
 * rgb + f * frame_stride (>= rows * pitch, ignored when nframes = 1; any byte alignment). Only the first 3 * cols
 * bytes of each row of each frame are written: pitch padding and the gap between frames keep the caller's bytes.
 * Coders (BIC_CODER_EG_ADAPTIVE with bic_egad_row_index's index included), row_index, BIC_EDATA from bic_sync,
 * cols <= 16384 and rows = 0 as for bic_decode_rgb; BIC_EINVAL also for nframes < 1 and nframes * 3 * nplanes >
 * 65535. */
int bic_decode_rgb_frames(bic_ctx* ctx, int coder, const uint64_t* streams, size_t slot_words,
                          const uint64_t* word_off, const uint64_t* plane_bits, const uint64_t* row_index,
                          int nframes, int plane0, int nplanes, size_t rows, size_t cols, int predict,
                          const uint8_t* p00, uint8_t* rgb, size_t pitch, size_t frame_stride);
/* streams -> P4 rasters in one call: bic_decode_planes followed by bic_pbm_pack per frame, without the
 * planes. coder, streams, slot_words, word_off, plane_bits, row_index, predict, the limit cols <= 16384
 * and BIC_EDATA from bic_sync (the rasters are then undefined) as for bic_decode_gray; stream f is frame
 * f, written at raster + f * frame_stride (device, any byte alignment; frame_stride >= rows *
 * ceil(cols/8), ignored when nframes = 1). Only the rows * ceil(cols/8) bytes of each frame are written;
 * the pad bits of a row's last byte are written 0. p00 (device, one byte per frame; nullable: 0):
 * p00[f] = raster_f[0] >> 7, the frame's first pixel. The row decoders write D into the scratch arena
 * as for bic_decode_gray, and the last kernel forms each row's raster bytes as it sums D down the
 * columns. rows = 0: BIC_OK, nothing written. */
int bic_decode_pbm(bic_ctx* ctx, int coder, const uint64_t* streams, size_t slot_words, const uint64_t* word_off,
                   const uint64_t* plane_bits, const uint64_t* row_index, int nframes, size_t rows, size_t cols,
                   int predict, const uint8_t* p00, uint8_t* raster, size_t frame_stride);
/* A slot size (64-bit words) that every plane of this geometry fits for EG (exact) and for
 * Golomb on any input this build has seen (2*rows*(cols+1) bits + 64 words); a larger input
 * still reports BIC_ENOSPC rather than writing out of bounds. */
size_t bic_encode_slot_words(size_t rows, size_t cols, int coder);

/* ---- GolombCoder::codeSample over an arbitrary sample array (GolombCoder.cpp:29-34) --------
 * Coder state on entry: n0 samples already coded with accumulated error a0 (n0 = a0 = 0 is a
 * fresh GolombCoder). The stream is written starting at bit `bit0` of out (0 <= bit0 < 64;
 * lets a shard start at its global bit alignment); out[0 .. cap_words) must be writable.
 * bits_out (device, 2 x u64): [0] = codeword bits (= GolombCoder::bitcount), [1] = sum of samples.
 * out = NULL with cap_words = 0 computes bits_out only (no stream): a shard learns its length
 * before its bit offset is known, then encodes once at that offset. */
int bic_golomb_encode_samples(bic_ctx* ctx, const uint32_t* samples, size_t n, uint64_t n0,
                              uint64_t a0, unsigned bit0, uint64_t* out, size_t cap_words,
                              uint64_t* bits_out);

/* ---- a11-a13: W x W tile path (compress7_test.cpp:118-275 with R = 0) ---------------------
 * Per tile in raster order: w_nonpred = weight(P), w_pred = weight(med(P)) (med inside the tile,
 * R(0,0) = 0); mode 'O' iff lentab[w_nonpred] > lentab[w_pred] else 'o'; the chosen weight is
 * Golomb-coded (golomb_nomatch.codeSample, compress7_test.cpp:270) and lentab[chosen] summed (L).
 * lentab: HOST array of W*W+1 entries, lentab[w] = (idx_t)(2 + enumL(W*W, w)) (see coding.h).
 * Requires 1 <= W <= 64, rows % W == 0, cols % W == 0 (no edge wrap).
 * Outputs (device, each nullable except stream): weights (chosen), w_nonpred, w_pred (u32 per
 * tile), modes (u8 per tile), resid (the image after the residual write-back of :266/:272),
 * stream (cap_words words) and stats (device u64[3]: Golomb bits, sum of chosen weights, L). */
int bic_patch_encode(bic_ctx* ctx, const uint64_t* plane, size_t rows, size_t cols, size_t wpr,
                     unsigned W, const uint64_t* lentab, uint32_t* weights, uint32_t* w_nonpred,
                     uint32_t* w_pred, uint8_t* modes, uint64_t* resid, uint64_t* stream,
                     size_t cap_words, uint64_t* stats);

/* ---- patch match search (compress_test.cpp:73-111) ----------------------------
 * For every W x W tile in raster order over ceil(rows/W) x ceil(cols/W) (1 <= W <= 64): the
 * position (besti, bestj) and distance bestd of the least Hamming distance between the tile and a
 * W x W window over the causal search region -- rows 0 .. i0-W at every column, then rows
 * i0-W+1 .. i0 at columns 0 .. j0-W -- first in the reference's scan order; (0, 0, W*W) when no
 * window beats W*W. Windows use get_submatrix's flat indexing (binmat.cpp:267-298: past the right
 * edge they continue in the next row). Outputs: device u32 arrays, one entry per tile. */
int bic_patch_search(bic_ctx* ctx, const uint64_t* plane, size_t rows, size_t cols, size_t wpr, unsigned W,
                     uint32_t* besti, uint32_t* bestj, uint32_t* bestd);

/* ---- compress7_test.cpp:117-275 with a search window --------------------------
 * The driver's whole tile loop with its arguments W (argv[2]), T (argv[3]) and R (argv[4]): per W x W
 * tile in raster order, the least-distance window of the causal search region of the image as the
 * residual write-back of every earlier tile left it (rows i0 .. i0-W at columns j0-W .. j0-R, then
 * rows i0-W .. i0-R at columns j0+R .. j0-R, scanned downwards, stopping at the first distance
 * <= T), the four candidate lengths (2 + enumL, plus ceil(log2(search_win_size)) for a match), the
 * mode 'X' / 'x' (match, med or not) or 'O' / 'o' (no match), the chosen weight coded by
 * golomb_match or golomb_nomatch, and the residual written back.
 *   plane: device, rows x wpr, not modified; resid: device, rows x wpr, receives the image after
 *   the loop (may equal plane). enuml: HOST array of W*W+1 doubles, enuml[w] = enumL(W*W, w)
 *   (bic_enum_codelength, or the caller's GSL values). Requires 1 <= W <= 64, rows % W == 0,
 *   cols % W == 0, R <= 32767. Per tile (device, each nullable): besti, bestj, bestd (W*W+1 when
 *   the region holds no window), weights (the coded weight), modes. stream_match / stream_nomatch:
 *   device, cap_words each, the two coders' codewords. stats: device u64[4]: matches, bits of
 *   golomb_match, bits of golomb_nomatch, sum of the chosen lengths (the driver's L before it adds
 *   the two bitcounts). A search_win_size <= 0 (whose log2 the driver converts with undefined
 *   behaviour; 2^63 on x86-64) makes a match impossible for that tile. */
int bic_match_encode(bic_ctx* ctx, const uint64_t* plane, size_t rows, size_t cols, size_t wpr, unsigned W,
                     unsigned T, unsigned R, const double* enuml, uint32_t* besti, uint32_t* bestj,
                     uint32_t* bestd, uint32_t* weights, uint8_t* modes, uint64_t* resid,
                     uint64_t* stream_match, uint64_t* stream_nomatch, size_t cap_words, uint64_t* stats);
/* compress8_test.cpp:126-272's loop (patch inversion), otherwise as bic_match_encode:
 *   - a window's distance d becomes M - d when (M - d) < d, the window then inverted (:156-161);
 *     bestd is that min(d, M - d);
 *   - before any search a tile of weight <= T or >= M - T is a perfect match (:137: no window);
 *   - bestinv starts as (P.weight() - M) < P.weight() (:136, idx_t: the tile is all 1s) and takes
 *     the inversion of each better window (:163); an inverted tile is flipped (P.flip(), :207-210)
 *     before P3 and all four weights are formed;
 *   - the match lengths are 3 + idx_len + enumL (one bit more, :250-251).
 * inverted (device, per tile, nullable): bestinv. The driver leaves a non-inverted window's `inv`
 * uninitialised (:157); here it is false. T is the caller's (the driver's default is its goodT, :73). */
int bic_match_encode_inv(bic_ctx* ctx, const uint64_t* plane, size_t rows, size_t cols, size_t wpr, unsigned W,
                         unsigned T, unsigned R, const double* enuml, uint32_t* besti, uint32_t* bestj,
                         uint32_t* bestd, uint32_t* weights, uint8_t* modes, uint8_t* inverted, uint64_t* resid,
                         uint64_t* stream_match, uint64_t* stream_nomatch, size_t cap_words, uint64_t* stats);
/* The tile loops of the other windowed-search drivers, otherwise as bic_match_encode (same
 * arguments and outputs; the driver's W, T, R; variant 7 = bic_match_encode, 8 = bic_match_encode_inv
 * without the per-tile inversion flags):
 *   4: compress4_test.cpp:89-170 -- no med: the first loop starts at column j0 - W (none at j0 = 0),
 *      idx_len = ceil(log2(li)) of the tile's raster index li (li = 0: 2^63, never a match),
 *      nomatch_len = 1 + enumL(M, P.weight()), match_len = 1 + idx_len + enumL(M, bestd) when bestd
 *      <= M, else 100000; a match codes bestd with golomb_match and writes P ^ window back, no match
 *      codes P.weight() with golomb_nomatch and leaves the tile; modes 'x' / 'o';
 *   5: compress5_test.cpp:89-170 -- 4 with a window kept when (d - worstd) > (bestd - worstd) in
 *      idx_t arithmetic, worstd = W*W/2 (:94, :109, :126);
 *   6: compress6_test.cpp:111-208 -- 4 with P3 = P when no window and match_len = 1 + idx_len +
 *      enumL(M, P3.weight()) (no 100000 guard); its D / iD matrices (:64-76) are built but unused
 *      (#if 0, :172-182).
 * Schedule: per-tile workgroups (bic_set_match_parts 1..256, or automatic). */
int bic_match_encode_var(bic_ctx* ctx, int variant, const uint64_t* plane, size_t rows, size_t cols, size_t wpr,
                         unsigned W, unsigned T, unsigned R, const double* enuml, uint32_t* besti, uint32_t* bestj,
                         uint32_t* bestd, uint32_t* weights, uint8_t* modes, uint64_t* resid, uint64_t* stream_match,
                         uint64_t* stream_nomatch, size_t cap_words, uint64_t* stats);
/* Schedule of bic_match_encode (every schedule gives the same result): 0 (default) = automatic;
 * N in 1..256 = N workgroups per tile, tiles in raster order with flags between them;
 * 0x10000 | H = one workgroup per tile row walking its tiles, plus H helper workgroups that search
 * ahead of it (W of 8, 16 or 32 and a band of (R + 2W) x (cols/32 + 2) 32-bit words <= 30 Ki; other
 * W: the row workgroup alone); other values: per-tile workgroups, count from W and R. */
int bic_set_match_parts(bic_ctx* ctx, unsigned parts);

/* ---- the growing-dictionary tile coder: compress2_test.cpp:79-129, compress3_test.cpp:87-149 ------
 * The drivers' whole tile loop with W (argv[2]) and, variant 3, T (argv[3]). Tiles t = 0 .. ny*nx-1 in
 * raster order over ny = ceil(rows/W), nx = ceil(cols/W), read with get_submatrix's flat indexing as for
 * bic_patch_search; the image is never written. The dictionary is an ordered list of tiles. Per tile:
 *   - search: bestk = 0, bestd = W*W; the atoms in dictionary order with strict <, stopping at the first
 *     distance 0: the first atom at least distance, (0, W*W) when none beats W*W;
 *   - nomatch_len = (idx_t)(1 + enuml[weight(P)] + h), match_len = (idx_t)(1 + ceil(log2(|D|)) +
 *     enuml[bestd] + h), the doubles added left to right; h = 0.5 log2(W*W) (variant 2) or 0 (variant 3);
 *   - an empty dictionary: the tile is pushed, L += nomatch_len, mode 'o', no sample is coded;
 *   - variant 2: a match ('x', L += match_len) iff nomatch_len > match_len, else pushed ('o',
 *     L += nomatch_len); no Golomb coder;
 *   - variant 3: a match iff nomatch_len > match_len ('x', golomb_match codes bestd), else 'o'
 *     (golomb_nomatch codes weight(P)); then, whatever the mode, pushed iff bestd > T.
 * atom_step: the drivers push the tile's INDEX pair (i, j) and read atom windows at PIXEL (i, j)
 * (compress2_test.cpp:87-88,105,124; compress3_test.cpp:95-96,118,145). Atom k's window is at pixel
 * (i * atom_step, j * atom_step): 1 = the drivers, W = the tile itself; anything else is BIC_EINVAL.
 *   plane: device, rows x wpr. enuml: HOST array of W*W+1 doubles as for bic_match_encode. Per tile
 *   (device, each nullable): bestk, bestd, dsize (|D| as the tile saw it), weights (the coded value:
 *   bestd or weight(P)), modes, joined (1 iff pushed). dict_tiles (device, ny*nx u32, nullable): the
 *   tile index of every atom, in dictionary order. stream_match / stream_nomatch (device, cap_words each):
 *   variant 3's codewords; both may be NULL with cap_words = 0 (the lengths only); variant 2 ignores
 *   them. stats: device u64[5]: matches, bits of golomb_match, bits of golomb_nomatch, L, the final |D|.
 * BIC_EINVAL (arguments; no device work) for variant not 2 or 3, W outside 1..64, atom_step, geometry.
 * A stream too small is BIC_ENOSPC from bic_sync, as for bic_match_encode. Nothing is read back and
 * nothing waits inside the call. */
int bic_dict_encode(bic_ctx* ctx, int variant, const uint64_t* plane, size_t rows, size_t cols, size_t wpr,
                    unsigned W, unsigned T, unsigned atom_step, const double* enuml, uint32_t* bestk,
                    uint32_t* bestd, uint32_t* dsize, uint32_t* weights, uint8_t* modes, uint8_t* joined,
                    uint32_t* dict_tiles, uint64_t* stream_match, uint64_t* stream_nomatch, size_t cap_words,
                    uint64_t* stats);
/* Tiles bic_dict_encode resolves per block (every value gives the same result): 0 (default) = automatic,
 * else that many, at most 1024 and at most 4096 / W' with W' = W rounded up to a multiple of 8 (what the
 * resolving workgroup keeps in LDS). */
int bic_set_dict_block(bic_ctx* ctx, unsigned tiles);

/* log2 C(n, r) (enumerative_codelength, coding.cpp:19-22) computed without GSL, and the tile
 * length table lentab[w] = (uint64)(2 + log2 C(W*W, w)) for w = 0..W*W (host memory, W*W+1
 * entries) that bic_patch_encode takes. Host-side helpers; no device needed. */
double bic_enum_codelength(unsigned n, unsigned r);
int bic_tile_lentab(unsigned W, uint64_t* lentab);

/* ---- stream packing ---------------------------------------------------------------------------
 * Concatenates the nplanes slot streams (plane_bits from bic_encode_planes) word-aligned into
 * dst; word_off (device, nplanes+1): start word of each plane in dst, word_off[nplanes] = total. */
int bic_pack_streams(bic_ctx* ctx, const uint64_t* slots, int nplanes, size_t slot_words,
                     const uint64_t* plane_bits, uint64_t* dst, uint64_t* word_off);

/* ---- PBM (P4) rasters on the device (pbm.cpp:29-77) ------------------------------------------
 * A P4 raster is rows x ceil(cols/8) bytes, MSB = leftmost pixel, rows byte-aligned (device
 * memory, no header, any alignment: e.g. a file's bytes + data_offset). unpack: raster -> planes
 * (rows x wpr words; pad bits 0); pack: planes -> raster (pad bits of the last byte of a row 0), as
 * read_pbm_data / write_pbm do bit by bit. */
int bic_pbm_unpack(bic_ctx* ctx, const uint8_t* raster, size_t rows, size_t cols, uint64_t* plane, size_t wpr);
int bic_pbm_pack(bic_ctx* ctx, const uint64_t* plane, size_t rows, size_t cols, size_t wpr, uint8_t* raster);

/* ---- a1 / f3: PNM headers on the host, PGM samples on the device (pnm.cpp:5-89) -------------
 * bic_pnm_parse_header: the header of a P4 (pbm.cpp:4-27, " %d " swallowing whitespace after the
 * height, raster bytes included) or P2 / P5 / P6 file (pnm.cpp:20-42: '#' comment lines between
 * fields, one byte after maxval) from its first n bytes (host memory); data_offset = where the
 * raster starts. P4: maxval = 1. */
typedef struct {
  int type;            /* 4 = P4 (PBM); 2, 5 = PGM; 6 = PPM */
  size_t rows, cols;
  int maxval;
  size_t data_offset;
} bic_pnm_info;
int bic_pnm_parse_header(const uint8_t* bytes, size_t n, bic_pnm_info* info);
/* P5 samples on the device -> planes plane0 .. plane0 + nplanes - 1 (bitplane_tool.cpp:24-30):
 * raster = the first sample (device, any alignment, e.g. a file's bytes + data_offset), 1 byte per
 * sample when maxval < 256 else 2 bytes big-endian (pnm.cpp:71-74), rows of cols samples. */
int bic_pgm_bitplanes(bic_ctx* ctx, const uint8_t* raster, size_t rows, size_t cols, int maxval, int plane0,
                      int nplanes, uint64_t* planes, size_t wpr);
/* planes -> gray samples on the device (replaces plane2pgm_tool.cpp:33-52, the reassembly loop
 * `gray_img[li] |= mask` over planes 0, 1, ... with mask = 1 << plane): plane b sets bit plane0 + b
 * of each sample, bits no plane covers are 0. sample_bytes 1: one byte per sample (plane0 + nplanes
 * <= 8); 2: two bytes big-endian, the P5 raster write_p5_data writes for maxval >= 256
 * (pnm.cpp:111-124; plane0 + nplanes <= 16). gray: device, rows of `pitch` bytes (any alignment);
 * only the rows' first cols * sample_bytes bytes are written. From streams, bic_decode_gray writes
 * the same samples without the planes: the device round trip is gray -> bic_encode_gray_packed ->
 * bic_decode_gray. */
int bic_planes_to_gray(bic_ctx* ctx, const uint64_t* planes, int plane0, int nplanes, size_t rows, size_t cols,
                       size_t wpr, int sample_bytes, void* gray, size_t pitch);

/* ---- f4: binary_matrix algebra over GF(2) (binmat.cpp:199-214, 516-616) ---------------------
 * Matrices are rows x cols bits in the plane layout (wpr >= ceil(cols/64) words per row, device
 * memory). bic_gf2_transpose replaces transpose_to / get_transposed: dst (cols x rows, dst_wpr >=
 * ceil(rows/64)) gets dst(j,i) = src(i,j); the ceil(rows/64) words of every dst row are written
 * (bits past rows 0). bic_gf2_mul replaces mul(A, At, B, Bt, C) (binmat.cpp:606-616) with op =
 * BIC_GF2_AB (mul_AB :516-542), BIC_GF2_ATB (mul_AtB :545-572), BIC_GF2_ABT (mul_ABt :575-594) or
 * BIC_GF2_ATBT (mul_AtBt :596-604, not implemented there: C unchanged); the reference's asserts on
 * the shapes become BIC_EINVAL. C's first ceil(c_cols/64) words per row are written; mul_ABt as
 * written sets only bits j < b_cols of a row (0 for j >= b_rows) and keeps the others. Products
 * over the whole words of their operands, as the reference's block loops (padding bits included
 * where its loops include them). Scratch for the transposed operand is stream-ordered. */
#define BIC_GF2_AB 0
#define BIC_GF2_ATB 1
#define BIC_GF2_ABT 2
#define BIC_GF2_ATBT 3
int bic_gf2_transpose(bic_ctx* ctx, const uint64_t* src, size_t rows, size_t cols, size_t wpr, uint64_t* dst,
                      size_t dst_wpr);
int bic_gf2_mul(bic_ctx* ctx, int op, const uint64_t* A, size_t a_rows, size_t a_cols, size_t a_wpr,
                const uint64_t* B, size_t b_rows, size_t b_cols, size_t b_wpr, uint64_t* C, size_t c_rows,
                size_t c_cols, size_t c_wpr);

/* ---- binary dictionary learning (bsvd.cpp) ----------------------------------------------------
 * The two alternating steps of the reference's dictionary learning and the loop around them, for
 * X = A D ^ E over GF(2): E (n x m) the residual, D (p x m) one atom per row, A (n x p) the
 * coefficients, X (n x m) the data; all in the plane layout, device memory, pitches e_wpr, d_wpr,
 * x_wpr >= ceil(m/64) and a_wpr >= ceil(p/64). Domain: 1 <= m <= 4096, 1 <= p <= 4096, n < 2^31;
 * outside it BIC_EINVAL; n = 0 is BIC_OK with changed = 0. The whole domain runs: where one launch's
 * grid cannot hold n rows (the transpose and the product behind these entries take 16,776,960 rows
 * per launch) the rows go in chunks. Padding bits are not masked: as the
 * reference's dist, weight and add (binmat.cpp:57-67, 463-512) the kernels run over the first
 * ceil(m/64) whole words of a row; the padding bits of D and A are never changed; words past a
 * row's own (the pitch) are neither read nor written. The caller supplies D and A, its own or those
 * of the model initialisers below (bic_bsvd_initialize).
 *
 * bic_bsvd_update_coefficients = update_coefficients_basic / _omp (bsvd.cpp:399-460, 1029-1107; the
 * same result, rows are independent): for each row i, repeat: w = weight(E_i), d_k = dist(E_i, D_k)
 * for every k, bestk the smallest k that attains the minimum (the scan runs k upward with a strict
 * <, :423-437); if d_bestk < w then E_i ^= D_bestk and A(i, bestk) is flipped (an atom may be
 * switched off again), else the row is done. Every step lowers weight(E_i): at most
 * 64 ceil(m/64) steps per row. changed (device u64, nullable) is written, not accumulated, with the
 * number of rows that took at least one step.
 *
 * bic_bsvd_update_dictionary = update_dictionary_steepest (bsvd.cpp:463-527; not the _omp variant,
 * whose counters race). The atoms are updated in order, k = 0 .. p - 1: U = the rows with A(i,k)
 * set (U = 0 skips the atom); c_j = how many of them have bit j of E_i ^ D_k set, j < m; the new
 * atom has bit j = (c_j > U / 2), integer division, and D_k's own padding bits; if it differs from
 * D_k, every using row gets E_i ^= D_k ^ new, D_k = new, and changed (device u64, nullable,
 * written) counts the atom. The order is part of the result: a row that uses atoms k1 < k2 carries
 * k1's change into k2's counts. Runs as launches ordered on the ctx stream, p + 1 of one kernel (or
 * one when a single workgroup owns every row), without host synchronisation and without any
 * workgroup waiting for another; the transpose of A and the counters live in the ctx scratch.
 *
 * Both steps can be stream-captured once the scratch has its size: it is sized on first use, so
 * call bic_bsvd_update_dictionary once with the same n and p before capturing.
 *
 * bic_bsvd_learn = learn_model_traditional (bsvd.cpp:1215-1244): E = A D ^ X (bic_gf2_mul with
 * BIC_GF2_AB, then a word-wise XOR), then the two steps alternate until the sum of their changed
 * counts is 0. iters (HOST pointer, nullable) receives the number of iterations run, the
 * reference's return value; max_iter = 0 means no cap (as the reference), otherwise the call stops
 * after max_iter iterations and still returns BIC_OK. This call blocks: it reads the two counts
 * back every iteration, so it returns after the work has completed and cannot be stream-captured. */
int bic_bsvd_update_coefficients(bic_ctx* ctx, uint64_t* E, size_t n, size_t m, size_t e_wpr, const uint64_t* D,
                                 size_t p, size_t d_wpr, uint64_t* A, size_t a_wpr, uint64_t* changed);
int bic_bsvd_update_dictionary(bic_ctx* ctx, uint64_t* E, size_t n, size_t m, size_t e_wpr, uint64_t* D, size_t p,
                               size_t d_wpr, const uint64_t* A, size_t a_wpr, uint64_t* changed);
int bic_bsvd_learn(bic_ctx* ctx, const uint64_t* X, size_t x_wpr, uint64_t* E, size_t n, size_t m, size_t e_wpr,
                   uint64_t* D, size_t p, size_t d_wpr, uint64_t* A, size_t a_wpr, size_t max_iter, size_t* iters);

/* bic_bsvd_update_dictionary_proximus = update_dictionary_proximus (bsvd.cpp:530-735; _omp, :822-1027,
 * is the same text), the rank-one refinement that moves an atom and its coefficients together.
 * Layout, domain, BIC_EINVAL cases and whole-word conventions are those of
 * bic_bsvd_update_dictionary; A is updated too. For every atom k = 0 .. p - 1 in order, rounds of two
 * halves until a round changes nothing:
 *   atom half (:628-671): the steepest step for this atom alone (U = 0 skips it); if D_k changes,
 *     its users get E_i ^= D_k ^ new over whole words.
 *   coefficient half (:676-719): S = the set bits of D_k for j < m (|S| = 0 skips it, so a zero atom
 *     keeps its users); for EVERY row, Aw_i = the bits j in S with E(i,j) ^ A(i,k) set; the new
 *     A(i,k) is Aw_i > |S| / 2 (integer division: a tie gives 0); where it differs, A(i,k) flips
 *     and E_i ^= D_k for j < m only (D_k's padding bits are not carried into E here).
 * An atom without users can recruit some in its coefficient half. changed (device u64, nullable,
 * written) receives the reference's return value: the atoms whose D_k changed in some round; an atom
 * whose users changed while its bits did not is not counted (bsvd.cpp:706 is commented out). rounds
 * (HOST pointer, nullable) receives the number of rounds run over all atoms. The reference's `#if 0`
 * correlation initialisation (:566-620) is not built. n = 0 is BIC_OK with changed = 0, rounds = 0.
 *
 * The number of rounds depends on the data and the atoms are ordered, so the host has to learn how
 * far the device got: per atom a budget of rounds is enqueued (two launches each; those of the
 * rounds an atom does not need leave at once), all atoms up front, and what the device reports is
 * read back once per batch; an atom that needs more than its budget is enqueued again with the atoms
 * after it. bic_bsvd_update_dictionary_proximus therefore blocks: it returns after the work has
 * completed and cannot be stream-captured. No workgroup ever waits for another. bic_set_bsvd_rounds
 * sets the budget (0 = automatic, else 1 .. 64; other values BIC_EINVAL); every value gives the
 * same result.
 *
 * bic_bsvd_learn_du is bic_bsvd_learn with the dictionary rule chosen: BIC_BSVD_DU_STEEPEST gives
 * bic_bsvd_learn itself (the same launches, the same result), BIC_BSVD_DU_PROXIMUS sums the
 * sparse-coding count and bic_bsvd_update_dictionary_proximus's changed count (so the loop may stop
 * after a call that moved only coefficients, as the reference's does); any other du is BIC_EINVAL.
 * It blocks and cannot be stream-captured, as bic_bsvd_learn. */
#define BIC_BSVD_DU_STEEPEST 0
#define BIC_BSVD_DU_PROXIMUS 1
int bic_bsvd_update_dictionary_proximus(bic_ctx* ctx, uint64_t* E, size_t n, size_t m, size_t e_wpr, uint64_t* D,
                                        size_t p, size_t d_wpr, uint64_t* A, size_t a_wpr, uint64_t* changed,
                                        size_t* rounds);
int bic_bsvd_learn_du(bic_ctx* ctx, int du, const uint64_t* X, size_t x_wpr, uint64_t* E, size_t n, size_t m,
                      size_t e_wpr, uint64_t* D, size_t p, size_t d_wpr, uint64_t* A, size_t a_wpr, size_t max_iter,
                      size_t* iters);
int bic_set_bsvd_rounds(bic_ctx* ctx, unsigned rounds);

/* ---- wide rows and the role-switching learners (bsvd.cpp:1247-1434) ----------------------------
 * bic_bsvd_update_coefficients_wide and bic_bsvd_update_dictionary_wide are the three steps above for
 * rows of any width. Domain: 1 <= m <= 1048576, 1 <= p <= 4096, n < 2^31; outside it BIC_EINVAL; n = 0
 * is BIC_OK with changed = 0 and rounds = 0 (under either rule). The meaning is, word for word, that of
 * bic_bsvd_update_coefficients, of bic_bsvd_update_dictionary (du = BIC_BSVD_DU_STEEPEST: rounds is
 * not written, A is only read) and of bic_bsvd_update_dictionary_proximus (du = BIC_BSVD_DU_PROXIMUS),
 * with every convention stated for them: whole words in distances, weights and XORs, D_k's last word
 * masked in the PROXIMUS coefficient vote, the padding bits of D and A never changed, words past a
 * row's own never touched, changed and rounds as defined there, bic_set_bsvd_rounds honoured with
 * every budget giving the same result; any other du is BIC_EINVAL. These entries always run the wide
 * kernels, whatever m, and give the narrow entries' outputs where m <= 4096.
 *
 * Sparse coding is one launch (a workgroup per row, repeated inside until no atom lowers the weight).
 * The steepest rule is one launch in which every chunk of 1,024 columns walks the p atoms by itself
 * (bit c of an atom depends on column c of E alone), and one that counts the atoms changed. PROXIMUS
 * keeps the narrow entry's schedule and therefore blocks, as that entry does; the other two do not
 * synchronise with the host. No workgroup ever waits for another. The scratch is the ctx's, sized on
 * first use.
 *
 * bic_bsvd_learn_lm runs a learner of the reference's catalogue. lm = BIC_BSVD_LM_TRADITIONAL is
 * bic_bsvd_learn_du for m up to 1048576: the same launches for m <= 4096, the wide steps above that.
 * lm = BIC_BSVD_LM_ALTER1, _ALTER2, _ALTER3 are learn_model_alter1 / 2 / 3 exactly as written: they
 * transpose A, D and E (bic_gf2_transpose, into the ctx scratch), run the same steps with the roles
 * exchanged -- update_coefficients(Et, At, Dt), update_dictionary(Et, At, Dt): Et (m x n) the
 * residual, At's p rows of n bits the atoms, Dt (m x p) the coefficients -- and transpose back. Kept
 * as the text has them:
 *   alter1 (:1247-1312): direct sparse coding and dictionary step, then the transposed pair; the loop
 *     goes on only on the transposed dictionary step's count (:1297 overwrites the sums before it), so
 *     it can stop with direct coefficient moves still pending.
 *   alter2 (:1315-1385): a direct loop to convergence, then a transposed one, repeated while either
 *     changed anything; `changed` is not reset before the direct loop of a second outer pass, so that
 *     loop is skipped; iter is reset before every transposed loop, so the return value is the last
 *     transposed loop's count.
 *   alter3 (:1388-1434): no sparse coding at all; the transposed dictionary step, then the direct one,
 *     and only the direct one's count decides.
 * transpose_to clears the padding (binmat.cpp:199-208): the transposed matrices have zero padding, and
 * after the transposes back the padding bits inside the words of E, D and A are zero (words past a
 * row's own are untouched); the direct steps before the first switch still see the caller's padding.
 * Domain for lm >= 1: 1 <= m <= 1048576, 1 <= n <= 1048576, 1 <= p <= 4096 (BIC_ENOMEM where the
 * transposes do not fit the device). Each half uses the narrow kernels where its rows have at most
 * 4096 bits and the wide ones above; the result is the same either way. max_iter (0 = none) caps the
 * loop passes, every iter++ of the text, counted over the whole call: the pass that reaches the cap is
 * finished, transposes back included, and the call returns BIC_OK. iters (HOST pointer, nullable)
 * receives the reference's return value. The call blocks, as bic_bsvd_learn. Any other lm or du is
 * BIC_EINVAL. */
#define BIC_BSVD_LM_TRADITIONAL 0
#define BIC_BSVD_LM_ALTER1 1
#define BIC_BSVD_LM_ALTER2 2
#define BIC_BSVD_LM_ALTER3 3
int bic_bsvd_update_coefficients_wide(bic_ctx* ctx, uint64_t* E, size_t n, size_t m, size_t e_wpr, const uint64_t* D,
                                      size_t p, size_t d_wpr, uint64_t* A, size_t a_wpr, uint64_t* changed);
int bic_bsvd_update_dictionary_wide(bic_ctx* ctx, int du, uint64_t* E, size_t n, size_t m, size_t e_wpr, uint64_t* D,
                                    size_t p, size_t d_wpr, uint64_t* A, size_t a_wpr, uint64_t* changed,
                                    size_t* rounds);
int bic_bsvd_learn_lm(bic_ctx* ctx, int lm, int du, const uint64_t* X, size_t x_wpr, uint64_t* E, size_t n, size_t m,
                      size_t e_wpr, uint64_t* D, size_t p, size_t d_wpr, uint64_t* A, size_t a_wpr, size_t max_iter,
                      size_t* iters);

/* ---- model initialisers (bsvd.cpp:99-267) -----------------------------------------------------
 * The four rules the reference starts a dictionary from: D (p x m) and A (n x p) are made from the data
 * E (n x m, const), which the driver passes as E = X before learning (bsvd_test.cpp:114-119).
 * initialize_model_graph_grow and the file-static initialize_model_random are not built. Layout and
 * pitches as above. Domain: 1 <= m, p <= 4096, 1 <= n < 2^31, pitches at least the row's words, no null
 * matrix; anything else is BIC_EINVAL, n = 0 too: nothing can be initialised from no data.
 *
 * Padding differs from the steps above: every read of E here is masked at the trailing word, as get(i, j)
 * with j < m, weight(), bool_and and add are (they go through get_block, binmat.h:188-190), so E's
 * padding bits are ignored. All four rules start with A.clear() and D.clear(): the first ceil(m/64) words of
 * every row of D and the first ceil(p/64) words of every row of A are written, with zero padding bits;
 * words past a row's own (the pitch) are neither read nor written.
 *
 * BIC_BSVD_MI_NEIGHBOR (:227-267), bic_bsvd_init_neighbor with rows (DEVICE, p row indices), atom k from
 * the pick i = rows[k]: N = the rows j, i among them, with E_j & E_i != 0 over columns < m, u = |N|,
 * s_c = the rows of N with bit c of E_j & E_i set; D(k, c) = (s_c >= u / 2) for c < m, integer division.
 * So u = 1 gives an all-ones atom (0 >= 0 in every column), u = 2 or 3 gives E_i, and for u >= 2 the atom
 * lies inside the pick's support. The same row may be picked twice. A stays zero. A pick whose masked
 * weight is 0 leaves its atom zero (the reference never makes such a pick), and so does an index >= n,
 * which is skipped, never dereferenced.
 *
 * BIC_BSVD_MI_PARTITION (:173-219), bic_bsvd_init_partition: w_c = col_weight(c) as written
 * (binmat.cpp:80-92): it counts bit c over rows 0 .. ceil(n / ceil(m/64)) - 1 only, all rows only when
 * m <= 64. The columns are ranked by (w_c descending, c ascending), which is what counting_sort
 * (util.cpp:7-51) and ranking[m-k-1] yield. For k < min(p, m) the pivot is the k-th ranked column, the
 * members are ALL rows with E(i, pivot) set, u their number, s_c their count of bit c;
 * D(k, c) = (s_c >= u / 2), so u = 0 or 1 gives all ones. Atoms k >= m stay zero. A stays zero. No random
 * numbers are used.
 *
 * BIC_BSVD_MI_CENTROIDS (:128-166), bic_bsvd_init_centroids with atom_of_row (DEVICE, n entries < p):
 * A(i, atom_of_row[i]) = 1; u_k = the rows of atom k, s_kc their count of bit c;
 * D(k, c) = (2 s_kc >= u_k): a tie sets the bit and an atom without rows is all ones.
 * BIC_BSVD_MI_CENTROIDS_XOR (:99-126): the same A; D_k = the XOR of the masked rows of atom k, an atom
 * without rows is zero. An entry >= p is skipped: its row of A stays zero and it joins no atom.
 *
 * The three explicit entries only enqueue device work on the ctx stream: a fixed number of launches
 * whatever n and p (the rows are walked in shares), no host synchronisation, no workgroup ever waits for
 * another. Their counters live in the ctx scratch and are cleared by the call itself; the scratch is
 * sized on first use, as for bic_bsvd_update_dictionary.
 *
 * The generator is GSL's gsl_rng_rand48, the Unix rand48 sequence, with its state explicit (the
 * reference keeps one per process, seeded with random_seed = 34503498 on first use). bic_bsvd_rng_seed
 * (host only): state = (s << 16) | 0x330E with s the low 32 bits of seed, 0x1234ABCD330E for s = 0. One
 * output: state = (0x5DEECE66D state + 0xB) mod 2^48, the output is state >> 16. bic_bsvd_rng_uniform
 * (host only) is gsl_rng_uniform_int, count times: scale = 0xFFFFFFFF / bound, k = output / scale is drawn
 * until k < bound, and a rejected output is used up; out (HOST) receives count values; bound = 0, a
 * null state or a null out with count > 0 is BIC_EINVAL.
 *
 * bic_bsvd_initialize is the reference's call: it draws on the host from *state (HOST, in and out; may
 * be NULL for PARTITION, otherwise NULL is BIC_EINVAL), uploads what it drew and runs the explicit
 * entry. NEIGHBOR: one kernel writes the bitmap "row is non-zero over j < m" into the ctx scratch, the
 * host reads its n / 8 bytes back and draws p picks with bic_bsvd_rng_uniform's rule and bound n, where
 * a zero row is drawn again and uses up its draw (:243); if no row is non-zero it returns BIC_EINVAL
 * with *state unchanged (the reference would loop forever). CENTROIDS and CENTROIDS_XOR: n draws with
 * bound p, in row order. NEIGHBOR and both CENTROIDS kinds block: they return after the work has
 * completed and cannot be stream-captured. PARTITION does not block. Any other mi is BIC_EINVAL. */
#define BIC_BSVD_MI_NEIGHBOR 0
#define BIC_BSVD_MI_PARTITION 1
#define BIC_BSVD_MI_CENTROIDS 2
#define BIC_BSVD_MI_CENTROIDS_XOR 3
int bic_bsvd_rng_seed(uint64_t seed, uint64_t* state);
int bic_bsvd_rng_uniform(uint64_t* state, uint32_t bound, size_t count, uint32_t* out);
int bic_bsvd_init_neighbor(bic_ctx* ctx, const uint64_t* E, size_t n, size_t m, size_t e_wpr, uint64_t* D, size_t p,
                           size_t d_wpr, uint64_t* A, size_t a_wpr, const uint32_t* rows);
int bic_bsvd_init_partition(bic_ctx* ctx, const uint64_t* E, size_t n, size_t m, size_t e_wpr, uint64_t* D, size_t p,
                            size_t d_wpr, uint64_t* A, size_t a_wpr);
int bic_bsvd_init_centroids(bic_ctx* ctx, int mi, const uint64_t* E, size_t n, size_t m, size_t e_wpr, uint64_t* D,
                            size_t p, size_t d_wpr, uint64_t* A, size_t a_wpr, const uint32_t* atom_of_row);
int bic_bsvd_initialize(bic_ctx* ctx, int mi, const uint64_t* E, size_t n, size_t m, size_t e_wpr, uint64_t* D,
                        size_t p, size_t d_wpr, uint64_t* A, size_t a_wpr, uint64_t* state);

/* ---- MDL model order (bsvd.cpp:1438-1717) -------------------------------------------------------
 * model_codelength and the three searches that choose the number of atoms: learn_model_mdl_forward_selection,
 * _backward_selection and _full_search. Layout and pitches as above; E (n x m), D (p x m), A (n x p).
 *
 * The four primitives only enqueue on the ctx stream: no host synchronisation, no workgroup ever waits for
 * another, scratch from the ctx arena sized on first use, so they can be stream-captured after one warm-up call
 * with the same sizes. Their sums are integer adds: results are run-to-run identical. Every read of E, D and A
 * is masked at the row's trailing word, as weight() behind copy_row_to / copy_col_to and mul_AtB / add are (they
 * go through get_block, binmat.h:188-190): dirty padding bits never count. Words past a row's own are neither
 * read nor written. Domain: 1 <= m <= 1048576, 0 <= p <= 4096, 1 <= n < 2^31, pitches at least the row's
 * words; anything else is BIC_EINVAL.
 *
 * bic_bsvd_model_weights: *we (DEVICE u64) = the weight of E over columns < m; wd[k] (DEVICE u32 x p) = the
 * weight of D_k over columns < m; wa[k] (DEVICE u32 x p) = the rows with A(i, k) set. p = 0 writes we alone (D,
 * A, wd and wa may be NULL).
 * bic_bsvd_drop_weights (p >= 1): w[k] (DEVICE u64 x p) = the masked weight of E ^ (A_k^t D_k), the residual
 * once atom k is taken out of its users (mul(Ak, true, Dk, false, AkDk); add(AkDk, E, nextE), :1580-1582): the
 * weight of E plus, over the rows i with A(i, k) set, |E_i ^ D_k| - |E_i|. The work is proportional to A's set
 * bits times the row's words; D is read where it lies, nothing is staged, so no p x m has to fit anywhere.
 * bic_bsvd_drop_atom (1 <= p, k < p): in place, row k of D is removed (the rows after it move down one row,
 * their ceil(m/64) words as they are; row p - 1 is left as it was) and column k of A is removed (in every row
 * the columns after k move one place towards the MSB, across word boundaries); the vacated column p - 1 and
 * all padding bits inside the row's ceil(p/64) words become 0. The caller goes on with p - 1.
 * bic_bsvd_append_atom (0 <= p <= 4095): row p of D = atom (1 x m, DEVICE, masked at m: the new row's padding
 * bits are zero), column p of A = bit 63 of every row of coefs (n x 1, DEVICE, pitch c_wpr >= 1), and A's
 * bits after column p inside its ceil((p+1)/64) words are zero. The caller guarantees room: D has a row p and
 * a_wpr >= ceil((p+1)/64). This is what allocate and two set_submatrix calls leave at :1497-1513, where the
 * reference's padding is uninitialised memory; this build defines it as zero.
 *
 * bic_universal_codelength (host only) is coding.cpp's universal_codelength: n H(r/n) + log2(n)/2, and
 * log2(n)/2 alone for r = 0 or r >= n. bic_bsvd_model_codelength blocks: it runs bic_bsvd_model_weights, reads
 * the 1 + 2p numbers back and evaluates :1438-1461 as written: universal_codelength takes 32-bit arguments, so
 * rows*cols and the weights are truncated to 32 bits (a product that truncates to 0 is BIC_EINVAL); LE is the
 * double truncated to a u64; LD += double and LA += double convert the running sum to double, add, and truncate
 * toward zero on every term. *len (HOST) = LE + LD + LA, LE alone for p = 0.
 *
 * bic_bsvd_learn_mdl runs one search and blocks. search: BIC_BSVD_MDL_FORWARD, _BACKWARD or _FULL; lmi the
 * inner learner (BIC_BSVD_LM_*, bic_bsvd_learn_lm with max_iter 0); du its dictionary rule; mi the initialiser
 * (BIC_BSVD_MI_*, forward and full search only, drawing from *rng_state as bic_bsvd_initialize). X (n x m,
 * const); E, D (p_cap rows), A (a_wpr >= ceil(p_cap/64)) hold the caller's model of p atoms on entry and receive
 * the reference's outputs: *p_out atoms (the first *p_out rows of D and ceil(*p_out/64) words of every row of
 * A; what lies after them is left as it was, or holds the search's intermediate models), *best_len the
 * reference's return value. All working copies live in the ctx arena. Domain: that of the parts a search uses:
 * 1 <= p <= p_cap <= 4096; m <= 4096 where an initialiser runs (forward, full), else m <= 1048576; n < 2^31, and
 * 1 <= n, m <= 1048576 for lmi >= 1; otherwise BIC_EINVAL. The text's behaviour is kept as written, what look
 * like slips included:
 *  - lengths and the stuck statistics are unsigned 64-bit (idx_t): sumStuck += currL - bestL wraps,
 *    dev = int(sumStuck / allStuck) keeps the low 32 bits and is sign-extended in currL + dev < bestL, and
 *    dif = int(currL) - int(bestL);
 *  - forward (:1463-1546): the inner learner runs on the caller's model, then every pass initialises ONE atom
 *    from the current residual (bic_bsvd_initialize with p = 1), appends it, learns and measures; the current
 *    model grows every pass, accepted or not; ten consecutive rejected passes stop the search. The reference has
 *    no bound on K: here a pass that would need K + 1 > p_cap stops the call with BIC_ENOSPC (its trace record is
 *    still produced), and a neighbour rule that finds no non-zero row stops it with bic_bsvd_initialize's
 *    BIC_EINVAL; either way the best model so far is in the outputs;
 *  - backward (:1548-1663): the K removal scores of a pass use the caller-visible E, i.e. the BEST model's
 *    residual and not the current one's, with the current D and A; the score of k is
 *    model_codelength(E ^ A_k^t D_k, D, A), then -= universal_codelength(M, |D_k|), then -= universal_codelength(N,
 *    |A_k|), each -= through double and truncated; the smallest k at the minimum wins (strict <) and the start
 *    value is ~(1UL << (sizeof(idx_t) - 1)) = 0xFFFFFFFFFFFFFF7F; the current model shrinks every pass, accepted
 *    or not. At K = 1 the candidate is the empty model, scored with the residual the k = 0 score left; if it is
 *    accepted, *p_out = 0, E = X, and *best_len keeps its previous value (the break precedes the assignment);
 *  - full search (:1665-1717): k = 20, 40, .. <= p; per k one initialise + learn whose result is thrown away (its
 *    draws are used up), then 10 repetitions of initialise + learn + length; candL is the minimum of the ten, but
 *    the model copied out on candL < bestL is the LAST repetition's, not the minimum's; bestL starts at 1 << 30;
 *    p < 20 leaves E, D and A untouched, *p_out = 0 and *best_len = 1 << 30. (The random_seed arithmetic of
 *    the loop changes no draw: the generator is seeded once.)
 * trace (HOST, nullable) receives one bic_bsvd_mdl_step per pass, at most trace_cap of them; *trace_len is the
 * number of passes run, even when trace_cap is smaller. A record holds what the reference prints at the start
 * of the pass (K, currL, bestK, bestL, stuck, dif, dev); backward adds the atom it then chose. Full search: one
 * record per k with K = k, currL = candL, bestK and bestL after the comparison, and the ten lengths in lens. */
#define BIC_BSVD_MDL_FORWARD 0
#define BIC_BSVD_MDL_BACKWARD 1
#define BIC_BSVD_MDL_FULL 2
typedef struct bic_bsvd_mdl_step {
  uint64_t K, currL, bestK, bestL, stuck;
  int32_t dif, dev;
  uint32_t atom;      /* backward: the atom removed in this pass */
  uint32_t reserved;
  uint64_t lens[10];  /* full search: the ten lengths of this k */
} bic_bsvd_mdl_step;
double bic_universal_codelength(unsigned n, unsigned r);
int bic_bsvd_model_weights(bic_ctx* ctx, const uint64_t* E, size_t n, size_t m, size_t e_wpr, const uint64_t* D,
                           size_t p, size_t d_wpr, const uint64_t* A, size_t a_wpr, uint64_t* we, uint32_t* wd,
                           uint32_t* wa);
int bic_bsvd_drop_weights(bic_ctx* ctx, const uint64_t* E, size_t n, size_t m, size_t e_wpr, const uint64_t* D,
                          size_t p, size_t d_wpr, const uint64_t* A, size_t a_wpr, uint64_t* w);
int bic_bsvd_drop_atom(bic_ctx* ctx, uint64_t* D, size_t p, size_t m, size_t d_wpr, uint64_t* A, size_t n,
                       size_t a_wpr, size_t k);
int bic_bsvd_append_atom(bic_ctx* ctx, uint64_t* D, size_t p, size_t m, size_t d_wpr, uint64_t* A, size_t n,
                         size_t a_wpr, const uint64_t* atom, size_t atom_wpr, const uint64_t* coefs, size_t c_wpr);
int bic_bsvd_model_codelength(bic_ctx* ctx, const uint64_t* E, size_t n, size_t m, size_t e_wpr, const uint64_t* D,
                              size_t p, size_t d_wpr, const uint64_t* A, size_t a_wpr, uint64_t* len);
int bic_bsvd_learn_mdl(bic_ctx* ctx, int search, int lmi, int du, int mi, const uint64_t* X, size_t x_wpr,
                       uint64_t* E, size_t n, size_t m, size_t e_wpr, uint64_t* D, size_t p, size_t p_cap,
                       size_t d_wpr, uint64_t* A, size_t a_wpr, uint64_t* rng_state, size_t* p_out,
                       uint64_t* best_len, bic_bsvd_mdl_step* trace, size_t trace_cap, size_t* trace_len);

/* ---- image mode (bsvd_test.cpp:78-151, util.cpp:53-82) ------------------------------------------
 * What the driver does around the learner when its input is an image: the W x W tiles of a plane become the
 * samples, the residual's rows go back into an image, and D or E is drawn as a mosaic of small tiles. Plane
 * layout and device memory as everywhere; pitches in words. Each of the three kernels is one launch whatever the
 * size, enqueued on the ctx stream: no host synchronisation, no workgroup ever waits for another, no scratch, so
 * they can be stream-captured. Domain: rows, cols, n >= 1, rows < 2^31, cols < 2^31 - 1, 1 <= W <= 1024 (W^2 <=
 * 1048576, the steps' limit on m), 1 <= m <= 1048576, the number of patches and n < 2^31, every pitch at least
 * the row's own words, no null pointer; anything else is BIC_EINVAL before any launch.
 *
 * bic_patches_gather = bsvd_test.cpp:89-97 (copy_submatrix_to + copy_vectorized_to + set_row). Ny = ceil(rows/W),
 * Nx = ceil(cols/W); patch li = ti Nx + tj is row li of X (N x W^2, N = Ny Nx). Bit r W + c of that row (r, c < W)
 * is the plane's FLAT bit at row ti W + r, column tj W + c, the flat read of get_submatrix (binmat.cpp:267-298)
 * that bic_dict_encode and bic_patch_search use: a row is its first ceil(cols/64) words and the word after them
 * is the next row's first word, so a tile that runs past the right edge continues with the next row's pixels,
 * as far as it reaches; the pad bits of a row's last word are read as stored; anything past the last row reads
 * 0; the words between ceil(cols/64) and wpr are never read. The first ceil(W^2/64) words of every row of X are
 * written, with pad bits 0 (copy_vectorized_to reads its tile through get_block); words up to x_wpr are neither
 * read nor written. The host binary_matrix of this build defines the reference's shift by 64 in
 * copy_vectorized_to as 0; with that the three host calls give these words exactly.
 *
 * bic_patches_scatter = bsvd_test.cpp:130-139 (copy_row_to + set_vectorized + set_submatrix). Pixel (i, j) with
 * i < rows, j < cols becomes bit (i mod W) W + (j mod W) of row (i / W) Nx + j / W of X; tile rows and columns
 * past the image are dropped. Every pixel belongs to exactly one tile, so the plane is written, never read: the
 * first ceil(cols/64) words of every row, with pad bits 0; the pitch words are left untouched. One difference
 * from the host: set_submatrix leaves an edge tile's bits in the pad columns it covers (and keeps what the pad
 * held elsewhere); this build writes zero padding, as the learners do. The valid pixels are the same.
 *
 * bic_mosaic_dims (host only) and bic_mosaic = render_mosaic's image (util.cpp:53-82) of D (n x m): w = the
 * largest integer with w^2 <= m, gn = the smallest with gn^2 >= n, gm = ceil(n / gn), gw = w + 1; the image is
 * gm gw rows x gn gw columns (*rows, *cols). Pixel (gw i + r, gw j + c) = D(i gn + j, r w + c) for r, c < w and
 * i gn + j < n; every other bit of the rows' own words, pad bits included, is 0 (zero padding, as every output
 * here); bits w^2 .. m - 1 of an atom are ignored; the image's pitch words are left untouched. The integer
 * arithmetic gives what the reference's (idx_t)sqrt(double(m)), ceil(sqrt(double(n))) and ceil(double(n)/gn)
 * give in this domain: doubles hold these integers exactly, sqrt is correctly rounded, and a quotient that is
 * not an integer lies at least 2^-16 from one.
 *
 * bic_bsvd_learn_image is the body of bsvd_test.cpp:78-145 in image mode, in this order: bic_patches_gather into
 * X; E = X (the rows' own words, device to device); bic_bsvd_initialize(mi, E, .., rng_state);
 * bic_bsvd_learn_lm(lm, du, X, E, .., max_iter, iters); and, if residual is not NULL, bic_patches_scatter of E into
 * it (rows x cols, pitch r_wpr). n = Ny Nx and m = W^2 follow from the image. Its results are bit for bit those of
 * the five separate calls, *rng_state and *iters included. Its domain is the intersection of theirs: W <= 64 (the
 * initialisers take m <= 4096), 1 <= p <= 4096, n <= 1048576 for lm >= 1, rng_state as bic_bsvd_initialize; anything
 * else is BIC_EINVAL before any launch. It blocks where they block and adds no kernel of its own. */
int bic_patches_gather(bic_ctx* ctx, const uint64_t* plane, size_t rows, size_t cols, size_t wpr, unsigned W,
                       uint64_t* X, size_t x_wpr);
int bic_patches_scatter(bic_ctx* ctx, const uint64_t* X, size_t x_wpr, unsigned W, uint64_t* plane, size_t rows,
                        size_t cols, size_t wpr);
int bic_mosaic_dims(size_t n, size_t m, size_t* rows, size_t* cols);
int bic_mosaic(bic_ctx* ctx, const uint64_t* D, size_t n, size_t m, size_t d_wpr, uint64_t* image, size_t i_wpr);
int bic_bsvd_learn_image(bic_ctx* ctx, int mi, int lm, int du, const uint64_t* plane, size_t rows, size_t cols,
                         size_t wpr, unsigned W, uint64_t* X, size_t x_wpr, uint64_t* E, size_t e_wpr, uint64_t* D,
                         size_t p, size_t d_wpr, uint64_t* A, size_t a_wpr, uint64_t* rng_state, size_t max_iter,
                         size_t* iters, uint64_t* residual, size_t r_wpr);

/* ---- kernel timing ------------------------------------------------------------------------
 * When enabled, every kernel launch of this ctx is bracketed by HIP events on the launch stream.
 * bic_prof_collect syncs, writes one line per kernel name ("name launches total_ms\n") into buf
 * and clears the records. */
int bic_prof_enable(bic_ctx* ctx, int on);
int bic_prof_collect(bic_ctx* ctx, char* buf, size_t cap);
/* Restrict the bracketing to launches recorded under `name` (NULL or "" = every launch). Each
 * event pair costs the step a few microseconds of pipeline drain, so a timed region that needs
 * one kernel's duration brackets only that kernel. */
int bic_prof_only(bic_ctx* ctx, const char* name);

#ifdef __cplusplus
}
#endif
#endif
