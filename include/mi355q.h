/*
 * mi355q.h -- C ABI of libmi355q.so: MI355X (gfx950) kernels for the AI Edge
 * Quantizer calibration + requantization hot path.
 *
 * This is the drop-in boundary. The reference has no native
 * code; each entry point below replaces a NumPy/SciPy routine of the reference
 * (cited as `ref:` relative to /root/reference/ai_edge_quantizer/). The Python
 * mirror of the reference's plugin interface (ai-edge-quantizer_amd/mi355q) binds
 * these symbols with ctypes; INTEGRATION.md shows the stub a reference maintainer
 * would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the parameter name ends in _host;
 *   - the caller owns every buffer; the library never allocates, frees or retains
 *     caller memory and keeps no state besides a thread-local error string;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); calls
 *     only enqueue work, they never synchronize;
 *   - functions return 0 on success or a negative mi355q_status; a message is
 *     available from mi355q_last_error();
 *   - weights are row-major FP32, `rows x cols` with `cols` contiguous (LiteRT
 *     FULLY_CONNECTED / EMBEDDING_LOOKUP layout [out, in]);
 *   - integer outputs are bit-exact with the reference (IEEE division, round half
 *     to even, NaN -> 0 in 8/16-bit and INT32_MIN in 32-bit containers, as NumPy's
 *     x86 cast); see DESIGN.md for the parity contract.
 */
#ifndef MI355Q_H_
#define MI355Q_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI355Q_VERSION 100 /* 0.1.0 */

typedef enum mi355q_status {
  MI355Q_OK = 0,
  MI355Q_BAD_ARG = -1,     /* null pointer, negative size, bad enum value */
  MI355Q_BAD_SHAPE = -2,   /* e.g. cols not divisible by block size */
  MI355Q_UNSUPPORTED = -3, /* valid request this build has no kernel for */
  MI355Q_HIP_ERROR = -4,   /* launch / runtime failure; see mi355q_last_error() */
  MI355Q_RCCL_ERROR = -5,  /* RCCL missing or a collective / communicator call failed */
  MI355Q_IO_ERROR = -6     /* pread / pwrite on a model file failed or came up short */
} mi355q_status;

int32_t mi355q_version(void);
/* Thread-local message of the last failing call on this thread ("" if none). */
const char* mi355q_last_error(void);
/* Device facts the host side uses for launch geometry and bench reporting. */
int32_t mi355q_device_info(int32_t* cu_count_host, int32_t* wavefront_size_host,
                           char* arch_name_host, int32_t arch_name_len);

/* ------------------------------------------------------------------------
 * K1 -- weight min / max.
 * ref: algorithms/uniform_quantize/common_quantize.py:1311-1359 (init_tensor_min_max)
 *
 * x is viewed as [outer, channels, inner] (row-major); min/max are reduced over
 * `outer` and `inner` for every channel:
 *   TENSORWISE            outer=1, channels=1,            inner=numel
 *   CHANNELWISE dim 0     outer=1, channels=shape[0],     inner=numel/shape[0]
 *   CHANNELWISE last dim  outer=numel/shape[-1], channels=shape[-1], inner=1
 *   BLOCKWISE_b (dim 1)   outer=1, channels=rows*cols/b,  inner=b
 * NaN propagates (np.min / np.max semantics).
 * workspace: mi355q_minmax_workspace_bytes(...) bytes of scratch (may be NULL
 * when that returns 0).
 * ------------------------------------------------------------------------ */
size_t mi355q_minmax_workspace_bytes(int64_t outer, int64_t channels, int64_t inner);
int32_t mi355q_minmax_f32(const float* x, int64_t outer, int64_t channels, int64_t inner,
                          float* min_out, float* max_out, void* workspace,
                          size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * K1+K2+K3(+K4) fused -- symmetric min/max requantization of a weight buffer.
 * ref: naive_min_max_quantize.py:34-110 (get_tensor_quant_params) =
 *      common_quantize.py:1311-1359 (min/max)
 *    + uniform_quantize_tensor.py:492-586 (scale; zero point is 0)
 *    + uniform_quantize_tensor.py:273-362 (divide, rint, clip, cast)
 *    + transformations/transformation_utils.py:293-353 (pack_data, optional)
 *
 *   block == 0 : CHANNELWISE on dim 0 -- one scale per row: scale[rows]
 *   block  > 0 : BLOCKWISE along cols -- scale[rows, cols/block], rounded
 *                f32 -> bf16 (RNE) -> f16 -> f32 as the reference does; block must
 *                be a multiple of 4 and divide cols
 *   bits       : 8, 4 or 2 (signed; narrow range [-127,127] only for 8 bits)
 *   clip       : NULL, or per-scale absolute clipping constants (OCTAV) applied as
 *                bound = clip(max|x|, -c, c) (+ the f16 range cap when blockwise)
 *   q_out      : NULL, or int8[rows*cols] unpacked values (UniformQuantParams.quantized_data)
 *   packed_out : NULL, or the bytes quantize_tensor stores in the flatbuffer:
 *                bits=8 -> same as q_out; bits=4 -> rows*cols/2 bytes, element 0 in
 *                the low nibble; bits=2 -> rows*cols/4 bytes. Requires
 *                rows*cols % (8/bits) == 0 (use mi355q_pack_bits for ragged tails).
 *   scale_out  : float[n_scales] (required)
 *   scale_f16_out : NULL, or uint16[n_scales] IEEE half bit patterns of
 *                f16(bf16(scale)) -- what transformations/quantize_tensor.py:129-137
 *                stores in the `<name>_scales` tensor. Blockwise only: with block == 0 the
 *                reference rounds no scale and nothing is written here
 * One HBM read of x; scales, q and packed bytes are written once.
 * x, q_out and packed_out 16-byte aligned with cols % 4 == 0, cols <= 16384 (block == 0) or
 * block in {32, 64, 128, 256} take the vector kernels; anything else takes a generic kernel
 * with the same results, which packs nothing below 8 bits (MI355Q_UNSUPPORTED, nothing written).
 * A NaN scale has NumPy's bits: 0x7FC00000 from NaN data and from any blockwise scale,
 * the sign of -clip from a NaN clip with block == 0 (np.clip hands back its lower bound).
 * ------------------------------------------------------------------------ */
int32_t mi355q_requant_sym_f32(const float* x, int64_t rows, int64_t cols, int32_t block,
                               int32_t bits, const float* clip, int8_t* q_out,
                               uint8_t* packed_out, float* scale_out,
                               uint16_t* scale_f16_out, void* stream);

/* Same, over `count` equally shaped weight buffers in ONE launch (model-level
 * batching of ParamsGenerator's per-op loop, ref: params_generator.py:110-183).
 * The pointer tables themselves live in device memory. Any output table may be
 * NULL (that output is skipped for all tensors); clip is not supported here.
 * The tables cannot be read on the host, so nothing about the buffers is checked:
 * every x must be 16-byte aligned, and every q / packed buffer aligned to the
 * widest store of the kernel (8 bytes always suffice; equally shaped consecutive
 * slices of one 16-byte aligned allocation comply on every route). */
int32_t mi355q_requant_sym_f32_batched(const float* const* x_ptrs, int32_t count,
                                       int64_t rows, int64_t cols, int32_t block,
                                       int32_t bits, int8_t* const* q_ptrs,
                                       uint8_t* const* packed_ptrs,
                                       float* const* scale_ptrs,
                                       uint16_t* const* scale_f16_ptrs, void* stream);

/* The same launch with the pointer tables in HOST memory, read before the call returns: the device pointers travel
 * inside the kernel arguments (16 buffers per dispatch; more than 16 leave as several dispatches), so a group of weights
 * needs no host-to-device copy of its tables in front of its launch -- on an in-order stream that copy's completion
 * signal, not its few hundred bytes, costs ~10 us per launch against 14 us of kernel per 4096 x 4096 buffer. What
 * requant_queue issues for the resident weights of ParamsGenerator's per-op loop (ref: params_generator.py:162-183).
 * Inputs must be 16-byte aligned (outputs as in the device-table form; both are checked here and MI355Q_BAD_ARG names
 * the entry); entries of x / scale tables must not be NULL. */
int32_t mi355q_requant_sym_f32_batched_hostptrs(const float* const* x_ptrs_host, int32_t count,
                                                int64_t rows, int64_t cols, int32_t block,
                                                int32_t bits, int8_t* const* q_ptrs_host,
                                                uint8_t* const* packed_ptrs_host,
                                                float* const* scale_ptrs_host,
                                                uint16_t* const* scale_f16_ptrs_host, void* stream);

/* ------------------------------------------------------------------------
 * K3 -- uniform quantize with given parameters ("T1" path; also asymmetric,
 * tensorwise and channel-last layouts).
 * ref: uniform_quantize_tensor.py:273-362
 *
 * x is viewed as [outer, channels, inner]; scale/zero_point have `channels`
 * entries (1 for TENSORWISE; rows*cols/b with inner=b for BLOCKWISE).
 *   q = cast(clip(rint(x / scale[c] + zp[c]), lo, hi)),  lo = qmin + (narrow ? 1 : 0)
 *   scale_is_f64 : scale points at double[channels]; the division and the zero-point
 *                  add are then done in FP64 as NumPy does for a float64 scale
 *   zero_point   : NULL (all zero) or int32[channels]
 *   zp_via_f64   : the reference adds an int32/int64 zero point in FP64 and rounds
 *                  back to FP32 (np.add(f32, int32, out=f32)); int8/int16 zero points
 *                  are added in FP32. Pass 1 for the former.
 *   out_bits     : container of q_out: 8 -> int8, 16 -> int16, 32 -> int32. A NaN quotient
 *                  casts as NumPy's does on x86: 0 in int8 / int16, INT32_MIN in int32 (as does
 *                  a value past the int32 range), for either scale type
 * ------------------------------------------------------------------------ */
int32_t mi355q_quantize_f32(const float* x, int64_t outer, int64_t channels, int64_t inner,
                            const void* scale, int32_t scale_is_f64,
                            const int32_t* zero_point, int32_t zp_via_f64, int32_t bits,
                            int32_t narrow, int32_t out_bits, void* q_out, void* stream);

/* (q - zp) * scale. ref: uniform_quantize_tensor.py:365-409.
 * q is int8/int16/int32 per in_bits; same [outer, channels, inner] view.
 *   scale_is_f64 : scale points at double[channels] (NumPy multiplies by the float64 scale);
 *                  needs out_is_f64
 *   diff_bits    : width NumPy subtracts in = promoted type of (q, zero_point):
 *                  8 when both are int8 (the difference wraps, as in the reference),
 *                  16 / 32 (wraps likewise), 64 (an int64 zero point: no wrap)
 *   out_is_f64   : 0 -> float32 out (int8/int16 times float32 scale);
 *                  1 -> double out (NumPy promotes int32 / int64 * float32 and anything
 *                  * float64 to float64) */
int32_t mi355q_dequantize_f32(const void* q, int32_t in_bits, int64_t outer,
                              int64_t channels, int64_t inner, const void* scale,
                              int32_t scale_is_f64, const int32_t* zero_point,
                              int32_t diff_bits, int32_t out_is_f64, void* out, void* stream);

/* ------------------------------------------------------------------------
 * float_casting -- float32 weights stored as float16 (round to nearest even, overflow -> inf,
 * subnormals kept), i.e. `weight.astype(np.float16)`.
 * ref: algorithms/nonlinear_quantize/float_casting.py:157-160, 272-275
 * ------------------------------------------------------------------------ */
int32_t mi355q_cast_f32_to_f16(const float* x, int64_t n, uint16_t* out, void* stream);

/* ------------------------------------------------------------------------
 * K4 -- bit packing of int4 / int2 values held in int8 containers.
 * ref: transformations/transformation_utils.py:293-353 (pack_data)
 * out has ceil(n * bits / 8) bytes; element 0 sits in the lowest bits; the ragged
 * tail is zero padded. bits=8 copies.
 * ------------------------------------------------------------------------ */
int32_t mi355q_pack_bits(const int8_t* q, int64_t n, int32_t bits, uint8_t* out,
                         void* stream);
/* The inverse: n sign-extended int8 values from ceil(n * bits / 8) packed bytes. The fused
 * requantization of sub-byte targets writes only the packed bytes the model file stores
 * (4.5 instead of 5.5 bytes of HBM traffic per int4 weight); the int8 containers of
 * UniformQuantParams.quantized_data (ref: uniform_quantize_tensor.py:357-360 yields them,
 * transformations/quantize_tensor.py:176-194 packs them) are produced from those bytes only
 * if a caller actually reads them. */
int32_t mi355q_unpack_bits(const uint8_t* packed, int64_t n, int32_t bits, int8_t* q_out,
                           void* stream);

/* ------------------------------------------------------------------------
 * K7 -- activation statistics: scalar min over x > lo, max over x < hi, with the
 * all-masked fallback to the plain min / max.
 * ref: common_quantize.py:1362-1413 (get_activation_min_max)
 *
 * Processes `count` tensors (one calibration sample each, or any mix) in one
 * launch. `x_ptrs`, `numel` are device tables. minmax_out is float[count][2].
 * use_range == 0 disables the masks (integer-like / no valid range).
 * workspace: mi355q_act_minmax_workspace_bytes(count) bytes.
 * ------------------------------------------------------------------------ */
size_t mi355q_act_minmax_workspace_bytes(int32_t count);
int32_t mi355q_act_minmax_f32(const float* const* x_ptrs, const int64_t* numel,
                              int32_t count, float lo, float hi, int32_t use_range,
                              float* minmax_out, void* workspace, size_t workspace_bytes,
                              void* stream);

/* ------------------------------------------------------------------------
 * Activation histograms -- the two per-element passes of DynamicHistogram.
 * ref: utils/histogram_utils.py:139-164 (_DynamicHistogram1D.add), :396-416 (the
 *      isfinite filter of DynamicHistogram.add)
 *
 * Both take `count` float32 tensors as device tables: x_ptrs and the
 * [outer, channels, inner] view of each (channels == 1: one histogram per
 * tensor), plus slot0, the first of the entry's `channels` consecutive slots.
 * `slots` is the number of slots of the whole table, max_numel the element
 * count of the largest entry (it only sizes the grid).
 *
 * mi355q_hist_stats_f32: per slot the minimum and maximum of the finite
 * elements (+inf / -inf when there is none) and their number. NaN and +-inf
 * are left out by a finiteness test.
 *
 * mi355q_hist_bins_f32: per slot with n_bins > 0, every finite element adds one
 * to counts_out[row_offset + clip(int32(floor((x - lower_bound) / bin_width)),
 * 0, n_bins - 1)]; a slot with n_bins == 0 is skipped. counts_out (out_len
 * int64) is added to, not cleared; a row that does not lie inside it, or an
 * n_bins above n_max (the largest n_bins of the table), is skipped.
 *   precision 0: float32 subtraction and division (a float32 state);
 *             1: float32 subtraction, float64 division;
 *             2: both in float64 (the element is widened first).
 * lower_bound / bin_width travel as doubles and are rounded to float32 where
 * the arithmetic is float32. The quotient is the IEEE one (no reciprocal).
 * ------------------------------------------------------------------------ */
size_t mi355q_hist_stats_workspace_bytes(int64_t slots);
int32_t mi355q_hist_stats_f32(const float* const* x_ptrs, const int64_t* outer,
                              const int64_t* channels, const int64_t* inner,
                              const int64_t* slot0, int32_t count, int64_t slots,
                              int64_t max_numel, float* min_out, float* max_out,
                              int64_t* count_out, void* workspace, size_t workspace_bytes,
                              void* stream);
size_t mi355q_hist_bins_workspace_bytes(int64_t slots);
int32_t mi355q_hist_bins_f32(const float* const* x_ptrs, const int64_t* outer,
                             const int64_t* channels, const int64_t* inner,
                             const int64_t* slot0, int32_t count, int64_t slots,
                             int64_t max_numel, const double* lower_bound,
                             const double* bin_width, const int64_t* n_bins,
                             const int64_t* row_offset, int64_t n_max, int32_t precision,
                             int64_t* counts_out, int64_t out_len, void* workspace,
                             size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * K5 -- OCTAV clipping constants, NumPy-order exact.
 * ref: algorithms/uniform_quantize/octav.py:30-112 (_guess_clipping_with_octav)
 *
 * x holds `units` contiguous reduction units of `unit_len` floats (rows for
 * CHANNELWISE on dim 0, blocks for BLOCKWISE_*, the whole tensor for TENSORWISE).
 *   c <- (sum_{x>=c} x - sum_{x<=-c} x) / (n_{|x|>=c} (1-s) + s N),  s = f32(4^-bits / divisor)
 * starting from c = 1 for at most max_iter steps; with early_stop the result is
 * the iterate at which np.allclose(old, new) first holds for ALL units.
 *   count_is_f64 : 1 when the reference reduces over an axis (N is np.int64 and
 *                  s*N is evaluated in float64), 0 for TENSORWISE (axis=None).
 * The float32 sums are accumulated in the order NumPy uses (8192-element chunks,
 * pairwise over runs of selected elements), so clip_out is bit-identical.
 *   clip_out  : float[units];  iters_out: NULL or int32[1] (iterations used)
 *   workspace : mi355q_octav_workspace_bytes(units, max_iter) bytes
 * ------------------------------------------------------------------------ */
size_t mi355q_octav_workspace_bytes(int64_t units, int32_t max_iter);
/* The same plus, for units of 129 .. 16384 elements (the rows kernel's: weight rows), room for the hand-over of a
 * row's late iterations to a one-wave tail kernel (the few per cent of a row a converging guess still
 * selects are listed once and re-tested instead of the row): a caller that passes this much gets
 * that path, one that passes mi355q_octav_workspace_bytes() gets every iteration from the row's own
 * workgroup -- same bits either way. */
size_t mi355q_octav_rows_workspace_bytes(int64_t units, int64_t unit_len, int32_t max_iter);
int32_t mi355q_octav_clip_f32(const float* x, int64_t units, int64_t unit_len, int32_t bits,
                              int32_t max_iter, float exponent_divisor, int32_t early_stop,
                              int32_t count_is_f64, float* clip_out, int32_t* iters_out,
                              void* workspace, size_t workspace_bytes, void* stream);
/* K5, one read (opt-in, tolerance class T2; mi355q.ops.octav_mode("fast") / MI355Q_OCTAV_FAST=1).
 * ref: algorithms/uniform_quantize/octav.py:30-112, the same iteration and the same global early stop as
 * mi355q_octav_clip_f32 with an axis given (count_is_f64 = 1). A unit stays in registers as |x| for all iterations:
 * ONE pass over HBM instead of one per iteration. The masked sums are float32 partials per lane (<= 64 elements), a
 * float32 tree over a wave's lanes and a float64 sum over a unit's waves -- not NumPy's order: clip_out agrees with the
 * reference to ~1e-7 relative (scales within 1e-6, integers +-1 on <= 1e-5 of the elements: SURVEY 7's T2), not bit for
 * bit. unit_len: a multiple of 4 in [4, 65536]; x 16-byte aligned; anything else is UNSUPPORTED (use the exact entry).
 * workspace: mi355q_octav_workspace_bytes(units, max_iter). */
int32_t mi355q_octav_clip_fast_f32(const float* x, int64_t units, int64_t unit_len, int32_t bits,
                                   int32_t max_iter, float exponent_divisor, int32_t early_stop,
                                   float* clip_out, int32_t* iters_out, void* workspace,
                                   size_t workspace_bytes, void* stream);

/* General form: x is viewed as [outer, channels, inner] row-major and channel c's unit is the
 * `outer` segments x[o, c, :] (the reduction NumPy does when a middle or last axis is the
 * quantized dimension: DEPTHWISE_CONV_2D weights, BATCH_MATMUL right-hand sides; ref
 * octav.py:186-199 with common_utils.get_reduce_dims). NumPy keeps one running float32 total
 * per channel and adds each segment's runs to it in order; inner == 1 is a plain left-to-right
 * column sum, outer == 1 is the contiguous form above.
 * workspace: mi355q_octav_workspace_bytes(channels, max_iter). */
int32_t mi355q_octav_clip_nd_f32(const float* x, int64_t outer, int64_t channels, int64_t inner,
                                 int32_t bits, int32_t max_iter, float exponent_divisor,
                                 int32_t early_stop, float* clip_out, int32_t* iters_out,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * a14 -- MSE scale: scale[u] = multiplier * sqrt(mean(x_u^2)), NumPy-order exact.
 * ref: algorithms/uniform_quantize/mse.py:100-109
 * ------------------------------------------------------------------------ */
int32_t mi355q_mse_scale_f32(const float* x, int64_t units, int64_t unit_len, float multiplier,
                             float* scale_out, void* stream);
/* [outer, channels, inner] view, one scale per channel (see mi355q_octav_clip_nd_f32). channels == 1 is ONE contiguous
 * unit of outer * inner elements, as NumPy sums it (it merges the axes: chunks of 8192 run across the segments). */
int32_t mi355q_mse_scale_nd_f32(const float* x, int64_t outer, int64_t channels, int64_t inner,
                                float multiplier, float* scale_out, void* stream);
/* a14 whole: the scale of every contiguous unit AND its integers, q = clip(rint(x / scale[u])) with a zero zero point
 * (ref: mse.py:100-128 -> uniform_quantize_tensor.py:273-362), int8 containers, lo = -2^(bits-1) + (narrow ? 1 : 0).
 * One kernel when a unit's pairwise tree is complete (every length 128 * 2^k, and 8192-multiples of those) and x is
 * 16-byte aligned: the wave that summed a unit quantizes it out of the L2; otherwise mi355q_mse_scale_f32 followed by
 * mi355q_quantize_f32. Same bits either way. */
int32_t mi355q_mse_requant_f32(const float* x, int64_t units, int64_t unit_len, float multiplier, int32_t bits,
                               int32_t narrow, float* scale_out, int8_t* q_out, void* stream);

/* ------------------------------------------------------------------------
 * K6 -- block-diagonal Hadamard rotation: out = reshape(x, (n_vec, h)) @ (H_h / sqrt(h)),
 * H_h the Sylvester matrix, h a power of two <= 16384. In-LDS fast Walsh-Hadamard
 * transform; FP32; out may alias x.
 * ref: algorithms/uniform_quantize/hadamard_rotation.py:48-134
 * ------------------------------------------------------------------------ */
int32_t mi355q_hadamard_rotate_f32(const float* x, int64_t n_vec, int32_t h, float* out,
                                   void* stream);

/* ------------------------------------------------------------------------
 * Dense contraction building blocks (MFMA): C = beta*C + alpha * A.B with
 * A(i,k) at A + i*a_i + k*a_k (element strides; likewise B(k,j), C(i,j)), so
 * transposes and sub-matrices need no copies. float -> v_mfma_f32_32x32x2_f32
 * (exact FP32 fmaf chains, sgemm-class numerics), double -> v_mfma_f64_16x16x4_f64.
 * lower_only writes only j <= i. Used by the GPTQ entry points below; replaces
 * the BLAS calls behind np.matmul / x.T.dot(x) on this path
 * (ref: gptq.py:106, 214; hadamard_rotation.py:129 uses the FWHT instead).
 * ------------------------------------------------------------------------ */
int32_t mi355q_gemm_f32(const float* A, int64_t a_i, int64_t a_k, const float* B, int64_t b_k,
                        int64_t b_j, float* C, int64_t c_i, int64_t c_j, int64_t M, int64_t N,
                        int64_t K, float alpha, float beta, int32_t lower_only, void* stream);
int32_t mi355q_gemm_f64(const double* A, int64_t a_i, int64_t a_k, const double* B, int64_t b_k,
                        int64_t b_j, double* C, int64_t c_i, int64_t c_j, int64_t M, int64_t N,
                        int64_t K, double alpha, double beta, int32_t lower_only, void* stream);

/* The same contraction with every argument of the launcher the GPTQ entry points below use
 * (csrc/gemm.h), so that each of its routes can be driven and checked on its own.
 *   lower_only  0: all of C; 1 or 3: only j <= i is written (1 launches a triangular grid when
 *               M == N, 3 a square grid with early exit); everything above the diagonal is kept.
 *   k_mode      a promise about zeros that lets a tile skip part of K; the skipped range is
 *               never read. With E the tile edge of the kernel that runs (64 or 128) and
 *               i0 / j0 the first row / column of a tile:
 *               0: nothing skipped;
 *               1: A(i,k) == 0 for k > i                            -> k < i0 + E;
 *               2: A(i,k) == 0 for k < i and B(k,j) == 0 for k < j  -> k >= max(i0, j0);
 *               3: B(k,j) == 0 for k < j                            -> k >= j0.
 *   batch > 1   that many problems of this shape in one launch; problem b's operands start
 *               sa / sb / sc elements after those of problem b - 1 (c32: sc floats).
 *   outer > 1   another batch around it (max(batch, 1) * outer problems), steps oa / ob / oc
 *               (oc32 floats for c32). The kernel is chosen from the single problem, so the
 *               results have the bits of separate launches.
 *   c32         not NULL (needs beta == 0): alpha * A.B is stored there as float32
 *               with C's strides and C is left alone (it must still be non-null).
 * splitk_ws / splitk_ws_bytes: optional. With at least mi355q_gemm_splitk_workspace_bytes_*()
 * bytes a long-K product of few tiles is split along K into the workspace and its slices are
 * added in a fixed order (deterministic); with less, or NULL, or batch / outer / c32 / a k_mode
 * other than 0, the product runs unsplit. 0 bytes = this shape is never split. */
typedef struct mi355q_gemm_desc {
  const void* A;
  int64_t a_i, a_k;
  const void* B;
  int64_t b_k, b_j;
  void* C;
  int64_t c_i, c_j;
  int64_t M, N, K;
  double alpha, beta;
  int32_t lower_only, k_mode;
  int32_t batch, outer;
  int64_t sa, sb, sc;
  int64_t oa, ob, oc, oc32;
  float* c32;
} mi355q_gemm_desc;
size_t mi355q_gemm_splitk_workspace_bytes_f32(int64_t M, int64_t N, int64_t K, int32_t lower_only);
size_t mi355q_gemm_splitk_workspace_bytes_f64(int64_t M, int64_t N, int64_t K, int32_t lower_only);
int32_t mi355q_gemm_ex_f32(const mi355q_gemm_desc* desc, void* splitk_ws, size_t splitk_ws_bytes, void* stream);
int32_t mi355q_gemm_ex_f64(const mi355q_gemm_desc* desc, void* splitk_ws, size_t splitk_ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * K8 -- GPTQ Hessian of one calibration tensor: hessian_out (FLOAT64 [d,d]) =
 * alpha * (X^T X), X = float32 [n, d] (tokens x channels), X^T X accumulated in
 * FP32 on the MFMA units, alpha = 2 / num_samples applied in FLOAT64 exactly as
 * `(2.0 / num_samples) * x.T.dot(x)` promotes in the reference.
 * ref: algorithms/uniform_quantize/gptq.py:100-107
 * When d is a multiple of 128 and n >= 1024 the float32 products are formed on the
 * bf16 matrix cores: each float32 is split exactly into three bfloat16 and six
 * exact bf16 products per pair are accumulated in FP32 (what is dropped is below
 * half an ulp of each product; csrc/xtx_bf16x3.hip). MI355Q_XTX_FP32_MFMA=1 in the
 * environment selects the FP32-MFMA product for those shapes too. Either way the
 * result is an FP32-accumulated sgemm whose addition order is the kernel's own
 * (tolerance class T2), symmetric bit for bit, and deterministic run to run.
 * workspace: mi355q_gptq_xtx_workspace_bytes(n, d) bytes (X^T X in FP32, plus the
 * bfloat16 planes of one slab of <= 16384 tokens or the split-K partial sums).
 * ------------------------------------------------------------------------ */
size_t mi355q_gptq_xtx_workspace_bytes(int64_t n, int64_t d);
int32_t mi355q_gptq_xtx_f32(const float* x, int64_t n, int64_t d, double alpha,
                            double* hessian_out, void* workspace, size_t workspace_bytes,
                            void* stream);

/* K8 in two steps, for statistics collected over many calibration samples: the sample-weighted
 * mean of (2 / n_i) X_i^T X_i over samples i (what chaining _gptq_merge_hessian yields, ref
 * utils/qsv_utils.py:71-102) is (2 / N) sum_i X_i^T X_i with N = sum n_i, so the float32 product
 * itself is accumulated -- product (float32 [d, d], lower-triangular part valid) (+)= X^T X, the
 * addition in float32 like the K loop's own -- and scaled into FLOAT64 once at the end:
 * hessian_out = alpha * product, mirrored to both triangles. accumulate == 0 starts a product.
 * workspace: mi355q_gptq_xtx_accum_workspace_bytes(n, d) (the bfloat16 planes of one slab of
 * <= 16384 tokens or the split-K partial sums; no room for the product, which is the caller's). */
size_t mi355q_gptq_xtx_accum_workspace_bytes(int64_t n, int64_t d);
int32_t mi355q_gptq_xtx_accum_f32(const float* x, int64_t n, int64_t d, float* product,
                                  int32_t accumulate, void* workspace, size_t workspace_bytes,
                                  void* stream);
int32_t mi355q_gptq_xtx_finish_f64(const float* product, int64_t d, double alpha,
                                   double* hessian_out, void* stream);

/* Sample-weighted running mean of two Hessians, FLOAT64:
 * h_out = (h_cur*n_cur + h_new*n_new) / (n_cur + n_new); h_out may alias an input.
 * ref: utils/qsv_utils.py:71-88 (_gptq_merge_hessian) */
int32_t mi355q_gptq_hessian_merge_f64(const double* h_cur, double n_cur, const double* h_new,
                                      double n_new, int64_t d, double* h_out, void* stream);

/* ------------------------------------------------------------------------
 * K9 -- damped Hessian inverse: diag zeros -> 1, diag += damp*mean(diag), blocked
 * FP64 Cholesky (MFMA trailing updates), triangular inverse, H^-1 = L^-T L^-1;
 * hinv_out is float32 [d,d] (both triangles). info_out (device int32): 0 on
 * success, j+1 if the leading minor of order j+1 is not positive definite
 * (np.linalg.cholesky would raise LinAlgError).
 * ref: algorithms/uniform_quantize/gptq.py:111-128 (_prepare_hessian_inverse)
 * workspace: mi355q_gptq_hinv_workspace_bytes(d) bytes.
 * ------------------------------------------------------------------------ */
size_t mi355q_gptq_hinv_workspace_bytes(int64_t d);
/* Releases the per-device side stream + events the blocked Cholesky creates on first use for
 * its look-ahead (the only state the library keeps between calls). Safe to call at any time. */
int32_t mi355q_shutdown(void);
/* Creates the current device's look-ahead stream and the eight lanes of the batched inverse NOW instead of on
 * the first inverse that needs them (~35 ms; a hardware queue costs 3 - 4 times as much to create later).
 * The HIP runtime multiplexes streams onto GPU_MAX_HW_QUEUES (default 4) hardware queues, least used
 * first: created after an application's stream pools (PyTorch makes 64 streams at its first
 * torch.cuda.Stream()), the look-ahead stream can land on the caller's own hardware queue, where its
 * trailing updates run IN TURN with the panel chain instead of beside it -- 76 instead of 56 ms for a
 * d = 16384 inverse (tools/hinv_after_c5_probe.py; GPU_MAX_HW_QUEUES=16 has the same effect). The host
 * side calls this before its first kernel on a device. Safe to call any number of times. */
int32_t mi355q_prepare_device(void);
/* hipMalloc / hipFree for a workspace the host side wants to own itself (round 4). A fresh GiB of HBM costs its caller
 * ~30 ms, the workspace of a d = 16384 inverse is 5 GiB, and the framework's caching allocator holds its lock (and the
 * interpreter's) for that long; through these two a helper thread of the host side allocates while the thread that
 * feeds the GPU goes on (mi355q/ops.py: HinvWorkspace). mi355q_device_free(NULL) is a no-op; freeing waits for the
 * device like hipFree. */
/* Measurement aid (bench.py `clock_while_timed`): one wave counts shader clocks (clock64) over `seconds` of the constant
 * 100 MHz counter (wall_clock64) and writes {clocks, ticks} to the device int64[2] -- clocks / ticks * 100 = MHz sustained
 * while whatever else is running runs. Launch it on a stream of its own beside the kernel under test. */
int32_t mi355q_clock_probe(double seconds, int64_t* clocks_and_ticks_out, void* stream);
int32_t mi355q_device_alloc(size_t nbytes, void** out);
int32_t mi355q_device_free(void* p);
int32_t mi355q_gptq_hinv_f64(const double* hessian, int64_t d, double damp_factor, float* hinv_out,
                             int32_t* info_out, void* workspace, size_t workspace_bytes,
                             void* stream);

/* The same inverse of hessian = alpha * product, taken straight from the float32 product X^T X that
 * mi355q_gptq_xtx_accum_f32 collected (lower triangle valid): alpha * double(product) is formed where
 * the damped copy reads it, so the 2 GiB float64 Hessian of a d = 16384 layer is never materialized
 * (mi355q_gptq_xtx_finish_f64 makes it only when a caller reads the statistic). Bit-identical to
 * mi355q_gptq_hinv_f64 on the finished Hessian. Same workspace. */
int32_t mi355q_gptq_hinv_from_product_f32(const float* product, int64_t d, double alpha, double damp_factor,
                                          float* hinv_out, int32_t* info_out, void* workspace,
                                          size_t workspace_bytes, void* stream);

/* `count` independent inverses of equally sized Hessians in one call (a model has one per distinct
 * FULLY_CONNECTED input: 54 of order 2048 and 18 of order 16384 in a Gemma-2B; ref gptq.py:111-128 is
 * called once per weight, the calls share nothing). d < 4096, where one inverse is a chain of small
 * dependent kernels that leaves the chip idle: the matrices advance through every step together.
 * d >= 4096: one after the other on the caller's stream (a lone large inverse keeps the machine busy with its
 * own look-ahead update; MI355Q_HINV_PAIRS=1 keeps two in flight, each with a look-ahead stream of its own --
 * measured slower, profiles/r05_hinv_pairs.txt). Every matrix sees the launches of a single call in the
 * same order: results are bit-identical to `count` calls of mi355q_gptq_hinv_f64. The two pointer tables
 * are HOST arrays of device pointers; info_out is device int32[count].
 * workspace: mi355q_gptq_hinv_batched_workspace_bytes(count, d). */
size_t mi355q_gptq_hinv_batched_workspace_bytes(int32_t count, int64_t d);
int32_t mi355q_gptq_hinv_f64_batched(const double* const* hessians_host, int32_t count, int64_t d,
                                     double damp_factor, float* const* hinv_out_host, int32_t* info_out,
                                     void* workspace, size_t workspace_bytes, void* stream);

/* The same for Hessians handed over as hessian[i] = alphas_host[i] * products_host[i] (float32 X^T X, lower
 * triangle valid: see mi355q_gptq_hinv_from_product_f32) -- what calibration leaves behind for the large
 * layers. alphas_host is a HOST array of count doubles. Bit-identical to `count` single calls.
 * workspace: mi355q_gptq_hinv_from_product_batched_workspace_bytes(count, d). */
size_t mi355q_gptq_hinv_from_product_batched_workspace_bytes(int32_t count, int64_t d);
int32_t mi355q_gptq_hinv_from_product_f32_batched(const float* const* products_host, const double* alphas_host,
                                                  int32_t count, int64_t d, double damp_factor,
                                                  float* const* hinv_out_host, int32_t* info_out, void* workspace,
                                                  size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * K10 -- GPTQ weight update + quantization: for each 64-column block, quantize
 * column by column with the up-front scales, propagate err/Hinv[c,c] to the rest
 * of the block (rank-1, FP32, product rounded before the subtraction as NumPy's
 * np.outer does) and then to all later columns with MFMA GEMMs (lazy batch
 * updates: the later blocks of a group of four catch up inside their own
 * kernel, the columns beyond the group get one K = 256 product per group; for
 * rows and d multiples of 128 with d >= 4096 or rows >= 8192 that product runs on
 * the bf16 matrix cores on the exact three-way split of its float32 operands,
 * csrc/xtx_bf16x3.hip -- MI355Q_UPD_FP32_MFMA=1 keeps the FP32 MFMA product).
 * ref: algorithms/uniform_quantize/gptq.py:131-216 (_apply_gptq, blocksize 64)
 *   w [rows, d] float32 (not modified); hinv float32 [d, d]
 *   scale_mode 0: scale[1] (TENSORWISE); 1: scale[rows] (CHANNELWISE);
 *              2: scale[rows, d/block_size] (BLOCKWISE)
 *   scale_is_f64 / zp_via_f64 / diff_bits: NumPy promotion switches, see
 *              mi355q_quantize_f32 / mi355q_dequantize_f32
 *   q_out int8 [rows, d]; workspace: mi355q_gptq_apply_workspace_bytes(rows, d)
 * ------------------------------------------------------------------------ */
size_t mi355q_gptq_apply_workspace_bytes(int64_t rows, int64_t d);
int32_t mi355q_gptq_apply_f32(const float* w, int64_t rows, int64_t d, const float* hinv,
                              const void* scale, int32_t scale_is_f64, const int32_t* zero_point,
                              int32_t scale_mode, int32_t block_size, int32_t bits, int32_t narrow,
                              int32_t zp_via_f64, int32_t diff_bits, int8_t* q_out, void* workspace,
                              size_t workspace_bytes, void* stream);
/* The same sweep for targets of 9..32 bits (ref gptq.py:141-151: `_get_quantized_dtype` gives int16 / int32 containers;
 * the reference's policy admits 2-, 4- and 8-bit weights only, so only a direct caller of get_tensor_quant_params gets
 * here): q_out int32 [rows, d] -- for 9..16 bits the host narrows to the int16 the reference returns --, the general
 * 64-column block kernel (one launch per block: the symmetric fast path packs bytes), the far update per block as for
 * 8 bits; diff_bits 16 wraps q - zp like int16 - int16. From 17 bits on the container is int32 and the reference's
 * float32 arithmetic is kept as it is: clip bounds are the float32 nearest to the integer bounds (2^(bits-1) from 26 bits
 * on), a quotient of 2^31 or a NaN casts to INT32_MIN (x86), q - zp wraps in int32, (q - zp) * scale is a float64
 * product rounded once with the subtraction (NumPy: int32 x float32). Same workspace. */
int32_t mi355q_gptq_apply_wide_f32(const float* w, int64_t rows, int64_t d, const float* hinv,
                                   const void* scale, int32_t scale_is_f64, const int32_t* zero_point,
                                   int32_t scale_mode, int32_t block_size, int32_t bits, int32_t narrow,
                                   int32_t zp_via_f64, int32_t diff_bits, int32_t* q_out, void* workspace,
                                   size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * f4 -- OSCAR (activation-aware channel scaling + optimal clipping), FULLY_CONNECTED weights
 * w float32 [n, d] (n output channels, d input channels). All arithmetic FP64 as in the
 * reference; summation orders are NumPy's. The O(d) vector algebra between these calls
 * (geometric-mean normalisation, clamps) is host NumPy, as in the reference.
 * ref: algorithms/uniform_quantize/oscar.py
 * ------------------------------------------------------------------------ */
/* out[j] = sum_r x[r, j]^2 (rows added in order), divided by rows when mean != 0. A single column (d == 1) is a
 * contiguous vector to NumPy, which adds it as np.sum does: 8192-element chunks in order, each pairwise.
 *   mean=1: calibration statistic mu2 = np.mean(x*x, axis=0)            (ref oscar.py:318-324)
 *   mean=0: column energies (w*w).sum(0)                                 (ref oscar.py:224) */
int32_t mi355q_oscar_col_sumsq_f32(const float* x, int64_t rows, int64_t d, int32_t mean,
                                   double* out, void* stream);
/* Per (row, group of g consecutive columns; g == d or g in {32,64,128,256}):
 *   top = max_j |w[r,j]| * s[j], winner = first argmax, wsq = w[r, winner]^2;
 *   sums_out[k] = np.sum over rows of top^2 for group k (8192-chunk pairwise order).
 * The objective of ref oscar.py:175-194 is sum_k sums_out[k] * mass_k (host); winner / wsq
 * feed mi355q_oscar_winner_energy_f64 (ref oscar.py:236-246).
 *   top2_workspace double [d/g * n]; winner_out int32 [d/g, n]; wsq_out double [d/g, n]
 * The blockwise route (g != d) reads w as float4 and s as double2: w and s must be 16-byte aligned, and d is a
 * multiple of g, hence of 4, so that every row of w starts on such a boundary. */
int32_t mi355q_oscar_group_terms_f32(const float* w, const double* s, int64_t n, int64_t d,
                                     int32_t g, double* top2_workspace, int32_t* winner_out,
                                     double* wsq_out, double* sums_out, void* stream);
/* eff_out[j] = sum over rows in order of wsq[j/g, r] where winner[j/g, r] == j
 * (np.add.at(a_eff, j_star, w[rows, j_star]**2), ref oscar.py:243-246). */
int32_t mi355q_oscar_winner_energy_f64(const int32_t* winner, const double* wsq, int64_t n,
                                       int64_t d, int32_t g, double* eff_out, void* stream);
/* Optimal clip bound of every segment of g consecutive elements of the flattened [n, d]
 * matrix (g divides d, or g == n*d for TENSORWISE): stable descending sort of |w|*s carrying
 * the masses m[j], sequential running sums, closed-form candidate per breakpoint interval,
 * first minimum (ref oscar.py:62-108). u[k], noise[k] per column group k (host FP64); the product passes
 * u[k] = M_k/(6 qmax^2), noise[k] = M_k/(12 qmax^2) with M_k the group's total mass + 1e-12, but any
 * values are accepted and used as given.
 * scale_out (optional) is tensor_zp_scale_from_min_max(-bound, bound) of the symmetric signed
 * target: max(bound, 1e-9) / qmax, and with blockwise_scale != 0 rounded FP64 -> float32 ->
 * bfloat16 -> float16 (ref uniform_quantize_tensor.py:553-581), stored as double.
 *   bounds_out / scale_out double [n*d/g], either may be NULL;
 *   workspace: mi355q_oscar_clip_workspace_bytes(n, d, g) (two (key, mass) slabs for the sort's merge passes + one byte per
 *   segment + the masses' total).
 * CHANNELWISE rows (g == d, 384 <= g <= 16384, qmax >= 7) are answered from a sorted prefix of their largest magnitudes
 * where a convexity argument with an explicit rounding bound shows that no later breakpoint can hold the first minimum;
 * rows where it cannot take the full sort + scan. Same bits either way, for any u / noise: the bound takes the total
 * mass from m itself, and rows with noise < 0 or a negative mass take the full route (csrc/oscar.hip: clip_prefix_kernel).
 * Environment: MI355Q_OSCAR_PREFIX=0 full sort + scan for every row; MI355Q_OSCAR_PREFIX_TARGET=<n> elements asked for. */
int32_t mi355q_oscar_clip_workspace_bytes(int64_t n, int64_t d, int64_t g, size_t* bytes_out);
int32_t mi355q_oscar_clip_bounds_f32(const float* w, const double* s, const double* m, int64_t n,
                                     int64_t d, int64_t g, const double* u, const double* noise,
                                     int32_t qmax, int32_t blockwise_scale, double* bounds_out,
                                     double* scale_out, void* workspace, size_t workspace_bytes,
                                     void* stream);
/* out = clip(rint((w * s[j]) / scale[segment]), qlo, qhi) with FP64 product and quotient
 * (uniform_quantize of the FP64 scaled weight, ref oscar.py:470-478). scale double [n*d/g]. */
int32_t mi355q_oscar_quantize_f32(const float* w, const double* s, const double* scale, int64_t n,
                                  int64_t d, int64_t g, int32_t qlo, int32_t qhi, int8_t* out,
                                  void* stream);

/* ------------------------------------------------------------------------
 * dequantized_weight_recovery -- scales of fake-quantized (QAT) weights and the recovery check.
 * ref: algorithms/uniform_quantize/dequantized_weight_recovery.py:48-61, 118-186, 30-45
 * ------------------------------------------------------------------------ */
/* scale_out[k] = smallest positive step between the sorted magnitudes (0 appended) of segment k
 * of g consecutive elements of w [n, d] (g divides d, or g == n*d), floored at 1e-9.
 *   rounded != 0: float32 arithmetic of the channel- / blockwise path (steps rounded to float32,
 *   only steps > float32(1e-9) count, floor float32(1e-9)); rounded == 0: the TENSORWISE path's
 *   float64. workspace: mi355q_oscar_clip_workspace_bytes(n, d, g). */
int32_t mi355q_dwr_scales_f32(const float* w, int64_t n, int64_t d, int64_t g, int32_t rounded,
                              double* scale_out, void* workspace, size_t workspace_bytes,
                              void* stream);
/* *max_out = max |q * scale[e / g] - w| in FP64 (NaN if any), the quantity
 * _validate_recovered_weights compares with its tolerance. */
int32_t mi355q_dwr_max_error_f32(const float* w, const int8_t* q, const double* scale, int64_t total,
                                 int64_t g, double* max_out, void* stream);

/* ------------------------------------------------------------------------
 * Multi-GPU exchange steps: one process per GPU, RCCL over xGMI. The
 * reference is single-process; these define what the sharded calibration adds and must
 * reproduce. `comm` is an opaque RCCL communicator (ncclComm_t) owned by the caller:
 *   rank 0: mi355q_comm_unique_id(id)  ->  the host broadcasts the 128 bytes over its own
 *   rendezvous  ->  every rank: mi355q_comm_init_rank(&comm, nranks, id, rank) with its GPU
 *   current. Collectives enqueue on `stream` and return; all ranks must call them in the same
 *   order. RCCL is bound at run time (the librccl.so.1 already in the process under
 *   PyTorch-ROCm); without it these calls -- and only these -- return MI355Q_RCCL_ERROR.
 * ------------------------------------------------------------------------ */
#define MI355Q_UNIQUE_ID_BYTES 128
int32_t mi355q_comm_unique_id(char* id_host /* [MI355Q_UNIQUE_ID_BYTES] */);
int32_t mi355q_comm_init_rank(void** comm_out_host, int32_t nranks, const char* id_host, int32_t rank);
int32_t mi355q_comm_info(void* comm, int32_t* nranks_host, int32_t* rank_host);
int32_t mi355q_comm_destroy(void* comm);
/* X1 -- per-sample activation statistics of every rank to every rank: out[r*n .. r*n+n) =
 * rank r's local[0..n) (float (min, max) pairs, n floats per rank, equal on all ranks: shards
 * are padded to the longest). The host then replays the order-dependent moving average
 * (ref: utils/qsv_utils.py:43-68, calibrator.py:395-421) over all samples in dataset order. */
int32_t mi355q_allgather_minmax(void* comm, const float* local, int64_t n, float* out, void* stream);
/* X1 fast path -- global ranges when the update rule is min_max_update (ref:
 * utils/qsv_utils.py:105-122; associative and commutative): in-place all-reduce(min) of mins[n]
 * and all-reduce(max) of maxs[n], issued as one RCCL group. */
int32_t mi355q_allreduce_minmax_f32(void* comm, float* mins, float* maxs, int64_t n, void* stream);
/* In-place all-reduce(sum) building blocks (OSCAR's sample-weighted second moments, counts). */
int32_t mi355q_allreduce_sum_f32(void* comm, float* buf, int64_t n, void* stream);
int32_t mi355q_allreduce_sum_f64(void* comm, double* buf, int64_t n, void* stream);
/* X2 -- GPTQ Hessian over sample-sharded calibration: hessian (FLOAT64 [d, d], this rank's
 * sample-weighted mean over its own samples, as chaining mi355q_gptq_hessian_merge_f64 yields) is
 * scaled by weight = n_rank / N and all-reduced(sum) in place; every rank ends with the mean over
 * all N samples, which is what chaining _gptq_merge_hessian over the whole dataset yields up to
 * FP64 rounding (ref: utils/qsv_utils.py:71-102). One collective of d*d*8 bytes per distinct
 * Hessian: 32 MiB at d = 2048, 2 GiB at d = 16384. A rank without samples passes zeros, weight 0. */
int32_t mi355q_allreduce_hessian_f64(void* comm, double* hessian, int64_t d, double weight, void* stream);
/* X2 at half the bytes, and to the one rank that needs it: the Hessian is symmetric, so only its
 * packed lower triangle (d (d + 1) / 2 doubles: 1 GiB at d = 16384) travels -- packed = weight *
 * lower(hessian) in `workspace`, one all-reduce(sum) (root < 0: every rank ends with the mean) or one
 * reduce(sum) to `root` (under GPTQ exactly one rank reads a given Hessian: the owner of the ops
 * whose input it belongs to; a ring reduce moves half of what a ring all-reduce does), then the
 * receiving ranks unpack to both triangles in place. On the other ranks `hessian` is left as it was.
 * The sum is the same FP64 sum of the same weighted entries as in mi355q_allreduce_hessian_f64.
 * workspace: mi355q_hessian_exchange_workspace_bytes(d) bytes. */
size_t mi355q_hessian_exchange_workspace_bytes(int64_t d);
int32_t mi355q_reduce_hessian_f64(void* comm, double* hessian, int64_t d, double weight, int32_t root,
                                  void* workspace, size_t workspace_bytes, void* stream);
/* X2 in the form the statistic is kept in: the mean of ref utils/qsv_utils.py:71-102 over all samples is
 * (2 / N) * sum over ranks of P_rank, P_rank = sum of X^T X over the rank's own samples -- the FLOAT32
 * product mi355q_gptq_xtx_accum_f32 accumulates (lower triangle valid). Only that triangle travels, as
 * float32: d (d + 1) / 2 * 4 bytes, 0.5 GiB at d = 16384 (a quarter of the float64 all-reduce, half of the
 * packed float64 reduce), summed across ranks in float32 -- the precision in which a single process adds
 * its own slabs' products -- by one reduce(sum) to `root` (root < 0: all-reduce). The receiving ranks end
 * with the sum in `product`'s lower triangle and keep the statistic in product form
 * (mi355q_gptq_hinv_from_product_f32 with alpha = 2 / N reads it as it is); no float64 d x d array is
 * made on any rank. product == NULL: this rank saw no sample (it contributes zeros and must not be `root`).
 * workspace: mi355q_product_exchange_workspace_bytes(d) bytes. */
size_t mi355q_product_exchange_workspace_bytes(int64_t d);
int32_t mi355q_reduce_product_f32(void* comm, float* product, int64_t d, int32_t root, void* workspace,
                                  size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Model file <-> HBM without a host copy of the weights (the file path's io ring).
 *   ref: utils/tfl_flatbuffer_utils.py:142-163  the model file is mapped / read whole into host memory;
 *        model_modifier.py:290-391              the serializers copy every quantized buffer into one host
 *                                               bytearray and write it out
 * mi355q_file_to_device: bytes [file_offset, file_offset + nbytes) of the open file `fd` -> `dst` (device):
 * pread() on the library's io threads into a ring of three pinned 8 MiB slots (made on first use, per
 * device), hipMemcpyAsync on `copy_stream` (the caller orders its compute stream behind it). Returns when the
 * last copy is ENQUEUED and every read is done. mi355q_device_to_file: `src` (device; the caller has ordered
 * `copy_stream` behind its producer) -> the file at file_offset: asynchronous copies into the ring, pwrite()
 * from there on the io threads; returns with the last writes possibly in flight -- mi355q_file_io_finish()
 * waits for them and reports the first write error. A short read (end of file) or a failing pread / pwrite is
 * MI355Q_IO_ERROR. One transfer enqueues at a time per process; mi355q_shutdown() releases ring and threads. */
int32_t mi355q_file_to_device(int32_t fd, int64_t file_offset, int64_t nbytes, void* dst, void* copy_stream);
int32_t mi355q_device_to_file(const void* src, int64_t nbytes, int32_t fd, int64_t file_offset, void* copy_stream);
int32_t mi355q_file_io_finish(void);

/* The same transfers without holding the caller (round 4). mi355q_file_to_device returns when the file has been READ --
 * a model's weights cross at the ring's rate while the calling thread, the one that walks the ops and launches the
 * kernels, stands still (0.62 s of a 3.6 s Gemma-2B GPTQ run; 30 of the 60 ms of a 1.4 GB file -> file run).
 *   mi355q_file_io_submit_upload    queues the transfer on the library's upload thread (first in, first out) and
 *                                   returns a ticket at once; `dst` and `fd` stay valid until the ticket is waited for.
 *   mi355q_file_io_wait             blocks until the ticket's last copy is ENQUEUED on its copy stream (an event the
 *                                   caller records on that stream afterwards lies behind all of them), frees the
 *                                   ticket and returns the transfer's status (a short or failing read is
 *                                   MI355Q_IO_ERROR here; nothing of a spoiled slot was copied).
 *   mi355q_file_io_submit_download  queues `src` -> file on the download thread (its own ring: uploads and
 *                                   downloads run at the same time). `ready_event`, when not null, is a hipEvent_t
 *                                   the caller has RECORDED behind the payload's producer: the download thread waits for it
 *                                   (hipEventSynchronize) before it enqueues the first copy -- for that producer, not
 *                                   for everything queued on the compute stream. No ticket:
 *                                   mi355q_file_io_finish waits for every submitted transfer of both directions
 *                                   and the writes behind them, and reports the first failure.
 * ref: the same two call sites (utils/tfl_flatbuffer_utils.py:142-163, model_modifier.py:290-391). */
int32_t mi355q_file_io_submit_upload(int32_t fd, int64_t file_offset, int64_t nbytes, void* dst, void* copy_stream,
                                     int64_t* ticket);
int32_t mi355q_file_io_wait(int64_t ticket);
int32_t mi355q_file_io_submit_download(const void* src, int64_t nbytes, int32_t fd, int64_t file_offset,
                                       void* copy_stream, void* ready_event);
/* The same download with memory as its destination (round 5): `dst` is the payload's place inside the OUTPUT FILE'S OWN
 * shared mapping, whose pages exist already (the host allocates them ahead of time, LiteRTLMFile.prepare_output). The io
 * threads then copy each staged piece into the mapping instead of pwrite()ing it: buffered writes of several threads to
 * one file take turns on its inode lock (11 GB/s into allocated pages with 4 threads, 7 into fresh ones), copies into
 * mapped pages do not (22 - 30 GB/s with 4 - 8 threads; tools/tmpfs_write_probe.py). Same queue, gate and completion
 * (mi355q_file_io_finish) as mi355q_file_io_submit_download; `dst` .. `dst + nbytes` must stay mapped until then.
 * ref: model_modifier.py:290-391 (the reference copies every quantized buffer into one host bytearray). */
int32_t mi355q_file_io_submit_download_mapped(const void* src, int64_t nbytes, void* dst, void* copy_stream,
                                              void* ready_event);

/* ------------------------------------------------------------------------
 * Tensor comparison for model validation: the five metrics of the reference's
 * validation_utils for one float32 REFERENCE operand against a TARGET read in
 * its stored form (dequantized in registers, never written back as float32).
 * ref: utils/validation_utils.py:63-255, model_validator.py:357-361
 *
 * Both operands go through np.nan_to_num(nan=1e-9, neginf=-1e9, posinf=1e9).
 * Integer targets are viewed as [outer, channels, inner]: element e uses
 * scale[c] / zero_point[c] with c = (e / inner) % channels (channels = 1:
 * per tensor; blockwise along the last axis: channels = n / block, inner =
 * block). (q - zp) is formed in a `diff_bits`-wide integer and wraps, as NumPy
 * does in the promoted type of (q, zero_point); diff_bits 32 multiplies in
 * float64 and casts to float32, 8 / 16 multiply in float32
 * (ref: uniform_quantize_tensor.py:365-409). I4 / I2 are packed as pack_bits
 * writes them, element 0 in the low bits.
 *
 * Per pair the result carries
 *   sum_sq_diff  Sum (t - r)^2        float32, NumPy's order for np.sum of a
 *   sum_ref_sq   Sum r^2              contiguous 1-D array (8192-element
 *   sum_kl       Sum p log((p+e)/(q+e)), p = max(0, r), q = max(0, t), e = 1e-9
 *                                     chunks, pairwise inside, added in order)
 *   median_lo/hi the lower / upper middle value of |t - r| / (|r| + 1e-6)
 *                (equal for odd n); only with MI355Q_COMPARE_MEDIAN
 *   dot_tr/tt/rr float32 products summed in float64 (cosine similarity).
 * The means and ratios are formed on the host. n = 0 enqueues nothing.
 * workspace: mi355q_compare_workspace_bytes(count, total_chunks), where
 * total_chunks = Sum mi355q_compare_chunks(n_i) (count = 1 for the single form).
 * ------------------------------------------------------------------------ */
enum {
  MI355Q_CMP_F32 = 0,
  MI355Q_CMP_F16 = 1,
  MI355Q_CMP_BF16 = 2,
  MI355Q_CMP_I8 = 3,
  MI355Q_CMP_I16 = 4,
  MI355Q_CMP_I32 = 5,
  MI355Q_CMP_I4 = 6,
  MI355Q_CMP_I2 = 7
};
#define MI355Q_COMPARE_MEDIAN 1   /* median_lo / median_hi (three more passes over the operands) */
#define MI355Q_COMPARE_NO_KL 2    /* skip sum_kl (left 0): no logf per element */

typedef struct mi355q_compare_pair {
  const float* reference;      /* n float32 */
  const void* target;          /* n elements of target_kind (packed for I4 / I2) */
  int64_t n;
  int32_t target_kind;         /* MI355Q_CMP_* */
  int32_t diff_bits;           /* integer kinds: 8, 16 or 32 */
  int64_t channels, inner;     /* integer kinds: the scale view */
  const float* scale;          /* integer kinds: `channels` entries */
  const int32_t* zero_point;   /* integer kinds: `channels` entries, or NULL (all zero) */
} mi355q_compare_pair;         /* 64 bytes */

typedef struct mi355q_compare_result {
  float sum_sq_diff, sum_ref_sq, sum_kl;
  float median_lo, median_hi, reserved;
  double dot_tr, dot_tt, dot_rr;
} mi355q_compare_result;       /* 48 bytes */

int64_t mi355q_compare_chunks(int64_t n);
size_t mi355q_compare_workspace_bytes(int32_t count, int64_t total_chunks);
int32_t mi355q_compare_f32(const float* reference, const void* target, int64_t n, int32_t target_kind,
                           int32_t diff_bits, int64_t channels, int64_t inner, const float* scale,
                           const int32_t* zero_point, int32_t flags, mi355q_compare_result* result,
                           void* workspace, size_t workspace_bytes, void* stream);
/* `count` pairs in one set of launches; `pairs` is a DEVICE table, so its entries are checked on the device: when
 * an entry is invalid (as mi355q_compare_f32 would refuse it) or total_chunks is not Sum mi355q_compare_chunks(n_i),
 * no operand is read and every float field of every result of the call is NaN. An entry with n = 0 is valid whatever its
 * other fields hold: nothing of it is read, it takes no chunk, and its result is all zeros (a table of only such
 * entries has total_chunks = 0). */
int32_t mi355q_compare_f32_batched(const mi355q_compare_pair* pairs, int32_t count, int64_t total_chunks,
                                   int32_t flags, mi355q_compare_result* results, void* workspace,
                                   size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Layer output error of a quantized FULLY_CONNECTED weight (csrc/layer_error.hip)
 *
 * With H = (2/n) X^T X, the statistic GPTQ calibration keeps per FULLY_CONNECTED
 * input, and dW = W - dequant(W^):
 *   (1/n) ||X dW^T||_F^2 = 1/2 tr(dW H dW^T) = 1/2 Sum_r d_r H d_r^T
 * so the layer's output error over the calibration set is one quadratic form per
 * output channel against a matrix that is already resident.
 *
 * mi355q_weight_delta_f32: delta_out[e] = reference[e] - dequant(target)[e] in
 * float32. The target is described exactly as for mi355q_compare_f32 (MI355Q_CMP_*
 * kinds, [outer, channels, inner] scale view, the diff_bits rule, I4 / I2 packed
 * low bits first) and dequantized in registers by the same rule. There is no
 * nan_to_num here: values pass through as they are. n = 0 enqueues nothing.
 *
 * mi355q_quadform_rows_f32: out_rows[r] = alpha * a_r Psym a_r^T in FLOAT64 for
 * a = float32 [rows, d] row-major and Psym the symmetric matrix whose LOWER
 * triangle (j <= i) is product[i*d + j] -- the float32 product form of a Hessian
 * accumulator. Nothing above the diagonal is ever read and nothing of `product`
 * is written. FP32 MFMA tiles C = a L' over (128 rows x 128 columns j0), where
 * L'[k][j] = 2 P[k][j] for k > j, P[j][j] for k = j and 0 for k < j: the K loop
 * runs over k >= j0 only, the doubling is exact, and no 2*lower - diagonal
 * subtraction exists. The epilogue multiplies C by the `a` tile, sums every row's
 * 64 columns in float64 into partials[ceil(d / 64)][rows], and a second kernel
 * adds a row's partials in index order: the result has the same bits in every
 * run (no floating-point atomics) and there is no rows x d intermediate.
 * |out_r - exact_r| <= (2d + 3) 2^-24 alpha Sum_ij |a_ri| |P_ij| |a_rj| to first
 * order. Non-finite inputs give non-finite rows; rows = 0 enqueues nothing.
 * workspace: mi355q_quadform_rows_workspace_bytes(rows, d) =
 * rows * ceil(d / 64) * 8 rounded up to 256 bytes.
 *
 * mi355q_weight_delta_transformed_f32 (csrc/hadamard.hip): the delta of a weight
 * whose quantized op reads a TRANSFORMED activation. Both transformations the
 * recipes insert are linear maps on the reduction dimension, so the error is the
 * same quadratic form against the Hessian of the untransformed input with
 *   multiply   y = (x * m) W^'T:   dW = W - dequant(W^) * m   (m: d floats, column e % d)
 *   Hadamard   y = (x R) W^'T:     dW = W - rotate_h(dequant(W^)),  R = blockdiag(H_h / sqrt(h))
 * The target is described as for mi355q_weight_delta_f32; d is the row length
 * (n % d == 0). `multiplier` may be NULL; hadamard_size 0 or 1 means no rotation,
 * otherwise it is a power of two <= 16384 that divides d. With neither, the
 * result is mi355q_weight_delta_f32's bit for bit; both at once is
 * MI355Q_UNSUPPORTED. Multiply: delta_out[e] = reference[e] - fl(dq[e] * m[e % d]),
 * the float32 product rounded once, then a float32 subtraction. Hadamard: rotate_h
 * is the float32 butterfly network of mi355q_hadamard_rotate_f32 for aligned
 * operands (r = 1 / sqrtf(h) on load; the radix-2 LDS kernel for h < 256, the
 * radix-16 tiles of 4096 / 8192 / 16384 elements above) instantiated with the
 * dequantizing load and `reference[e] - v` as its store, so the result equals
 * dequantize -> mi355q_hadamard_rotate_f32 -> subtract bit for bit without the
 * two n-element temporaries. The network is chosen from h alone: misaligned
 * reference / delta_out only make the accesses scalar. delta_out must not alias
 * the inputs. n = 0 enqueues nothing.
 * ------------------------------------------------------------------------ */
int32_t mi355q_weight_delta_f32(const float* reference, const void* target, int64_t n, int32_t target_kind,
                                int32_t diff_bits, int64_t channels, int64_t inner, const float* scale,
                                const int32_t* zero_point, float* delta_out, void* stream);
int32_t mi355q_weight_delta_transformed_f32(
    const float* reference, const void* target, int64_t n, int32_t target_kind, int32_t diff_bits,
    int64_t channels, int64_t inner, const float* scale, const int32_t* zero_point,
    int64_t d, const float* multiplier, int32_t hadamard_size, float* delta_out, void* stream);
size_t mi355q_quadform_rows_workspace_bytes(int64_t rows, int64_t d);
int32_t mi355q_quadform_rows_f32(const float* a, int64_t rows, int64_t d, const float* product, double alpha,
                                 double* out_rows, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Sensitivity sweep (csrc/sensitivity.hip): the weight deltas of up to 8 candidate
 * configurations from ONE read of the weight.
 *
 * Candidate k is the symmetric min/max fake-quantization of x [rows, cols]
 * (float32, row-major) with bits[k] in {2, 4, 8} and block[k] in {0, 32, 64, 128,
 * 256}: block 0 is one scale per row, block > 0 one scale per block along cols,
 * rounded f32 -> bf16 -> f16 -> f32 as the blockwise scales of
 * mi355q_requant_sym_f32 are. `bits` and `block` are HOST arrays of `count`
 * entries (1 <= count <= 8); they travel in the kernel arguments, as the pointer
 * tables of mi355q_requant_sym_f32_batched_hostptrs do.
 *   delta_out[k * delta_stride + e] = x[e] - fl(float(q_k[e]) * s_k)
 * where q_k and s_k are bit for bit what mi355q_requant_sym_f32(x, rows, cols,
 * block[k], bits[k], clip = NULL, ...) writes to q_out / scale_out: the result
 * equals that call followed by mi355q_weight_delta_f32 (MI355Q_CMP_I8, diff_bits
 * 8) bit for bit. The product is rounded to float32 once and subtracted in
 * float32 (no FMA). There is no nan_to_num: NaN / inf data and NaN scales pass
 * through as in that composition. No integers and no scales are stored.
 * delta_stride (in floats) >= rows * cols.
 *
 * sq_rows_out: NULL, or double[count][rows] with sq[k][r] = Sum_c double(delta)^2
 * of row r in FLOAT64, added in a fixed order (a lane's pieces in ascending
 * order, a wave butterfly, the waves' partials in index order; no floating-point
 * atomics): the same bits in every run.
 *
 * Vector route (cols % 4 == 0, cols <= 16384, x and delta_out 16-byte aligned,
 * delta_stride % 4 == 0 when count > 1): a row is held in registers as 16-byte
 * pieces by one wave (cols <= 1024) or one 256-thread workgroup, x is read from
 * HBM once for all candidates, the |x|-max butterfly runs once (the maxima of 8 /
 * 16 / 32 / 64 adjacent lanes are the block-32 / 64 / 128 / 256 maxima, the wave's
 * or workgroup's the row's), and every delta piece leaves as one non-temporal
 * 16-byte store: 4 + 4 count bytes per element against 14 count for requant_sym
 * -> weight_delta. Every other shape (cols % 4 != 0, misaligned pointers,
 * cols > 16384) takes a scalar kernel with the same bits, which passes over x once
 * for the row maximum and once per candidate: the one-read property holds for the
 * vector route only.
 *
 * Refused before any launch with MI355Q_BAD_ARG: count outside [1, 8], null
 * tables, bits or block outside the sets above, a block that does not divide
 * cols ("Quantized dimension <cols> is not divisible by block size <block>."),
 * negative shapes; then rows == 0 or cols == 0 enqueues nothing; then null x /
 * delta_out or delta_stride < rows * cols are MI355Q_BAD_ARG, rows > 2^31 - 1
 * MI355Q_UNSUPPORTED. delta_out must not alias x.
 * ------------------------------------------------------------------------ */
int32_t mi355q_requant_delta_sweep_f32(const float* x, int64_t rows, int64_t cols, int32_t count,
                                       const int32_t* bits, const int32_t* block, float* delta_out,
                                       int64_t delta_stride, double* sq_rows_out, void* stream);

/* ---------------------------------------------------------------------------
 * Integer execution of a quantized FULLY_CONNECTED op (csrc/qfc.hip): what the
 * op computes in integers on the calibration samples, up to the int32
 * accumulator and its float rescale. Bias, fused activation and the
 * requantization of the op's output are outside: the result is the pre-bias
 * product, the boundary the layer output error draws.
 *
 * mi355q_qfc_quantize_rows_f32: the dynamic-range activation quantizer. x is
 * float32 [n, d] row-major. Per row t: range = max_k |x[t,k]|;
 *   range == 0            scale_out[t] = 1.0f, q = 0
 *   a NaN or an infinity  scale_out[t] = NaN,  q = 0
 *   otherwise             scale_out[t] = range / 127.0f, inv = 127.0f / range
 *                         (IEEE float32 divides),
 *                         q = clamp(round_half_away_from_zero(fl(x * inv)), -127, 127)
 * The product is rounded to float32 once and the rounding of it is exact
 * (trunc + the exact remainder, never "add 0.5"): 0.49999997f gives 0. Vector
 * route (d % 16 == 0, d <= 16384, x and q_out 16-byte aligned): one workgroup
 * per row keeps the row in registers between the maximum and the rounding, so x
 * is read once, with 16-byte loads and one 16-byte store per 16 elements. Every
 * other shape or alignment takes a scalar kernel with the same bits that reads
 * the row twice. n == 0 or d == 0 enqueues nothing; n > 2^31 - 1 is
 * MI355Q_UNSUPPORTED.
 *
 * mi355q_qfc_forward_i8: xq is int8 [n, d]; w the stored integer weight
 * [rows, d] of w_kind MI355Q_CMP_I8, _I4 or _I2 (I4 / I2 packed over the flat
 * tensor, element 0 in the low bits, as mi355q_pack_bits writes them); weight
 * zero points are 0.
 *   acc[t,r] = Sum_k (xq[t,k] - x_zero_point) * w[r,k]        (int32, exact)
 * formed as Sum xq * w - x_zero_point * Sum_k w[r,k], the second sum from a
 * kernel of its own into `workspace` (not launched when x_zero_point == 0).
 * x_scale has x_scale_count in {1, n} entries (one per token for dynamic rows).
 * block == 0 with w_scale_count in {1, rows}: one scale per tensor or per output
 * channel,
 *   y_out[t,r] = fl(float(acc[t,r]) * fl(x_scale[t] * w_scale[r]))
 * with the int32 -> float32 conversion rounding to nearest even. block in
 * {32, 64, 128, 256} with w_scale_count == rows * d / block: blockwise, the
 * accumulator of every block kept apart,
 *   y_out[t,r] = (...((0 + p_0) + p_1) + ...),
 *   p_b = fl(float(acc_b[t,r]) * fl(x_scale[t] * w_scale[r * d / block + b]))
 * in float32, blocks in ascending order, no FMA. acc_out is NULL or int32
 * [n, rows] and receives acc; with blockwise scales it must be NULL. A NaN
 * x_scale gives NaN outputs, which is no error.
 *
 * MFMA route: xq and w 16-byte aligned and d % 64 == 0 (d % 32 == 0 for block
 * 32). v_mfma_i32_16x16x64_i8 with A = a 16-token tile of xq and B = a
 * 16-channel tile of w, both contiguous along the reduction dimension: lane l
 * holds the 16 consecutive bytes k = 16 (l >> 4) .. + 15 of row l & 15 of each
 * (A and B share the assignment of k to lanes, so the sum does not depend on it);
 * C / D is column (channel) l & 15, row (token) 4 (l >> 4) + register. I4 / I2
 * fragments are 8 / 4 bytes unpacked and sign-extended in registers; no unpacked
 * weight is written to memory. Block 32 uses v_mfma_i32_16x16x32_i8 with 8
 * consecutive bytes per lane. A wave owns 64 tokens x 64 channels (4 x 4 MFMA
 * tiles: 8 fragment loads feed 16 MFMAs, the next step's loads in flight), a
 * workgroup 128 x 128. Generic route (every other d, e.g. odd d with packed
 * weights whose rows begin inside a byte, and misaligned xq or w): one thread
 * per output, one element at a time, the same bits.
 *
 * Refused before any launch: negative shapes, null xq / x_scale / w / w_scale /
 * y_out, another w_kind, x_zero_point outside int8, block outside {0, 32, 64,
 * 128, 256}, counts outside the sets above, acc_out with blockwise scales
 * (MI355Q_BAD_ARG); a block that does not divide d (MI355Q_BAD_SHAPE,
 * "Quantized dimension <d> is not divisible by block size <block>.");
 * d > 65536 (MI355Q_UNSUPPORTED: d * 255 * 128 must stay below 2^31). After
 * those n == 0 or rows == 0 enqueues nothing. workspace:
 * mi355q_qfc_forward_workspace_bytes(rows, d, block) = 4 * rows * (block ? d /
 * block : 1) rounded up to 256 bytes; it may be NULL when x_zero_point == 0.
 *
 * mi355q_sqdiff_cols_f64: a, b float32 [n, cols] row-major. Per column c
 *   sq_diff_cols[c] = Sum_t (double(a[t,c]) - double(b[t,c]))^2
 *   sq_b_cols[c]    = Sum_t double(b[t,c])^2
 * in FLOAT64 and in a fixed order: strand p (of P = 4 * min(64, ceil(n / 256)))
 * adds rows p, p + P, p + 2P, ... in ascending order, then a second kernel adds
 * a column's P partials in index order; no floating-point atomics, the same bits
 * in every run, |result - exact| <= n 2^-52 result. accumulate != 0 adds the
 * sums onto what the outputs hold (the samples of a calibration set, in order);
 * otherwise they are overwritten. cols == 0 enqueues nothing; n == 0 clears the
 * outputs unless accumulate. workspace: mi355q_sqdiff_cols_workspace_bytes(n, cols).
 * ------------------------------------------------------------------------ */
int32_t mi355q_qfc_quantize_rows_f32(const float* x, int64_t n, int64_t d, int8_t* q_out, float* scale_out,
                                     void* stream);
size_t mi355q_qfc_forward_workspace_bytes(int64_t rows, int64_t d, int32_t block);
int32_t mi355q_qfc_forward_i8(const int8_t* xq, int64_t n, int64_t d, const float* x_scale, int64_t x_scale_count,
                              int32_t x_zero_point, const void* w, int32_t w_kind, int64_t rows, const float* w_scale,
                              int64_t w_scale_count, int32_t block, float* y_out, int32_t* acc_out, void* workspace,
                              size_t workspace_bytes, void* stream);
size_t mi355q_sqdiff_cols_workspace_bytes(int64_t n, int64_t cols);
int32_t mi355q_sqdiff_cols_f64(const float* a, const float* b, int64_t n, int64_t cols, double* sq_diff_cols,
                               double* sq_b_cols, int32_t accumulate, void* workspace, size_t workspace_bytes,
                               void* stream);

/* ---------------------------------------------------------------------------
 * Integer execution, int16 activations (csrc/qfc16.hip): the FULLY_CONNECTED op
 * of an a16w8 model (static_wi8_ai16). The arithmetic is this library's own
 * definition.
 *
 * mi355q_qfc_forward_i16: xq is int16 [n, d] over the full range -32768 ..
 * 32767 with NO zero point (INT16 activations are symmetric); w, w_kind, rows,
 * w_scale, w_scale_count, block, x_scale and x_scale_count are as for
 * mi355q_qfc_forward_i8 (weight zero points 0).
 *   acc[t,r] = Sum_k xq[t,k] * w[r,k]                          (int64, exact)
 *   y_out[t,r] = fl32( double(acc[t,r]) * double( fl32(x_scale[t] * w_scale[r]) ) )
 * The scale product is rounded to float32; the accumulator (up to 39 bits) goes
 * through float64, where it is exact, so the rescale adds one float64 and one
 * float32 rounding and no float32 rounding of the integer itself. In NumPy:
 *   sc = xs[:, None] * sw[None, :]                              (float32)
 *   y = (acc.astype(np.float64) * sc.astype(np.float64)).astype(np.float32)
 * Blockwise (block in {32, 64, 128, 256}, w_scale_count == rows * d / block):
 * one exact accumulator per block,
 *   p_b = fl32( double(acc_b[t,r]) * double( fl32(x_scale[t] * w_scale[r * d / block + b]) ) )
 *   y_out[t,r] = (...((0 + p_0) + p_1) + ...)
 * in float32, blocks in ascending order, no FMA (the i8 entry's rule). acc_out
 * is NULL or int64 [n, rows]; with blockwise scales it must be NULL. A NaN
 * x_scale gives NaN outputs, which is no error.
 *
 * MFMA route (xq and w 16-byte aligned, d % 64 == 0, or d % 32 == 0 for block
 * 32): gfx950 has no int16 matrix instruction, so with h = x >> 8 (arithmetic,
 * -128 .. 127), l_u = x & 255 and l_s = int8(l_u ^ 0x80) = l_u - 128
 *   acc = 256 * Sum_k h w + Sum_k l_s w + 128 * Sum_k w[r,k]
 * The first two sums are int32-exact for d <= 65536 (each within 65536 * 128 *
 * 128 = 2^30) and run on v_mfma_i32_16x16x64_i8 (v_mfma_i32_16x16x32_i8 for
 * block 32); the third is the weight-sums kernel's, per row or per block, into
 * `workspace`; the three are combined in int64 in the epilogue. A lane's A
 * fragment is 16 consecutive int16 of a row of xq (two 16-byte loads), split
 * into the high-byte and the biased low-byte fragment in registers (v_perm_b32);
 * the B fragment is the i8 entry's, read and unpacked once per step for both
 * planes. Lane, row / column and C / D maps are the i8 entry's. A wave owns 32
 * tokens x 64 channels (2 x 4 MFMA tiles in two planes: 6 fragment loads feed
 * 16 MFMAs), a workgroup 64 x 128. Generic route (every other d or alignment):
 * one thread per output with an int64 accumulator, the same bits.
 *
 * Refused before any launch, with the i8 entry's texts: negative shapes, null
 * xq / x_scale / w / w_scale / y_out, another w_kind, block outside {0, 32, 64,
 * 128, 256}, counts outside the sets above, acc_out with blockwise scales
 * (MI355Q_BAD_ARG); a block that does not divide d (MI355Q_BAD_SHAPE); d > 65536
 * (MI355Q_UNSUPPORTED: the int32 planes); a workspace that is NULL or smaller
 * than mi355q_qfc_forward_i16_workspace_bytes(rows, d, block) = 4 * rows *
 * (block ? d / block : 1) rounded up to 256 bytes (MI355Q_BAD_ARG; the weight
 * sums are a term of every accumulator, so it is always required). After those
 * n == 0 or rows == 0 enqueues nothing.
 * ------------------------------------------------------------------------ */
size_t mi355q_qfc_forward_i16_workspace_bytes(int64_t rows, int64_t d, int32_t block);
int32_t mi355q_qfc_forward_i16(const int16_t* xq, int64_t n, int64_t d, const float* x_scale, int64_t x_scale_count,
                               const void* w, int32_t w_kind, int64_t rows, const float* w_scale, int64_t w_scale_count,
                               int32_t block, float* y_out, int64_t* acc_out, void* workspace, size_t workspace_bytes,
                               void* stream);

/* ---------------------------------------------------------------------------
 * Integer execution, through to the stored output (csrc/qfc_out.hip): what a
 * static FULLY_CONNECTED op (static_wi8_ai8, static_wi8_ai16) leaves in its
 * INT8 / INT16 output tensor, the tensor the next op reads: accumulator, bias,
 * fixed-point multiplier, output zero point, the fused activation's integer
 * range. The arithmetic is this library's own definition, modelled on LiteRT's
 * integer FULLY_CONNECTED; agreement with LiteRT's kernels has not been checked,
 * the claim is bit equality with the statement below. There is no blockwise
 * form: a static op has one accumulator per output.
 *
 * xq, w, w_kind, rows and x_zero_point are as for mi355q_qfc_forward_i8 /
 * mi355q_qfc_forward_i16 (weight zero points 0). bias is NULL (0) or has rows
 * entries; multiplier and shift have mcount in {1, rows} entries (M, s below:
 * one for the tensor, or one per output channel r).
 *
 * mi355q_qfc_output_i8 (xq int8 [n, d], bias int32, q_out int8 [n, rows]):
 *   acc = Sum_k (xq[t,k] - x_zero_point) * w[r,k]      (int32, exact, formed as
 *         the i8 forward entry forms it; no weight-sums launch when the zero
 *         point is 0)
 *   a   = sat32(int64(acc) + bias[r])
 *   mbqm32(a, M, s):  L = max(s, 0), R = max(-s, 0)
 *     v = sat32(int64(a) * 2^L)
 *     p = int64(v) * M
 *     h = (p + (p >= 0 ? 2^30 : 1 - 2^30)) / 2^31      (C++ truncating division)
 *     mask = 2^R - 1
 *     r = (h >> R) + ((h & mask) > (mask >> 1) + (h < 0))
 *   q_out[t,r] = clamp(r + out_zero_point, act_min, act_max)
 * sat32 clamps to [-2^31, 2^31 - 1]. The two sat32 are THIS LIBRARY'S CHOICE
 * where LiteRT's int32 arithmetic would overflow (a + bias, a * 2^L): with them
 * every intermediate is defined for every int32 input. Precondition: M >= 0 and
 * s in [-31, 30] (what a quantized multiplier of a positive real below 2^30 is);
 * the entry clamps s into that range so that no undefined shift is executed,
 * and does not check M (|p| stays below 2^62 for every int32 M).
 *
 * mi355q_qfc_output_i16 (xq int16 [n, d], bias int64, q_out int16 [n, rows];
 * no zero points):
 *   acc = Sum_k xq[t,k] * w[r,k]                         (int64, exact: the two
 *         int8 planes of the i16 forward entry plus 128 Sum_k w[r,k])
 *   a   = clamp(acc + bias[r], -2^47, 2^47 - 1)
 *   Mr  = M < 0x7FFF0000 ? (M + 2^15) >> 16 : 0x7FFF
 *   T   = 15 - s
 *   r   = (a * Mr + 2^(T - 1)) >> T                      (arithmetic shift)
 *   q_out[t,r] = clamp(r, act_min, act_max)
 * Precondition: M >= 0 and s in [-31, 14] (T in [1, 46]; |a * Mr| <= 2^62); the
 * entry clamps s into that range, and a bias beyond +-2^62 acts as +-2^62 (the
 * clamp of a gives the same).
 *
 * Routes are the forward entries': xq and w 16-byte aligned and d % 64 == 0
 * take v_mfma_i32_16x16x64_i8 with the forward kernels' lane and tile maps (a
 * wave owns 64 x 64 outputs, under int16 32 x 64 in two planes). The epilogue
 * runs on the accumulator tile IN REGISTERS and only q_out is stored: no
 * [n, rows] accumulator or float array is written to memory. In the C / D map a
 * lane's values of a tile column all belong to channel l & 15, so bias,
 * multiplier and shift are read once per 16-channel tile and lane. Every other
 * d or alignment: one thread per output, the same bits.
 *
 * Refused before any launch, with the forward entries' texts where they overlap:
 * negative shapes, null xq / w / multiplier / shift / q_out, another w_kind,
 * mcount outside {1, rows}, x_zero_point / out_zero_point outside int8,
 * act_min > act_max or either outside the output type (MI355Q_BAD_ARG);
 * d > 65536 (MI355Q_UNSUPPORTED); a workspace that is NULL or smaller than
 * mi355q_qfc_output_workspace_bytes(rows, d) = 4 * rows rounded up to 256 bytes
 * where one is needed: under int8 when x_zero_point != 0, under int16 always
 * (MI355Q_BAD_ARG). After those n == 0 or rows == 0 enqueues nothing.
 * ------------------------------------------------------------------------ */
size_t mi355q_qfc_output_workspace_bytes(int64_t rows, int64_t d);
int32_t mi355q_qfc_output_i8(const int8_t* xq, int64_t n, int64_t d, int32_t x_zero_point, const void* w, int32_t w_kind,
                             int64_t rows, const int32_t* bias, const int32_t* multiplier, const int32_t* shift,
                             int64_t mcount, int32_t out_zero_point, int32_t act_min, int32_t act_max, int8_t* q_out,
                             void* workspace, size_t workspace_bytes, void* stream);
int32_t mi355q_qfc_output_i16(const int16_t* xq, int64_t n, int64_t d, const void* w, int32_t w_kind, int64_t rows,
                              const int64_t* bias, const int32_t* multiplier, const int32_t* shift, int64_t mcount,
                              int32_t act_min, int32_t act_max, int16_t* q_out, void* workspace, size_t workspace_bytes,
                              void* stream);

/* ---------------------------------------------------------------------------
 * Patch gather for CONV_2D (csrc/conv_patches.hip): an NHWC activation
 * x [N, H, W, C] becomes the rows the integer FULLY_CONNECTED entries above
 * read. A TFLite filter is [O, KH, KW, I]: its reduction dimension
 * K = KH KW C is contiguous per output channel, so after this gather a
 * CONV_2D is the product xq [n, K] w [O, K]^T those entries execute.
 *
 * Statement. For t in [first_row, first_row + row_count):
 *   n = t / (OH OW)      oh = (t / OW) % OH      ow = t % OW
 * and for k = (kh KW + kw) C + c:
 *   ih = oh stride_h - pad_top + kh dil_h
 *   iw = ow stride_w - pad_left + kw dil_w
 *   out[(t - first_row) K + k] = x[((n H + ih) W + iw) C + c]
 *                                          when 0 <= ih < H and 0 <= iw < W
 *                              = *pad_element                    otherwise
 * Elements are elem_bytes (1, 2 or 4) wide and are copied as bytes: a float
 * NaN keeps its payload and -0.0 its sign. pad_element is a HOST pointer to one
 * element, read before the call returns (the activation's zero point for an
 * integer tensor, so that q - zp = 0 in a padded tap). OH, OW, pad_top and
 * pad_left are the caller's (for TFLite's SAME / VALID: ops.conv_geometry);
 * whatever they are, no element outside x is read. All index arithmetic is
 * 64-bit: N H W C may exceed 2^31. The window [first_row, first_row +
 * row_count) lets a caller walk the patch rows in chunks, so that no
 * [N OH OW, K] array has to exist.
 *
 * Routes. C elem_bytes % 16 == 0 with x and out 16-byte aligned: every 16-byte
 * piece of a patch row lies inside one tap and rows of out are 16-byte
 * aligned; one lane moves one piece (a 16-byte load, or the splatted pad
 * element, and a 16-byte store) and consecutive lanes write consecutive pieces.
 * Everything else: one element per thread. Both write the same bytes.
 *
 * Refused before any launch: elem_bytes outside {1, 2, 4}; N, H, W, C, KH, KW,
 * OH, OW, a stride or a dilation that is not positive; a negative first_row or
 * row_count; first_row + row_count > N OH OW (MI355Q_BAD_ARG); K > 65536, the
 * forward entries' limit; N OH OW > INT32_MAX; an activation beyond 2^62 bytes
 * (MI355Q_UNSUPPORTED). After those row_count == 0 enqueues nothing, whatever
 * the pointers; otherwise a null x, out or pad_element is MI355Q_BAD_ARG. A
 * request of 2^32 units or more (a launch holds fewer work-items) runs as one
 * launch whose lanes stride over the units with a 64-bit index.
 * ------------------------------------------------------------------------ */
int32_t mi355q_conv_patches_nhwc(const void* x, int32_t elem_bytes, int64_t N, int64_t H, int64_t W, int64_t C, int32_t KH,
                                 int32_t KW, int32_t stride_h, int32_t stride_w, int32_t dil_h, int32_t dil_w,
                                 int32_t pad_top, int32_t pad_left, int64_t OH, int64_t OW, int64_t first_row,
                                 int64_t row_count, const void* pad_element, void* out, void* stream);

/* ---------------------------------------------------------------------------
 * Patch gather for TRANSPOSE_CONV (csrc/conv_patches.hip): one sub-pixel
 * phase of a transposed convolution as the rows the integer FULLY_CONNECTED
 * entries read. A TFLite TRANSPOSE_CONV of x [N, IH, IW, C] with a filter
 * [O, KH, KW, C] and strides (sh, sw) writes out [N, OH, OW, O],
 *   out[n, oy, ox, o] = Sum_{ky, kx, c} x[n, a, b, c] W[o, ky, kx, c]
 * over the taps with (oy + pad_top - ky) % sh == 0, a = (oy + pad_top - ky) / sh
 * in [0, IH), and likewise b from ox, pad_left, kx and sw. (pad_top, pad_left)
 * is the padding of the FORWARD convolution from [OH, OW] back to [IH, IW]
 * (TFLite's rule, no dilation). The output pixels of one phase (py, px),
 * oy = qy sh + py and ox = qx sw + px, all use the same taps
 *   kys = {ky : (py + pad_top - ky) % sh == 0} = ry, ry + sh, ... < KH
 *   kxs likewise,   ry = (py + pad_top) % sh
 * so the phase is an ordinary product of its patch rows with the filter slice
 * W[:, kys][:, :, kxs] viewed as [O, |kys| |kxs| C], and the phases together
 * multiply no hole: a gather of full KH KW C rows over a zero-stuffed input
 * would multiply sh sw - 1 of every sh sw taps by nothing.
 *
 * Statement. With QH = ceil((OH - py) / sh), QW = ceil((OW - px) / sw),
 * TH = |kys|, TW = |kxs|, K = TH TW C, by = (py + pad_top) / sh and
 * bx = (px + pad_left) / sw (integer divisions, on the host), for
 * t in [first_row, first_row + row_count):
 *   n = t / (QH QW)      qy = (t / QW) % QH      qx = t % QW
 * and for k = (ti TW + tj) C + c  (tap ky = ry + ti sh, kx = rx + tj sw):
 *   a = qy + by - ti      b = qx + bx - tj
 *   out[(t - first_row) K + k] = x[((n IH + a) IW + b) C + c]
 *                                          when 0 <= a < IH and 0 <= b < IW
 *                              = *pad_element                    otherwise
 * Elements, pad_element, the byte copy, the two routes, the 64-bit index
 * arithmetic and the window are those of the CONV_2D gather above, and so is
 * the kernel: the phase is its stride-1 gather with a dilation of -1. Whatever
 * the arguments, no element outside x is read.
 *
 * Refused before any launch: elem_bytes outside {1, 2, 4}; N, IH, IW, C, KH,
 * KW, OH, OW or a stride that is not positive; a phase outside
 * [0, stride_h) x [0, stride_w); a negative first_row or row_count
 * (MI355Q_BAD_ARG); N, IH, IW, OH or OW above INT32_MAX (MI355Q_UNSUPPORTED);
 * a geometry whose forward convolution does not map [OH, OW] to [IH, IW]: per
 * axis IH = ceil(OH / sh) (SAME) or IH = (OH + sh - KH) / sh (VALID), and
 * pad_top = max(0, (IH - 1) sh + KH - OH) / 2 (MI355Q_BAD_ARG); a phase with no
 * tap, ry >= KH, which a stride above the kernel leaves (MI355Q_UNSUPPORTED);
 * K > 65536; N QH QW > INT32_MAX (MI355Q_UNSUPPORTED); first_row + row_count >
 * N QH QW (MI355Q_BAD_ARG; a phase with py >= OH has no rows). Those limits
 * keep the activation far below the 2^62 bytes of the CONV_2D entry. After
 * those row_count == 0 enqueues nothing; otherwise a null x, out or
 * pad_element is MI355Q_BAD_ARG.
 * ------------------------------------------------------------------------ */
int32_t mi355q_tconv_patches_nhwc(const void* x, int32_t elem_bytes, int64_t N, int64_t IH, int64_t IW, int64_t C, int32_t KH,
                                  int32_t KW, int32_t stride_h, int32_t stride_w, int32_t pad_top, int32_t pad_left,
                                  int64_t OH, int64_t OW, int32_t phase_h, int32_t phase_w, int64_t first_row,
                                  int64_t row_count, const void* pad_element, void* out, void* stream);

/* ---------------------------------------------------------------------------
 * Direct depthwise convolution (csrc/dwconv.hip): the DEPTHWISE_CONV_2D op on
 * an NHWC activation, in float32 and in integers. A TFLite depthwise filter is
 * [1, KH, KW, O]: the reduction of an output channel is its KH KW taps alone,
 * they are NOT contiguous, and every output channel reads ONE input channel, so
 * neither the patch gather above nor a shared GEMM applies. The arithmetic is
 * this library's own definition, modelled on LiteRT's DEPTHWISE_CONV_2D;
 * agreement with LiteRT's kernels has not been checked, the claim is bit
 * equality with the statement below.
 *
 * Geometry of every entry. x [N, H, W, C]; w [KH, KW, O] with O = C M (the
 * stored bytes of the [1, KH, KW, O] filter), M >= 1 the depth multiplier;
 * output channel oc reads input channel oc / M. Strides, dilations, pad_top,
 * pad_left, OH and OW are the caller's (ops.conv_geometry), and the window
 * [first_row, first_row + row_count) over the N OH OW output rows has the
 * gather's meaning. Outputs are row-major [row_count, O], what
 * mi355q_sqdiff_cols_f64 reads. For t in the window and oc in [0, O):
 *   n = t / (OH OW)      oh = (t / OW) % OH      ow = t % OW
 *   ih = oh stride_h - pad_top + kh dil_h      iw = ow stride_w - pad_left + kw dil_w
 * and the taps (kh, kw) are taken in ascending (kh, kw) order. A tap with ih
 * outside [0, H) or iw outside [0, W) is SKIPPED: it adds nothing, and no
 * element outside x is read, whatever the geometry arguments are. All index
 * arithmetic is 64-bit.
 *
 * mi355q_dwconv_forward_f32 (x, w float32):
 *   p(kh,kw) = fl32( x[n, ih, iw, oc / M] * w[kh, kw, oc] )
 *   y_out[t - first_row, oc] = (...((0 + p_0) + p_1) + ...)      taps inside
 * every product and every sum rounded to float32, no FMA contraction: the bits
 * of a NumPy float32 loop in that order (a first product of -0.0 gives +0.0,
 * as 0 + -0.0 does). This is the float op's pre-bias product, and with the
 * dequantized filter the weight-only route. Infinities and NaNs follow IEEE.
 *
 * mi355q_dwconv_forward_i8 (xq int8, w int8: w_kind MI355Q_CMP_I8 alone,
 * weight zero points 0):
 *   acc[t,oc] = Sum_{taps inside} (xq - x_zero_point) * w          (int32, exact:
 *               KH KW <= 65536 taps of at most 255 * 128)
 *   y_out[t,oc] = fl32( float(acc) * fl32(x_scale[.] * w_scale[.]) )
 * x_scale_count is 1 or N: ONE SCALE PER IMAGE, row t reads entry t / (OH OW)
 * (the dynamic mode of the conv path); w_scale_count is 1 or O. acc_out is NULL
 * or int32 [row_count, O].
 *
 * mi355q_dwconv_forward_i16 (xq int16 over its full range, no zero point):
 *   acc exact in int64
 *   y_out[t,oc] = fl32( double(acc) * double( fl32(x_scale[.] * w_scale[.]) ) )
 * the rescale of mi355q_qfc_forward_i16. acc_out is NULL or int64.
 *
 * mi355q_dwconv_output_i8 / mi355q_dwconv_output_i16: the same accumulators
 * taken through to the stored tensor with the arithmetic of
 * mi355q_qfc_output_i8 / mi355q_qfc_output_i16 UNCHANGED (one piece of device
 * code, csrc/qfc_epilogue.h): bias int32 / int64 (NULL: 0) with O entries,
 * sat32, mbqm32 (int16: Mr, T), out_zero_point, [act_min, act_max], int8 /
 * int16 store; multiplier and shift have mcount in {1, O} entries. The
 * epilogue runs on the accumulator in registers and only q_out [row_count, O]
 * is written.
 *
 * Routes; both give the same bits. Vector route (M == 1, C % 4 == 0, and x, w,
 * the outputs given and the per-channel vectors given 16-byte aligned): a lane
 * owns 4 consecutive channels of one output pixel, consecutive lanes take
 * consecutive channel groups and then the next pixel, so that per tap the
 * activation loads (16 / 4 / 8 bytes per lane for float32 / int8 / int16), the
 * filter loads and the stores are contiguous across the wave; float32 y_out
 * and int32 acc_out leave as 16-byte stores, int64 acc_out as two. The filter
 * is read through the caches by every pixel. Generic route (every other M, C
 * or alignment): one thread per output element. A request of 2^32 units or
 * more runs as one launch whose lanes stride over the units with a 64-bit
 * index. No kernel uses scratch memory.
 *
 * Refused before any launch, with the neighbouring entries' texts where they
 * overlap: N, H, W, C, KH, KW, OH, OW, M, a stride or a dilation that is not
 * positive; a negative first_row or row_count; first_row + row_count >
 * N OH OW; a w_kind other than MI355Q_CMP_I8; x_scale_count outside {1, N},
 * w_scale_count or mcount outside {1, O}; x_zero_point / out_zero_point
 * outside int8; act_min > act_max or either outside the output type
 * (MI355Q_BAD_ARG); KH KW > 65536; N OH OW > INT32_MAX; an activation beyond
 * 2^62 bytes; O > INT32_MAX (MI355Q_UNSUPPORTED). After those row_count == 0
 * enqueues nothing, whatever the pointers; otherwise a null x / xq, w,
 * x_scale, w_scale, multiplier, shift, y_out or q_out is MI355Q_BAD_ARG.
 * ------------------------------------------------------------------------ */
int32_t mi355q_dwconv_forward_f32(const float* x, int64_t N, int64_t H, int64_t W, int64_t C, const float* w, int32_t KH,
                                  int32_t KW, int32_t M, int32_t stride_h, int32_t stride_w, int32_t dil_h, int32_t dil_w,
                                  int32_t pad_top, int32_t pad_left, int64_t OH, int64_t OW, int64_t first_row,
                                  int64_t row_count, float* y_out, void* stream);
int32_t mi355q_dwconv_forward_i8(const int8_t* xq, int64_t N, int64_t H, int64_t W, int64_t C, const float* x_scale,
                                 int64_t x_scale_count, int32_t x_zero_point, const void* w, int32_t w_kind, int32_t KH,
                                 int32_t KW, int32_t M, const float* w_scale, int64_t w_scale_count, int32_t stride_h,
                                 int32_t stride_w, int32_t dil_h, int32_t dil_w, int32_t pad_top, int32_t pad_left,
                                 int64_t OH, int64_t OW, int64_t first_row, int64_t row_count, float* y_out,
                                 int32_t* acc_out, void* stream);
int32_t mi355q_dwconv_forward_i16(const int16_t* xq, int64_t N, int64_t H, int64_t W, int64_t C, const float* x_scale,
                                  int64_t x_scale_count, const void* w, int32_t w_kind, int32_t KH, int32_t KW, int32_t M,
                                  const float* w_scale, int64_t w_scale_count, int32_t stride_h, int32_t stride_w,
                                  int32_t dil_h, int32_t dil_w, int32_t pad_top, int32_t pad_left, int64_t OH, int64_t OW,
                                  int64_t first_row, int64_t row_count, float* y_out, int64_t* acc_out, void* stream);
int32_t mi355q_dwconv_output_i8(const int8_t* xq, int64_t N, int64_t H, int64_t W, int64_t C, int32_t x_zero_point,
                                const void* w, int32_t w_kind, int32_t KH, int32_t KW, int32_t M, const int32_t* bias,
                                const int32_t* multiplier, const int32_t* shift, int64_t mcount, int32_t out_zero_point,
                                int32_t act_min, int32_t act_max, int32_t stride_h, int32_t stride_w, int32_t dil_h,
                                int32_t dil_w, int32_t pad_top, int32_t pad_left, int64_t OH, int64_t OW, int64_t first_row,
                                int64_t row_count, int8_t* q_out, void* stream);
int32_t mi355q_dwconv_output_i16(const int16_t* xq, int64_t N, int64_t H, int64_t W, int64_t C, const void* w,
                                 int32_t w_kind, int32_t KH, int32_t KW, int32_t M, const int64_t* bias,
                                 const int32_t* multiplier, const int32_t* shift, int64_t mcount, int32_t act_min,
                                 int32_t act_max, int32_t stride_h, int32_t stride_w, int32_t dil_h, int32_t dil_w,
                                 int32_t pad_top, int32_t pad_left, int64_t OH, int64_t OW, int64_t first_row,
                                 int64_t row_count, int16_t* q_out, void* stream);

/* ---------------------------------------------------------------------------
 * Integer batched matrix product (csrc/qbmm.hip): the BATCH_MATMUL op with
 * int8 operands that BOTH carry a zero point, as the two attention products
 * of a statically quantized transformer have them (Q K^T with adj_y, P V
 * without). The arithmetic is this library's own definition, modelled on
 * LiteRT's BATCH_MATMUL; agreement with LiteRT's kernels has not been checked,
 * the claim is bit equality with the statement below.
 *
 * Statement. a is int8 [batch, M, K], or [batch, K, M] with adj_x; b is int8
 * [b_batch, K, N], or [b_batch, N, K] with adj_y; b_batch is 1 or batch, and
 * with b_batch = 1 the one matrix serves every batch (b' = 0, else b' = b).
 *   acc[b,m,n] = Sum_k (A[b,m,k] - a_zero_point) (B[b',k,n] - b_zero_point)
 * exact in int32: a term is at most 255 * 255 in magnitude, so K <= 32768
 * keeps |acc| <= 2 130 739 200 < 2^31; a larger K is refused.
 *   mi355q_qbmm_forward_i8:
 *     y_out[b,m,n] = fl32( float(acc) * fl32(a_scale[.] * b_scale[.]) )
 *   FULLY_CONNECTED's form. a_scale has 1 or batch M entries (entry b M + m:
 *   the per-row scales of the dynamic mode, meaningful without adj_x), b_scale
 *   1 or N. y_out is float32 [batch, M, N]; acc_out is NULL or int32
 *   [batch, M, N].
 *   mi355q_qbmm_output_i8:
 *     q_out[b,m,n] = clamp(mbqm32(acc, M[.], s[.]) + out_zero_point, -128, 127)
 *   int8 [batch, M, N], with the fixed-point requantization of
 *   mi355q_qfc_output_i8 UNCHANGED (one piece of device code,
 *   csrc/qfc_epilogue.h). BatchMatMulOptions has neither a bias nor a fused
 *   activation, so the epilogue gets no bias and the full int8 range;
 *   multiplier and shift have mcount in {1, N} entries. Only q_out is written.
 *
 * Routes; both give the same bits. MFMA route (K % 64 == 0, a and b 16-byte
 * aligned, M % 16 == 0 with adj_x, N % 16 == 0 without adj_y): Sum a b on
 * v_mfma_i32_16x16x64_i8 with the main loop and the tile of the
 * FULLY_CONNECTED route (qfc_tile.h): a wave on 64 x 64 outputs, a workgroup
 * of 2 x 2 waves on 128 x 128, the batch along the grid's z, both operands
 * read contiguous along K, 16 consecutive k per lane. An operand that is
 * strided along K (a with adj_x; b without adj_y, the default layout) is
 * first TRANSPOSED into the workspace by a pre-pass (64 x 64 byte tiles
 * through LDS, 16-byte loads and stores). Staging such an operand through LDS
 * inside the product (16-byte loads, a 4 x 4 byte transpose with v_perm_b32,
 * 16-byte read-back) was built and measured 5.3 - 6.6 x slower than
 * transposing first (profiles/qbmm_staged_bench.json), so it was not
 * kept. The zero points enter through operand sums,
 *   acc = Sum a b - zb Sum_k a - za Sum_k b + K za zb,
 * taken by a pre-pass into the workspace (Sum_k a only when zb != 0, Sum_k b
 * only when za != 0; each sum is at most 2^22 in magnitude and exact in
 * int32). Each of the four terms is at most 2^29 in magnitude and exact in
 * int32, but a partial sum of them can pass 2^31: they are combined in
 * uint32, whose wrap-around is defined, which gives the total modulo 2^32,
 * and the total lies within int32 by the bound above. No intermediate needs
 * int64. batch = 1 with (adj_x, adj_y) = (0, 1) and b_zero_point = 0 is the
 * FULLY_CONNECTED problem and mi355q_qbmm_forward_i8 hands it to
 * mi355q_qfc_forward_i8: same statement, same bits. Generic route (every other K, M, N or
 * alignment, K = 1 and misaligned bases among them): one thread per output
 * forms Sum (a - za)(b - zb) one element at a time in int32, which the bound
 * keeps exact. Tile edges in M, N and the batch are guarded; no kernel uses
 * scratch memory.
 *
 * Workspace. mi355q_qbmm_workspace_bytes is the most a call of these shapes
 * can need: the two sums, plus a copy of every operand that is strided along
 * K. With za = zb = 0 no sum is computed, and for (adj_x, adj_y) = (0, 1)
 * the workspace may then be NULL; a non-zero zero point needs the sums' part
 * on either route, and a K-strided operand on the MFMA route the whole, at a
 * 16-byte aligned address.
 *
 * Refused before any launch: a negative batch, M, K, N or b_batch; a null a
 * or b; a zero point outside int8 (MI355Q_BAD_ARG); b_batch outside
 * {1, batch} (MI355Q_BAD_SHAPE); K > 32768 (MI355Q_UNSUPPORTED); a null
 * a_scale, b_scale, y_out, multiplier, shift or q_out; a_scale_count outside
 * {1, batch M}, b_scale_count or mcount outside {1, N}; out_zero_point
 * outside int8; with a non-zero zero point a workspace that is NULL, too
 * small for the sums or not 4-byte aligned (MI355Q_BAD_ARG). After those batch, M or N == 0
 * enqueues nothing; K == 0 is the empty sum, acc = 0, on the generic route.
 * On the MFMA route a workspace that is NULL, misaligned or too small for
 * the transposed copies is MI355Q_BAD_ARG, more than 65535 batches or tiles
 * of 128 rows of M MI355Q_UNSUPPORTED. mi355q_qbmm_mfma_route answers on the
 * host, reading nothing, whether a call with these bases and shapes takes
 * the MFMA route (1) or the generic one (0).
 * ------------------------------------------------------------------------ */
int64_t mi355q_qbmm_mfma_route(const void* a, int64_t M, int64_t K, int32_t adj_x, const void* b, int64_t N, int32_t adj_y);
size_t mi355q_qbmm_workspace_bytes(int64_t batch, int64_t M, int64_t K, int32_t adj_x, int64_t b_batch, int64_t N,
                                   int32_t adj_y);
int32_t mi355q_qbmm_forward_i8(const int8_t* a, int64_t batch, int64_t M, int64_t K, int32_t adj_x, const float* a_scale,
                               int64_t a_scale_count, int32_t a_zero_point, const int8_t* b, int64_t b_batch, int64_t N,
                               int32_t adj_y, const float* b_scale, int64_t b_scale_count, int32_t b_zero_point,
                               float* y_out, int32_t* acc_out, void* workspace, size_t workspace_bytes, void* stream);
int32_t mi355q_qbmm_output_i8(const int8_t* a, int64_t batch, int64_t M, int64_t K, int32_t adj_x, int32_t a_zero_point,
                              const int8_t* b, int64_t b_batch, int64_t N, int32_t adj_y, int32_t b_zero_point,
                              const int32_t* multiplier, const int32_t* shift, int64_t mcount, int32_t out_zero_point,
                              int8_t* q_out, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif
#endif /* MI355Q_H_ */
