// Integer execution of a quantized FULLY_CONNECTED op on calibration data (include/mi355q.h, "Integer execution").
//
//   quantize_rows_*_kernel  the dynamic-range activation quantizer: per row t, range = max |x|, s_x = range / 127,
//                           q = clamp(round_half_away_from_zero(fl(x * (127 / range))), -127, 127). The vector route
//                           keeps the row in registers between the maximum and the rounding (one read of x), 16 floats
//                           per lane and chunk, and stores 16 int8 at once; the scalar route reads the row twice.
//   weight_sums_kernel      wsum[r][b] = Sum_k q_w[r][b * L + k] (int32, exact), the zero-point term of the accumulator
//                           (qfc_frag.h, with the weight fragments: qfc16.hip and qfc_out.hip use both as well).
//   qfc_mfma_kernel         acc = Xq W^^T on the int8 matrix cores: the main loop of qfc_tile.h with int8 activations.
//                           A lane's A fragment is 16 consecutive bytes of a row of Xq and its B fragment 16
//                           consecutive elements of a row of W^ (8 bytes of int4, 4 bytes of int2, unpacked and
//                           sign-extended in registers). A wave owns 64 tokens x 64 output channels = 4 x 4 MFMA tiles
//                           of v_mfma_i32_16x16x64_i8, and the four waves of a workgroup (128 x 128) share rows
//                           through L1 / L2. Block 32 uses v_mfma_i32_16x16x32_i8 (8 bytes per lane). This file adds
//                           the float rescale: blockwise scales flush the int32 tile into float32 sums after every
//                           block, in ascending order, without FMA.
//   qfc_generic_kernel      one thread per output, element by element: every other shape and alignment, same bits.
//   sqdiff_cols_*_kernel    per column Sum_t (a - b)^2 and Sum_t b^2 in float64 in a fixed order.
#include "common.h"
#include "compare_target.h"
#include "qfc_tile.h"

namespace mi355q {
namespace {

constexpr int kThreads = kQfcThreads;
constexpr int kVecMaxD = 16384;       // a row of the vector quantizer: 256 threads x 4 chunks x 16 floats

struct __attribute__((aligned(16))) F4 { float x, y, z, w; };
struct __attribute__((aligned(16))) U4 { uint32_t x, y, z, w; };

// ---------------------------------------------------------------- dynamic activation rows
struct RowScale {
  float s, inv;
  bool zero;   // every q of the row is 0
};

// m = the row's largest |x| bit pattern (NaN sorts above inf, common.h abs_bits)
__device__ __forceinline__ RowScale row_scale(uint32_t m) {
  if (m >= 0x7F800000u) return RowScale{u2f(0x7FC00000u), 0.f, true};
  if (m == 0u) return RowScale{1.0f, 0.f, true};
  const float range = u2f(m);
  return RowScale{range / 127.0f, 127.0f / range, false};
}

// clamp(round_half_away_from_zero(v), -127, 127); v - trunc(v) is exact in float32, so 0.49999997f gives 0
__device__ __forceinline__ int round_away_clamp(float v) {
  if (v != v) return 0;
  float r = __builtin_truncf(v);
  const float f = v - r;
  if (f >= 0.5f) r += 1.0f;
  else if (f <= -0.5f) r -= 1.0f;
  r = fminf(fmaxf(r, -127.0f), 127.0f);
  return static_cast<int>(r);
}

__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }

__device__ __forceinline__ uint32_t block_max(uint32_t v, uint32_t* sm) {
  v = group_max_u32<kWave>(v);
  if ((threadIdx.x & (kWave - 1)) == 0) sm[threadIdx.x / kWave] = v;
  __syncthreads();
  return umax(umax(sm[0], sm[1]), umax(sm[2], sm[3]));
}

__device__ __forceinline__ uint32_t quantize4(const F4& v, const RowScale& rs) {
  if (rs.zero) return 0u;
  const uint32_t a = static_cast<uint32_t>(round_away_clamp(v.x * rs.inv)) & 0xFFu;
  const uint32_t b = static_cast<uint32_t>(round_away_clamp(v.y * rs.inv)) & 0xFFu;
  const uint32_t c = static_cast<uint32_t>(round_away_clamp(v.z * rs.inv)) & 0xFFu;
  const uint32_t e = static_cast<uint32_t>(round_away_clamp(v.w * rs.inv)) & 0xFFu;
  return a | (b << 8) | (c << 16) | (e << 24);
}

// One workgroup per row, d % 16 == 0, d <= 256 * CH * 16, x and q 16-byte aligned. Chunk c = 16 consecutive floats.
template <int CH>
__global__ __launch_bounds__(kThreads) void quantize_rows_vec_kernel(const float* __restrict__ x, long long d,
                                                                     int8_t* __restrict__ q, float* __restrict__ scale) {
  __shared__ uint32_t sm[kThreads / kWave];
  const long long row = blockIdx.x;
  const F4* xr = reinterpret_cast<const F4*>(x + row * d);
  const int chunks = static_cast<int>(d / 16);
  F4 v[CH][4];
  uint32_t m = 0;
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    const int c = threadIdx.x + kThreads * i;
    if (c < chunks) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[i][j] = xr[c * 4 + j];
        m = umax(m, umax(umax(abs_bits(v[i][j].x), abs_bits(v[i][j].y)), umax(abs_bits(v[i][j].z), abs_bits(v[i][j].w))));
      }
    }
  }
  const RowScale rs = row_scale(block_max(m, sm));
  if (threadIdx.x == 0) scale[row] = rs.s;
  U4* qr = reinterpret_cast<U4*>(q + row * d);
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    const int c = threadIdx.x + kThreads * i;
    if (c < chunks)
      qr[c] = U4{quantize4(v[i][0], rs), quantize4(v[i][1], rs), quantize4(v[i][2], rs), quantize4(v[i][3], rs)};
  }
}

// Every other shape and alignment: one workgroup per row, the row read twice, the same arithmetic.
__global__ __launch_bounds__(kThreads) void quantize_rows_scalar_kernel(const float* __restrict__ x, long long d,
                                                                        int8_t* __restrict__ q,
                                                                        float* __restrict__ scale) {
  __shared__ uint32_t sm[kThreads / kWave];
  const long long row = blockIdx.x;
  const float* xr = x + row * d;
  uint32_t m = 0;
  for (long long k = threadIdx.x; k < d; k += kThreads) m = umax(m, abs_bits(xr[k]));
  const RowScale rs = row_scale(block_max(m, sm));
  if (threadIdx.x == 0) scale[row] = rs.s;
  int8_t* qr = q + row * d;
  for (long long k = threadIdx.x; k < d; k += kThreads)
    qr[k] = rs.zero ? static_cast<int8_t>(0) : static_cast<int8_t>(round_away_clamp(xr[k] * rs.inv));
}

// ---------------------------------------------------------------- the integer product
struct FwdArgs {
  const int8_t* xq;        // [n, d]
  const uint8_t* w;        // [rows, d] stored
  const float* x_scale;    // 1 or n
  const float* w_scale;    // 1, rows or rows * nblocks
  const int32_t* wsum;     // [rows, nblocks] (read only when zp != 0)
  float* y;                // [n, rows]
  int32_t* acc;            // [n, rows] or null
  long long n, rows, d;
  int x_per_row;           // x_scale has n entries
  int w_mode;              // 0 per tensor, 1 per channel, 2 blockwise
  int nblocks;             // blocks per weight row (1 unless blockwise)
  int block;               // elements per block (d unless blockwise)
  int zp;
  int kind;
};

struct ChanF {
  float sw;      // the channel's weight scale
  int corr;      // zp * Sum_k q_w[r][k]
};

template <int KIND, int KSTEP, bool BLOCKWISE>
__global__ __launch_bounds__(kThreads) void qfc_mfma_kernel(FwdArgs g) {
  constexpr int TA = QfcTile<int8_t>::TA;
  QfcWave wv;
  if (!qfc_wave<int8_t>(wv, g.n, g.rows)) return;

  I32x4 acc[QfcTile<int8_t>::TM][TB];
  float yf[TA][TB][4];
#pragma unroll
  for (int a = 0; a < TA; ++a)
#pragma unroll
    for (int b = 0; b < TB; ++b)
#pragma unroll
      for (int i = 0; i < 4; ++i) yf[a][b][i] = 0.0f;
  float sx[TA][4];
  if constexpr (BLOCKWISE) {
#pragma unroll
    for (int a = 0; a < TA; ++a)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long long t = wv.t0 + a * MF + wv.fg * 4 + i;
        sx[a][i] = t < g.n ? g.x_scale[g.x_per_row ? t : 0] : 0.0f;
      }
    // p_b = fl(float(acc_b) * fl(s_x * s_w[r, b])), y = y + p_b: blocks in ascending order, no FMA
    qfc_main_loop<int8_t, KIND, KSTEP>(wv, g.xq, g.w, g.n, g.rows, g.d, acc, g.block / KSTEP, [=, &acc, &yf](int bi) {
#pragma unroll
      for (int b = 0; b < TB; ++b) {
        const long long r = wv.r0 + b * MF + wv.fr;
        const bool rok = r < g.rows;
        const float sw = rok ? g.w_scale[r * g.nblocks + bi] : 0.0f;
        const int corr = (rok && g.zp != 0) ? g.zp * g.wsum[r * g.nblocks + bi] : 0;
#pragma unroll
        for (int a = 0; a < TA; ++a)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float sc = sx[a][i] * sw;
            const float p = static_cast<float>(acc[a][b][i] - corr) * sc;
            yf[a][b][i] = yf[a][b][i] + p;
            acc[a][b][i] = 0;
          }
      }
    });
  } else {
    qfc_main_loop<int8_t, KIND, KSTEP>(wv, g.xq, g.w, g.n, g.rows, g.d, acc);
  }

  qfc_walk_outputs<int8_t>(
      wv, g.n, g.rows,
      [=](long long r) {
        if (BLOCKWISE) return ChanF{0.0f, 0};
        return ChanF{g.w_scale[g.w_mode == 1 ? r : 0], g.zp != 0 ? g.zp * g.wsum[r] : 0};
      },
      [=, &acc, &yf](const ChanF& c, int a, int b, int i, long long t, long long r) {
        if (BLOCKWISE) {
          g.y[t * g.rows + r] = yf[a][b][i];
        } else {
          const int v = acc[a][b][i] - c.corr;
          const float sc = g.x_scale[g.x_per_row ? t : 0] * c.sw;
          g.y[t * g.rows + r] = static_cast<float>(v) * sc;
          if (g.acc) g.acc[t * g.rows + r] = v;
        }
      });
}

// Generic route: one thread per output element, one weight element at a time.
__global__ __launch_bounds__(kThreads) void qfc_generic_kernel(FwdArgs g) {
  const long long total = g.n * g.rows, step = static_cast<long long>(gridDim.x) * kThreads;
  for (long long o = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; o < total; o += step) {
    const long long t = o / g.rows, r = o % g.rows;
    const float s_x = g.x_scale[g.x_per_row ? t : 0];
    float y = 0.0f;
    for (int b = 0; b < g.nblocks; ++b) {
      int acc = qfc_dot<int>(g.xq + t * g.d, g.w, g.kind, r * g.d, static_cast<long long>(b) * g.block, g.block, 0);
      if (g.zp != 0) acc -= g.zp * g.wsum[r * g.nblocks + b];
      if (g.w_mode == 2) {
        const float sc = s_x * g.w_scale[r * g.nblocks + b];
        const float p = static_cast<float>(acc) * sc;
        y = y + p;
      } else {
        const float sc = s_x * g.w_scale[g.w_mode == 1 ? r : 0];
        y = static_cast<float>(acc) * sc;
        if (g.acc) g.acc[o] = acc;
      }
    }
    g.y[o] = y;
  }
}

template <int KIND>
void launch_mfma(const FwdArgs& g, bool blockwise, dim3 grid, hipStream_t st) {
  if (!blockwise) hipLaunchKernelGGL((qfc_mfma_kernel<KIND, 64, false>), grid, dim3(kThreads), 0, st, g);
  else if (g.block == 32) hipLaunchKernelGGL((qfc_mfma_kernel<KIND, 32, true>), grid, dim3(kThreads), 0, st, g);
  else hipLaunchKernelGGL((qfc_mfma_kernel<KIND, 64, true>), grid, dim3(kThreads), 0, st, g);
}

// ---------------------------------------------------------------- per-column squared differences
constexpr int kColsPerBlock = 64;                       // one lane per column: coalesced rows
constexpr int kRowLanes = kThreads / kColsPerBlock;     // 4 row strands per workgroup
constexpr int kRowsPerStrand = 64;                      // aimed-at rows per strand
constexpr int kMaxRowBlocks = 64;

int sqdiff_row_blocks(int64_t n) {
  const int64_t want = (n + kRowLanes * kRowsPerStrand - 1) / (kRowLanes * kRowsPerStrand);
  return static_cast<int>(want < 1 ? 1 : want > kMaxRowBlocks ? kMaxRowBlocks : want);
}

size_t sqdiff_workspace(int64_t n, int64_t cols) {
  const size_t strands = static_cast<size_t>(sqdiff_row_blocks(n)) * kRowLanes;
  return (2 * strands * static_cast<size_t>(cols) * sizeof(double) + 255) & ~static_cast<size_t>(255);
}

// strand p = blockIdx.y * kRowLanes + (thread / 64) adds rows p, p + P, p + 2P, ... of its column in ascending order
__global__ __launch_bounds__(kThreads) void sqdiff_cols_partial_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                       long long n, long long cols,
                                                                       double* __restrict__ part_d,
                                                                       double* __restrict__ part_b) {
  const long long c = static_cast<long long>(blockIdx.x) * kColsPerBlock + (threadIdx.x % kColsPerBlock);
  const long long strands = static_cast<long long>(gridDim.y) * kRowLanes;
  const long long p = static_cast<long long>(blockIdx.y) * kRowLanes + threadIdx.x / kColsPerBlock;
  if (c >= cols) return;
  double sd = 0.0, sb = 0.0;
  for (long long t = p; t < n; t += strands) {
    const double vb = static_cast<double>(b[t * cols + c]);
    const double df = static_cast<double>(a[t * cols + c]) - vb;
    sd += df * df;
    sb += vb * vb;
  }
  part_d[p * cols + c] = sd;
  part_b[p * cols + c] = sb;
}

__global__ __launch_bounds__(kThreads) void sqdiff_cols_sum_kernel(const double* __restrict__ part_d,
                                                                   const double* __restrict__ part_b, long long strands,
                                                                   long long cols, int accumulate,
                                                                   double* __restrict__ out_d, double* __restrict__ out_b) {
  const long long c = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x;
  if (c >= cols) return;
  double sd = 0.0, sb = 0.0;
  for (long long p = 0; p < strands; ++p) {
    sd += part_d[p * cols + c];
    sb += part_b[p * cols + c];
  }
  out_d[c] = accumulate ? out_d[c] + sd : sd;
  out_b[c] = accumulate ? out_b[c] + sb : sb;
}

}  // namespace
}  // namespace mi355q

using namespace mi355q;

extern "C" int32_t mi355q_qfc_quantize_rows_f32(const float* x, int64_t n, int64_t d, int8_t* q_out, float* scale_out,
                                                void* stream) {
  clear_error();
  if (n < 0 || d < 0) return fail(MI355Q_BAD_ARG, "negative shape");
  if (n == 0 || d == 0) return MI355Q_OK;
  if (!x || !q_out || !scale_out) return fail(MI355Q_BAD_ARG, "null pointer");
  if (n > 0x7FFFFFFFLL) return fail(MI355Q_UNSUPPORTED, "more than 2^31 - 1 rows");
  hipStream_t st = as_stream(stream);
  const dim3 grid(static_cast<unsigned>(n)), block(kThreads);
  const bool vec = d % 16 == 0 && d <= kVecMaxD && reinterpret_cast<uintptr_t>(x) % 16 == 0 &&
                   reinterpret_cast<uintptr_t>(q_out) % 16 == 0;
  if (!vec) hipLaunchKernelGGL(quantize_rows_scalar_kernel, grid, block, 0, st, x, static_cast<long long>(d), q_out, scale_out);
  else if (d <= kThreads * 16) hipLaunchKernelGGL(quantize_rows_vec_kernel<1>, grid, block, 0, st, x, static_cast<long long>(d), q_out, scale_out);
  else if (d <= kThreads * 32) hipLaunchKernelGGL(quantize_rows_vec_kernel<2>, grid, block, 0, st, x, static_cast<long long>(d), q_out, scale_out);
  else hipLaunchKernelGGL(quantize_rows_vec_kernel<4>, grid, block, 0, st, x, static_cast<long long>(d), q_out, scale_out);
  MI355Q_CHECK_LAUNCH("row quantizer launch");
  return MI355Q_OK;
}

extern "C" size_t mi355q_qfc_forward_workspace_bytes(int64_t rows, int64_t d, int32_t block) {
  if (rows <= 0 || d <= 0 || block < 0 || (block > 0 && d % block)) return 0;
  return wsum_workspace(rows, block > 0 ? d / block : 1);
}

extern "C" int32_t mi355q_qfc_forward_i8(const int8_t* xq, int64_t n, int64_t d, const float* x_scale,
                                         int64_t x_scale_count, int32_t x_zero_point, const void* w, int32_t w_kind,
                                         int64_t rows, const float* w_scale, int64_t w_scale_count, int32_t block,
                                         float* y_out, int32_t* acc_out, void* workspace, size_t workspace_bytes,
                                         void* stream) {
  clear_error();
  if (n < 0 || d < 0 || rows < 0) return fail(MI355Q_BAD_ARG, "negative shape");
  if (!xq || !x_scale || !w || !w_scale || !y_out) return fail(MI355Q_BAD_ARG, "null pointer");
  if (const int32_t bad = check_weight_kind(w_kind)) return bad;
  if (x_zero_point < -128 || x_zero_point > 127)
    return fail(MI355Q_BAD_ARG, "activation zero point %d is outside int8", x_zero_point);
  if (const int32_t bad = check_block(block, d)) return bad;
  bool blockwise;
  if (const int32_t bad = check_scale_counts(n, rows, d, block, x_scale_count, w_scale_count, acc_out != nullptr, &blockwise))
    return bad;
  if (d > kQfcMaxD)
    return fail(MI355Q_UNSUPPORTED, "d = %lld exceeds %d (the int32 accumulator)", static_cast<long long>(d), kQfcMaxD);
  if (n == 0 || rows == 0) return MI355Q_OK;
  if (d == 0) return fail(MI355Q_BAD_ARG, "d must be >= 1");
  const int64_t nblocks = blockwise ? d / block : 1;
  const size_t need = wsum_workspace(rows, nblocks);
  if (x_zero_point != 0 && (!workspace || workspace_bytes < need))
    return fail(MI355Q_BAD_ARG, "workspace of %zu bytes is smaller than the %zu needed", workspace_bytes, need);
  dim3 grid;
  if (const int32_t bad = tile_grid<int8_t>(n, rows, &grid)) return bad;

  FwdArgs g{};
  g.xq = xq; g.w = static_cast<const uint8_t*>(w); g.x_scale = x_scale; g.w_scale = w_scale;
  g.wsum = static_cast<const int32_t*>(workspace); g.y = y_out; g.acc = acc_out;
  g.n = n; g.rows = rows; g.d = d; g.x_per_row = x_scale_count != 1 ? 1 : 0;
  g.w_mode = blockwise ? 2 : (w_scale_count == rows && rows != 1) ? 1 : 0;
  g.nblocks = static_cast<int>(nblocks);
  g.block = blockwise ? block : static_cast<int>(d);
  g.zp = x_zero_point; g.kind = w_kind;
  hipStream_t st = as_stream(stream);

  if (x_zero_point != 0) {      // (on both routes: the generic kernel subtracts zp * wsum as well)
    const int32_t st_sums = launch_weight_sums(g.w, w_kind, rows * g.nblocks, static_cast<long long>(g.block),
                                               static_cast<int32_t*>(workspace), st);
    if (st_sums != MI355Q_OK) return st_sums;
  }

  if (mfma_route(xq, w, d, blockwise && block == 32 ? 32 : 64))
    dispatch_kind(w_kind, [&](auto kind) { launch_mfma<decltype(kind)::value>(g, blockwise, grid, st); });
  else
    hipLaunchKernelGGL(qfc_generic_kernel, dim3(generic_blocks(n * rows)), dim3(kThreads), 0, st, g);
  MI355Q_CHECK_LAUNCH("integer fully-connected launch");
  return MI355Q_OK;
}

extern "C" size_t mi355q_sqdiff_cols_workspace_bytes(int64_t n, int64_t cols) {
  if (n <= 0 || cols <= 0) return 0;
  return sqdiff_workspace(n, cols);
}

extern "C" int32_t mi355q_sqdiff_cols_f64(const float* a, const float* b, int64_t n, int64_t cols, double* sq_diff_cols,
                                          double* sq_b_cols, int32_t accumulate, void* workspace, size_t workspace_bytes,
                                          void* stream) {
  clear_error();
  if (n < 0 || cols < 0) return fail(MI355Q_BAD_ARG, "negative shape");
  if (cols == 0) return MI355Q_OK;
  if (!sq_diff_cols || !sq_b_cols) return fail(MI355Q_BAD_ARG, "null pointer");
  hipStream_t st = as_stream(stream);
  if (n == 0) {
    if (!accumulate) {
      hipError_t e = hipMemsetAsync(sq_diff_cols, 0, static_cast<size_t>(cols) * sizeof(double), st);
      if (e == hipSuccess) e = hipMemsetAsync(sq_b_cols, 0, static_cast<size_t>(cols) * sizeof(double), st);
      if (e != hipSuccess) return fail(MI355Q_HIP_ERROR, "clearing the column sums: %s", hipGetErrorString(e));
    }
    return MI355Q_OK;
  }
  if (!a || !b) return fail(MI355Q_BAD_ARG, "null pointer");
  const size_t need = sqdiff_workspace(n, cols);
  if (!workspace || workspace_bytes < need)
    return fail(MI355Q_BAD_ARG, "workspace of %zu bytes is smaller than the %zu needed", workspace_bytes, need);
  const int64_t col_blocks = (cols + kColsPerBlock - 1) / kColsPerBlock;
  if (col_blocks > 0x7FFFFFFFLL) return fail(MI355Q_UNSUPPORTED, "too many columns for one launch");
  const int row_blocks = sqdiff_row_blocks(n);
  const long long strands = static_cast<long long>(row_blocks) * kRowLanes;
  double* part_d = static_cast<double*>(workspace);
  double* part_b = part_d + strands * cols;
  hipLaunchKernelGGL(sqdiff_cols_partial_kernel, dim3(static_cast<unsigned>(col_blocks), static_cast<unsigned>(row_blocks)),
                     dim3(kThreads), 0, st, a, b, static_cast<long long>(n), static_cast<long long>(cols), part_d, part_b);
  MI355Q_CHECK_LAUNCH("column squared-difference launch");
  hipLaunchKernelGGL(sqdiff_cols_sum_kernel, dim3(static_cast<unsigned>((cols + kThreads - 1) / kThreads)), dim3(kThreads),
                     0, st, part_d, part_b, strands, static_cast<long long>(cols), accumulate, sq_diff_cols, sq_b_cols);
  MI355Q_CHECK_LAUNCH("column squared-difference sum launch");
  return MI355Q_OK;
}
