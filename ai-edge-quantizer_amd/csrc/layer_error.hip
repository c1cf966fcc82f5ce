// Layer output error of a quantized FULLY_CONNECTED weight on its calibration data.
//
// With H = (2/n) X^T X (what GPTQ calibration keeps per FULLY_CONNECTED input) and dW = W - dequant(W^),
//   (1/n) ||X dW^T||_F^2 = 1/2 tr(dW H dW^T) = 1/2 Sum_r d_r H d_r^T        (d_r = row r of dW)
// so the error a quantized weight leaves in the layer's output over the whole calibration set is one quadratic
// form per output channel; the same form of W is the signal.
//
//   weight_delta_kernel   dW = W - dequant(W^): the target is read in its stored form and dequantized in
//                         registers by the comparison metrics' rule (compare_target.h), without nan_to_num.
//   quadform_kernel       out_r = alpha a_r Psym a_r^T against the LOWER triangle of a float32 product
//                         (HessianAccumulator.product_form(): only j <= i is valid, and it must not be
//                         modified). C = a L' on the FP32 matrix cores (v_mfma_f32_32x32x2_f32) over tiles of
//                         128 rows x 128 columns j0, with
//                           L'[k][j] = 2 P[k][j] (k > j),  P[j][j] (k = j),  0 (k < j)
//                         so the K loop of a column tile runs over k >= j0 only, strictly-lower products are
//                         counted twice (the doubling is exact) and diagonal ones once; there is no
//                         2*lower - diagonal subtraction. Only the K steps that cross the diagonal (k0 < j0 + 128)
//                         look at the mask, and what the mask rejects is not loaded: an entry above the diagonal
//                         is never read. The epilogue multiplies the accumulator tile by the `a` tile (float32
//                         products are exact in float64), sums each row's 64 columns of a wave in float64 and
//                         writes partials[column tile][row].
//   quadform_sum_kernel   adds a row's partials in index order and scales by alpha: the same bits in every run,
//                         no floating-point atomics, no rows x d intermediate.
// Tiling and staging follow gemm_kernel of csrc/gemm.hip (global -> registers one K step ahead, two LDS buffers,
// operand fragments double-buffered in registers).
#include "common.h"
#include "compare_target.h"

namespace mi355q {
namespace {

constexpr int kThreads = 256;
constexpr int BM = 128;          // block tile edge = 2 waves x TM x MF (rows and columns)
constexpr int BK = 16;           // k per LDS stage
constexpr int MF = 32;           // MFMA tile edge
constexpr int KF = 2;            // k per MFMA
constexpr int TM = 2;            // MFMA tiles per wave along rows and along columns
constexpr int LD = BM + 4;       // keeps every LDS row 16-byte aligned, breaks the power-of-2 stride
constexpr int NL = BM * BK / 4 / kThreads;   // 16-byte pieces per thread per operand tile
constexpr int kColTile = TM * MF;            // columns per partial sum (one wave's share of the block tile)
static_assert(NL * 4 * kThreads == BM * BK, "whole 16-byte pieces per thread");

using Acc = __attribute__((ext_vector_type(16))) float;
struct __attribute__((aligned(16))) F4 { float x, y, z, w; };

// ---------------------------------------------------------------- dW = W - dequant(W^)
__global__ __launch_bounds__(kThreads) void weight_delta_kernel(mi355q_compare_pair p, float* __restrict__ out) {
  const int64_t step = static_cast<int64_t>(gridDim.x) * kThreads;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; e < p.n; e += step)
    out[e] = p.reference[e] - load_target(p, e);
}

// ---------------------------------------------------------------- out_r = alpha a_r Psym a_r^T
struct QuadArgs {
  const float* a;        // [rows, d]
  const float* p;        // [d, d], lower triangle valid
  long long rows, d;
  int a_vec, p_vec;      // 16-byte loads allowed (base aligned, d % 4 == 0)
  double* partials;      // [ceil(d / kColTile)][rows]
};

__device__ __forceinline__ float comp(const F4& v, int c) { return c == 0 ? v.x : c == 1 ? v.y : c == 2 ? v.z : v.w; }

// `a` tile: rows i0 .. i0+127 x k0 .. k0+15, k contiguous in memory. Piece e = (row e / 4, k (e % 4) * 4 .. + 3).
__device__ __forceinline__ void load_a(F4 (&st)[NL], const QuadArgs& g, long long i0, long long k0, int tid) {
  const bool whole = g.a_vec && i0 + BM <= g.rows && k0 + BK <= g.d;
#pragma unroll
  for (int l = 0; l < NL; ++l) {
    const int e = tid + kThreads * l, kv = e % (BK / 4), m = e / (BK / 4);
    const long long row = i0 + m, k = k0 + kv * 4;
    if (whole) {
      st[l] = *reinterpret_cast<const F4*>(g.a + row * g.d + k);
    } else {
      float t[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) t[c] = (row < g.rows && k + c < g.d) ? g.a[row * g.d + k + c] : 0.f;
      st[l] = F4{t[0], t[1], t[2], t[3]};
    }
  }
}

__device__ __forceinline__ void store_a(const F4 (&st)[NL], float (*lds)[LD], int tid) {
#pragma unroll
  for (int l = 0; l < NL; ++l) {
    const int e = tid + kThreads * l, kv = e % (BK / 4), m = e / (BK / 4);
#pragma unroll
    for (int c = 0; c < 4; ++c) lds[kv * 4 + c][m] = comp(st[l], c);
  }
}

// L' tile: columns j0 .. j0+127 x k0 .. k0+15, j contiguous in memory (P[k][j]). Piece e = (k e / 32, j (e % 32) * 4 .. + 3).
// Below the diagonal tiles (k0 >= j0 + 128) every entry is strictly lower: 2 P. On the tiles that cross the diagonal an
// entry with k < j is zero WITHOUT being loaded.
__device__ __forceinline__ void load_p(F4 (&st)[NL], const QuadArgs& g, long long j0, long long k0, int tid) {
  const bool below = k0 >= j0 + BM;
  const bool whole = g.p_vec && below && j0 + BM <= g.d && k0 + BK <= g.d;
#pragma unroll
  for (int l = 0; l < NL; ++l) {
    const int e = tid + kThreads * l, jv = e % (BM / 4), kk = e / (BM / 4);
    const long long j = j0 + jv * 4, k = k0 + kk;
    if (whole || (g.p_vec && k < g.d && j + 3 < g.d && k > j + 3)) {
      const F4 v = *reinterpret_cast<const F4*>(g.p + k * g.d + j);
      st[l] = F4{2.f * v.x, 2.f * v.y, 2.f * v.z, 2.f * v.w};
    } else {
      float t[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const long long jc = j + c;
        float v = 0.f;
        if (k < g.d && jc < g.d && jc <= k) {
          v = g.p[k * g.d + jc];
          if (jc < k) v = 2.f * v;
        }
        t[c] = v;
      }
      st[l] = F4{t[0], t[1], t[2], t[3]};
    }
  }
}

__device__ __forceinline__ void store_p(const F4 (&st)[NL], float (*lds)[LD], int tid) {
#pragma unroll
  for (int l = 0; l < NL; ++l) {
    const int e = tid + kThreads * l, jv = e % (BM / 4), kk = e / (BM / 4);
    *reinterpret_cast<F4*>(&lds[kk][jv * 4]) = st[l];
  }
}

// row of accumulator register `reg` for this lane (C/D layout of the 32x32 MFMAs; the column is lane % 32)
__device__ __forceinline__ int acc_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }

// grid: x = row tiles (neighbouring blocks share the L' tiles of one column tile), y = column tiles, the longest K
// ranges (j0 = 0) first.
__global__ __launch_bounds__(kThreads) void quadform_kernel(QuadArgs g) {
  __shared__ __attribute__((aligned(16))) float As[2][BK][LD];
  __shared__ __attribute__((aligned(16))) float Ps[2][BK][LD];
  const long long i0 = static_cast<long long>(blockIdx.x) * BM, j0 = static_cast<long long>(blockIdx.y) * BM;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wi = (wave >> 1) * (TM * MF), wj = (wave & 1) * (TM * MF);
  const int fi = lane % MF, fk = lane / MF;

  Acc acc[TM][TM];
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TM; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  const long long k_begin = j0, k_end = g.d;   // j0 < d for every block of the grid
  F4 sa[NL], sp[NL];
  load_a(sa, g, i0, k_begin, tid);
  load_p(sp, g, j0, k_begin, tid);
  store_a(sa, As[0], tid);
  store_p(sp, Ps[0], tid);
  __syncthreads();
  int buf = 0;
  for (long long k0 = k_begin; k0 < k_end; k0 += BK) {
    const long long kn = k0 + BK;
    const bool more = kn < k_end;
    if (more) {  // the next tile's global loads fly while this tile's MFMAs run
      load_a(sa, g, i0, kn, tid);
      load_p(sp, g, j0, kn, tid);
    }
    float af[2][TM], pf[2][TM];
#pragma unroll
    for (int t = 0; t < TM; ++t) {
      af[0][t] = As[buf][fk][wi + t * MF + fi];
      pf[0][t] = Ps[buf][fk][wj + t * MF + fi];
    }
#pragma unroll
    for (int s = 0; s < BK / KF; ++s) {
      const int cur = s & 1;
      if (s + 1 < BK / KF) {
#pragma unroll
        for (int t = 0; t < TM; ++t) {
          af[cur ^ 1][t] = As[buf][(s + 1) * KF + fk][wi + t * MF + fi];
          pf[cur ^ 1][t] = Ps[buf][(s + 1) * KF + fk][wj + t * MF + fi];
        }
      }
#pragma unroll
      for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TM; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[cur][a], pf[cur][b], acc[a][b], 0, 0, 0);
    }
    if (more) {
      store_a(sa, As[buf ^ 1], tid);
      store_p(sp, Ps[buf ^ 1], tid);
    }
    __syncthreads();
    buf ^= 1;
  }

  // ---- epilogue: partials[column tile][row] = Sum_j C[row][j] a[row][j] over the wave's 64 columns, float64
  const long long jw = j0 + wj;
  if (jw >= g.d) return;   // (the whole wave: its columns lie past the matrix)
  double* part = g.partials + (jw / kColTile) * g.rows;
#pragma unroll
  for (int a = 0; a < TM; ++a) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const long long row = i0 + wi + a * MF + acc_row(r, lane);
      double s = 0.0;
#pragma unroll
      for (int b = 0; b < TM; ++b) {
        const long long col = jw + b * MF + fi;
        if (row < g.rows && col < g.d) s += static_cast<double>(acc[a][b][r]) * static_cast<double>(g.a[row * g.d + col]);
      }
#pragma unroll
      for (int off = 1; off < MF; off <<= 1) s += __shfl_xor(s, off, kWave);   // the 32 lanes that share the row
      if (fi == 0 && row < g.rows) part[row] = s;
    }
  }
}

__global__ __launch_bounds__(kThreads) void quadform_sum_kernel(const double* __restrict__ partials, long long rows,
                                                                long long tiles, double alpha,
                                                                double* __restrict__ out) {
  const long long row = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x;
  if (row >= rows) return;
  double s = 0.0;
  for (long long t = 0; t < tiles; ++t) s += partials[t * rows + row];
  out[row] = alpha * s;
}

size_t quad_workspace(int64_t rows, int64_t d) {
  const size_t tiles = static_cast<size_t>((d + kColTile - 1) / kColTile);
  return (static_cast<size_t>(rows) * tiles * sizeof(double) + 255) & ~static_cast<size_t>(255);
}

}  // namespace
}  // namespace mi355q

using namespace mi355q;

extern "C" int32_t mi355q_weight_delta_f32(const float* reference, const void* target, int64_t n, int32_t target_kind,
                                           int32_t diff_bits, int64_t channels, int64_t inner, const float* scale,
                                           const int32_t* zero_point, float* delta_out, void* stream) {
  clear_error();
  if (n < 0) return fail(MI355Q_BAD_ARG, "negative element count");
  if (n == 0) return MI355Q_OK;
  if (!reference || !target || !delta_out) return fail(MI355Q_BAD_ARG, "null pointer");
  if (target_kind < MI355Q_CMP_F32 || target_kind > MI355Q_CMP_I2)
    return fail(MI355Q_BAD_ARG, "unknown target kind %d", target_kind);
  if (target_kind >= MI355Q_CMP_I8) {
    if (!scale) return fail(MI355Q_BAD_ARG, "integer target without scales");
    if (channels < 1 || inner < 1) return fail(MI355Q_BAD_ARG, "channels and inner must be >= 1");
    if (diff_bits != 8 && diff_bits != 16 && diff_bits != 32)
      return fail(MI355Q_BAD_ARG, "diff_bits must be 8, 16 or 32");
  }
  mi355q_compare_pair p{};
  p.reference = reference; p.target = target; p.n = n; p.target_kind = target_kind; p.diff_bits = diff_bits;
  p.channels = channels; p.inner = inner; p.scale = scale; p.zero_point = zero_point;
  const int64_t blocks = (n + kThreads - 1) / kThreads;
  const unsigned grid = static_cast<unsigned>(blocks < (1 << 20) ? blocks : (1 << 20));
  hipLaunchKernelGGL(weight_delta_kernel, dim3(grid), dim3(kThreads), 0, as_stream(stream), p, delta_out);
  MI355Q_CHECK_LAUNCH("weight delta launch");
  return MI355Q_OK;
}

extern "C" size_t mi355q_quadform_rows_workspace_bytes(int64_t rows, int64_t d) {
  if (rows <= 0 || d <= 0) return 0;
  return quad_workspace(rows, d);
}

extern "C" int32_t mi355q_quadform_rows_f32(const float* a, int64_t rows, int64_t d, const float* product,
                                            double alpha, double* out_rows, void* workspace, size_t workspace_bytes,
                                            void* stream) {
  clear_error();
  if (rows < 0 || d < 0) return fail(MI355Q_BAD_ARG, "negative shape");
  if (rows == 0) return MI355Q_OK;
  if (d < 1) return fail(MI355Q_BAD_ARG, "d must be >= 1");
  if (!a || !product || !out_rows) return fail(MI355Q_BAD_ARG, "null pointer");
  const int64_t row_tiles = (rows + BM - 1) / BM, col_tiles = (d + BM - 1) / BM;
  if (col_tiles > 65535 || row_tiles > 0x7FFFFFFFLL) return fail(MI355Q_BAD_SHAPE, "too many tiles for one launch");
  const size_t need = quad_workspace(rows, d);
  if (!workspace || workspace_bytes < need)
    return fail(MI355Q_BAD_ARG, "workspace of %zu bytes is smaller than the %zu needed", workspace_bytes, need);
  QuadArgs g{};
  g.a = a; g.p = product; g.rows = rows; g.d = d;
  g.a_vec = d % 4 == 0 && reinterpret_cast<uintptr_t>(a) % 16 == 0;
  g.p_vec = d % 4 == 0 && reinterpret_cast<uintptr_t>(product) % 16 == 0;
  g.partials = static_cast<double*>(workspace);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(quadform_kernel, dim3(static_cast<unsigned>(row_tiles), static_cast<unsigned>(col_tiles)),
                     dim3(kThreads), 0, st, g);
  MI355Q_CHECK_LAUNCH("quadratic form launch");
  hipLaunchKernelGGL(quadform_sum_kernel, dim3(static_cast<unsigned>((rows + kThreads - 1) / kThreads)),
                     dim3(kThreads), 0, st, g.partials, static_cast<long long>(rows),
                     static_cast<long long>((d + kColTile - 1) / kColTile), alpha, out_rows);
  MI355Q_CHECK_LAUNCH("quadratic form sum launch");
  return MI355Q_OK;
}
