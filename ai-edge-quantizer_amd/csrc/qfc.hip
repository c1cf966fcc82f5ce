// Integer execution of a quantized FULLY_CONNECTED op on calibration data (include/mi355q.h, "Integer execution").
//
//   quantize_rows_*_kernel  the dynamic-range activation quantizer: per row t, range = max |x|, s_x = range / 127,
//                           q = clamp(round_half_away_from_zero(fl(x * (127 / range))), -127, 127). The vector route
//                           keeps the row in registers between the maximum and the rounding (one read of x), 16 floats
//                           per lane and chunk, and stores 16 int8 at once; the scalar route reads the row twice.
//   weight_sums_kernel      wsum[r][b] = Sum_k q_w[r][b * L + k] (int32, exact), the zero-point term of the accumulator
//                           (qfc_frag.h, with the weight fragments: qfc16.hip uses both as well).
//   qfc_mfma_kernel         acc = Xq W^^T on the int8 matrix cores. Both operands are contiguous along the reduction
//                           dimension, so a lane's A fragment is 16 consecutive bytes of a row of Xq and its B fragment
//                           16 consecutive elements of a row of W^ (8 bytes of int4, 4 bytes of int2, unpacked and
//                           sign-extended in registers). A wave owns 64 tokens x 64 output channels = 4 x 4 MFMA tiles:
//                           4 + 4 fragments feed 16 v_mfma_i32_16x16x64_i8, the next step's fragments are in flight
//                           while they run, and the four waves of a workgroup (128 x 128) share rows through L1 / L2.
//                           Block 32 uses v_mfma_i32_16x16x32_i8 (8 bytes per lane). Blockwise scales flush the int32
//                           tile into float32 sums after every block, in ascending order, without FMA.
//   qfc_generic_kernel      one thread per output, element by element: every other shape and alignment, same bits.
//   sqdiff_cols_*_kernel    per column Sum_t (a - b)^2 and Sum_t b^2 in float64 in a fixed order.
#include "common.h"
#include "compare_target.h"
#include "qfc_frag.h"

namespace mi355q {
namespace {

constexpr int kThreads = kQfcThreads;
constexpr int kMaxD = 65536;           // d * 255 * 128 < 2^31
constexpr int kVecMaxD = 16384;        // a row of the vector quantizer: 256 threads x 4 chunks x 16 floats

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

template <int KSTEP> struct XFrag;
template <> struct XFrag<64> {
  static __device__ __forceinline__ I32x4 load(const int8_t* p) { return *reinterpret_cast<const I32x4*>(p); }
  static __device__ __forceinline__ I32x4 zero() { return I32x4{0, 0, 0, 0}; }
  static __device__ __forceinline__ I32x4 mfma(I32x4 a, I32x4 b, I32x4 c) {
    return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0);
  }
};
template <> struct XFrag<32> {
  static __device__ __forceinline__ long load(const int8_t* p) { return *reinterpret_cast<const long*>(p); }
  static __device__ __forceinline__ long zero() { return 0; }
  static __device__ __forceinline__ I32x4 mfma(long a, long b, I32x4 c) {
    return __builtin_amdgcn_mfma_i32_16x16x32_i8(a, b, c, 0, 0, 0);
  }
};

constexpr int MF = 16;             // MFMA tile edge
constexpr int TM = 4;              // MFMA tiles per wave along tokens and along output channels
constexpr int WT = TM * MF;        // a wave's tile edge (64)
constexpr int BT = 2 * WT;         // a workgroup's tile edge (2 x 2 waves)

// MFMA route: d % KSTEP == 0, xq and w 16-byte aligned (so every fragment load is aligned to its own size).
// grid: x = output-channel tiles, y = token tiles.
template <int KIND, int KSTEP, bool BLOCKWISE>
__global__ __launch_bounds__(kThreads) void qfc_mfma_kernel(FwdArgs g) {
  using XF = XFrag<KSTEP>;
  using RW = RawW<KIND, KSTEP>;
  using Frag = typename FragOf<KSTEP>::T;
  constexpr int E = KSTEP / 4;     // consecutive elements per lane and step
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const long long t0 = static_cast<long long>(blockIdx.y) * BT + (wave >> 1) * WT;
  const long long r0 = static_cast<long long>(blockIdx.x) * BT + (wave & 1) * WT;
  if (t0 >= g.n || r0 >= g.rows) return;     // (the whole wave; the kernel has no barrier)
  const int fr = lane & 15, fg = lane >> 4;

  const int8_t* xp[TM];
  long long we[TM];
  bool xok[TM], wok[TM];
#pragma unroll
  for (int a = 0; a < TM; ++a) {
    const long long t = t0 + a * MF + fr, r = r0 + a * MF + fr;
    xok[a] = t < g.n;
    wok[a] = r < g.rows;
    xp[a] = g.xq + (xok[a] ? t : 0) * g.d + fg * E;
    we[a] = (wok[a] ? r : 0) * g.d + fg * E;
  }

  I32x4 acc[TM][TM];
  float yf[TM][TM][4];
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TM; ++b) {
      acc[a][b] = I32x4{0, 0, 0, 0};
#pragma unroll
      for (int i = 0; i < 4; ++i) yf[a][b][i] = 0.0f;
    }
  float sx[TM][4];
  if (BLOCKWISE) {
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long long t = t0 + a * MF + fg * 4 + i;
        sx[a][i] = t < g.n ? g.x_scale[g.x_per_row ? t : 0] : 0.0f;
      }
  }

  const int steps = static_cast<int>(g.d / KSTEP);
  const int steps_per_block = BLOCKWISE ? g.block / KSTEP : steps;
  Frag xc[TM], xn[TM];
  typename RW::T wc[TM], wn[TM];
#pragma unroll
  for (int a = 0; a < TM; ++a) {
    xc[a] = xok[a] ? XF::load(xp[a]) : XF::zero();
    wc[a] = wok[a] ? RW::load(g.w, we[a]) : RW::zero();
  }
  int in_block = 0, bi = 0;
  for (int s = 0; s < steps; ++s) {
    if (s + 1 < steps) {     // the next step's fragments fly while this step's MFMAs run
      const long long k = static_cast<long long>(s + 1) * KSTEP;
#pragma unroll
      for (int a = 0; a < TM; ++a) {
        xn[a] = xok[a] ? XF::load(xp[a] + k) : XF::zero();
        wn[a] = wok[a] ? RW::load(g.w, we[a] + k) : RW::zero();
      }
    }
    Frag wf[TM];
#pragma unroll
    for (int b = 0; b < TM; ++b) wf[b] = RW::unpack(wc[b]);
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
      for (int b = 0; b < TM; ++b) acc[a][b] = XF::mfma(xc[a], wf[b], acc[a][b]);
#pragma unroll
    for (int a = 0; a < TM; ++a) {
      xc[a] = xn[a];
      wc[a] = wn[a];
    }
    if (BLOCKWISE && ++in_block == steps_per_block) {
      // p_b = fl(float(acc_b) * fl(s_x * s_w[r, b])), y = y + p_b: blocks in ascending order, no FMA
#pragma unroll
      for (int b = 0; b < TM; ++b) {
        const long long r = r0 + b * MF + fr;
        const bool rok = r < g.rows;
        const float sw = rok ? g.w_scale[r * g.nblocks + bi] : 0.0f;
        const int corr = (rok && g.zp != 0) ? g.zp * g.wsum[r * g.nblocks + bi] : 0;
#pragma unroll
        for (int a = 0; a < TM; ++a)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float sc = sx[a][i] * sw;
            const float p = static_cast<float>(acc[a][b][i] - corr) * sc;
            yf[a][b][i] = yf[a][b][i] + p;
            acc[a][b][i] = 0;
          }
      }
      in_block = 0;
      ++bi;
    }
  }

  // C / D map of the 16x16 MFMAs: column (output channel) = lane & 15, row (token) = 4 (lane >> 4) + register
#pragma unroll
  for (int b = 0; b < TM; ++b) {
    const long long r = r0 + b * MF + fr;
    if (r >= g.rows) continue;
    float sw = 0.0f;
    int corr = 0;
    if (!BLOCKWISE) {
      sw = g.w_scale[g.w_mode == 1 ? r : 0];
      corr = g.zp != 0 ? g.zp * g.wsum[r] : 0;
    }
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long long t = t0 + a * MF + fg * 4 + i;
        if (t >= g.n) continue;
        if (BLOCKWISE) {
          g.y[t * g.rows + r] = yf[a][b][i];
        } else {
          const int v = acc[a][b][i] - corr;
          const float sc = g.x_scale[g.x_per_row ? t : 0] * sw;
          g.y[t * g.rows + r] = static_cast<float>(v) * sc;
          if (g.acc) g.acc[t * g.rows + r] = v;
        }
      }
  }
}

// Generic route: one thread per output element, one weight element at a time.
__global__ __launch_bounds__(kThreads) void qfc_generic_kernel(FwdArgs g) {
  const long long total = g.n * g.rows, step = static_cast<long long>(gridDim.x) * kThreads;
  for (long long o = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; o < total; o += step) {
    const long long t = o / g.rows, r = o % g.rows;
    const int8_t* xr = g.xq + t * g.d;
    const float s_x = g.x_scale[g.x_per_row ? t : 0];
    float y = 0.0f;
    for (int b = 0; b < g.nblocks; ++b) {
      int acc = 0;
      const long long k0 = static_cast<long long>(b) * g.block;
      for (long long k = k0; k < k0 + g.block; ++k)
        acc += static_cast<int>(xr[k]) * weight_element(g.w, g.kind, r * g.d + k);
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

size_t fwd_workspace(int64_t rows, int64_t d, int32_t block) {
  const size_t nblocks = block > 0 ? static_cast<size_t>(d / block) : 1;
  return (static_cast<size_t>(rows) * nblocks * sizeof(int32_t) + 255) & ~static_cast<size_t>(255);
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
  return fwd_workspace(rows, d, block);
}

extern "C" int32_t mi355q_qfc_forward_i8(const int8_t* xq, int64_t n, int64_t d, const float* x_scale,
                                         int64_t x_scale_count, int32_t x_zero_point, const void* w, int32_t w_kind,
                                         int64_t rows, const float* w_scale, int64_t w_scale_count, int32_t block,
                                         float* y_out, int32_t* acc_out, void* workspace, size_t workspace_bytes,
                                         void* stream) {
  clear_error();
  if (n < 0 || d < 0 || rows < 0) return fail(MI355Q_BAD_ARG, "negative shape");
  if (!xq || !x_scale || !w || !w_scale || !y_out) return fail(MI355Q_BAD_ARG, "null pointer");
  if (w_kind != MI355Q_CMP_I8 && w_kind != MI355Q_CMP_I4 && w_kind != MI355Q_CMP_I2)
    return fail(MI355Q_BAD_ARG, "weight kind %d is not I8, I4 or I2", w_kind);
  if (x_zero_point < -128 || x_zero_point > 127)
    return fail(MI355Q_BAD_ARG, "activation zero point %d is outside int8", x_zero_point);
  if (block != 0 && block != 32 && block != 64 && block != 128 && block != 256)
    return fail(MI355Q_BAD_ARG, "block must be 0, 32, 64, 128 or 256 (got %d)", block);
  if (block > 0 && d % block)
    return fail(MI355Q_BAD_SHAPE, "Quantized dimension %lld is not divisible by block size %d.",
                static_cast<long long>(d), block);
  if (x_scale_count != 1 && x_scale_count != n)
    return fail(MI355Q_BAD_ARG, "x_scale_count must be 1 or n = %lld (got %lld)", static_cast<long long>(n),
                static_cast<long long>(x_scale_count));
  const int64_t nblocks = block > 0 ? d / block : 1;
  const bool blockwise = block > 0 && w_scale_count == rows * nblocks;   // (block = 0 with per-tensor / per-channel scales)
  if (!blockwise && w_scale_count != 1 && w_scale_count != rows)
    return fail(MI355Q_BAD_ARG, "w_scale_count must be 1, rows = %lld or rows * d / block (got %lld)",
                static_cast<long long>(rows), static_cast<long long>(w_scale_count));
  if (blockwise && acc_out) return fail(MI355Q_BAD_ARG, "acc_out is not available with blockwise scales");
  if (d > kMaxD) return fail(MI355Q_UNSUPPORTED, "d = %lld exceeds %d (the int32 accumulator)", static_cast<long long>(d), kMaxD);
  if (n == 0 || rows == 0) return MI355Q_OK;
  if (d == 0) return fail(MI355Q_BAD_ARG, "d must be >= 1");
  const size_t need = fwd_workspace(rows, d, blockwise ? block : 0);
  if (x_zero_point != 0 && (!workspace || workspace_bytes < need))
    return fail(MI355Q_BAD_ARG, "workspace of %zu bytes is smaller than the %zu needed", workspace_bytes, need);
  const int64_t row_tiles = (rows + BT - 1) / BT, tok_tiles = (n + BT - 1) / BT;
  if (row_tiles > 0x7FFFFFFFLL || tok_tiles > 65535) return fail(MI355Q_UNSUPPORTED, "too many tiles for one launch");

  FwdArgs g{};
  g.xq = xq; g.w = static_cast<const uint8_t*>(w); g.x_scale = x_scale; g.w_scale = w_scale;
  g.wsum = static_cast<const int32_t*>(workspace); g.y = y_out; g.acc = acc_out;
  g.n = n; g.rows = rows; g.d = d; g.x_per_row = x_scale_count != 1 ? 1 : 0;
  g.w_mode = blockwise ? 2 : (w_scale_count == rows && rows != 1) ? 1 : 0;
  g.nblocks = blockwise ? static_cast<int>(nblocks) : 1;
  g.block = blockwise ? block : static_cast<int>(d);
  g.zp = x_zero_point; g.kind = w_kind;
  hipStream_t st = as_stream(stream);

  if (x_zero_point != 0) {
    const int32_t st_sums = launch_weight_sums(g.w, w_kind, rows * g.nblocks, static_cast<long long>(g.block),
                                               static_cast<int32_t*>(workspace), st);
    if (st_sums != MI355Q_OK) return st_sums;
  }

  const int kstep = blockwise && block == 32 ? 32 : 64;
  const bool mfma = d % kstep == 0 && reinterpret_cast<uintptr_t>(xq) % 16 == 0 && reinterpret_cast<uintptr_t>(w) % 16 == 0;
  if (mfma) {
    const dim3 grid(static_cast<unsigned>(row_tiles), static_cast<unsigned>(tok_tiles));
    if (w_kind == MI355Q_CMP_I8) launch_mfma<MI355Q_CMP_I8>(g, blockwise, grid, st);
    else if (w_kind == MI355Q_CMP_I4) launch_mfma<MI355Q_CMP_I4>(g, blockwise, grid, st);
    else launch_mfma<MI355Q_CMP_I2>(g, blockwise, grid, st);
  } else {
    const long long total = n * rows, blocks = (total + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(qfc_generic_kernel, dim3(static_cast<unsigned>(blocks < (1 << 20) ? blocks : (1 << 20))),
                       dim3(kThreads), 0, st, g);
  }
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
