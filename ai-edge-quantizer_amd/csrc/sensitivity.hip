// Sensitivity sweep: the weight deltas of SEVERAL candidate configurations from one read of the weight.
//
// Candidate k is the symmetric min/max fake-quantization of x [rows, cols] with bits[k] in {2, 4, 8} and block[k] in
// {0 (one scale per row), 32, 64, 128, 256}; what leaves is
//   delta_k[e] = x[e] - fl(float(q_k[e]) * s_k)
// with q_k and s_k the integers and scales of mi355q_requant_sym_f32 (csrc/requant.hip) bit for bit: the same
// make_scale, the same quant4 / quant_sym, then the float32 product rounded once and a float32 subtraction, which is
// what mi355q_weight_delta_f32 does with an int8 target and diff_bits 8. No integers and no scales are stored.
// Optionally sq[k][row] = Sum_c double(delta)^2, added in a fixed order (lane partials over ascending pieces, a
// wave butterfly, the waves' partials in index order): the same bits in every run, no floating-point atomics.
//
//   delta_sweep_rows_kernel     the vector route (cols % 4 == 0, 16-byte aligned x / delta, cols <= 16384). A row is
//                               held by TPR threads as R 16-byte pieces, lane i owning pieces i + TPR j, as in
//                               requant_rows_kernel: x is read from HBM ONCE and stays in registers for every
//                               candidate. The |x|-max butterfly runs once per piece register and keeps what it
//                               passes through: after the exchanges over 1, 2, 4 lanes the maximum of 8 adjacent
//                               lanes is the block-32 maximum of the piece's block (a block of B columns is B / 4
//                               adjacent pieces, and TPR is a multiple of that), after 8 / 16 / 32 the block-64 /
//                               128 / 256 one; the wave's (TPR = 64) or the workgroup's (TPR = 256, one LDS
//                               exchange) maximum is the row's. The candidate loop runs over the wave-uniform
//                               (bits, block) of the kernel arguments and dispatches to the three quant4
//                               instantiations; every delta piece leaves as one non-temporal 16-byte store (the
//                               stream is written once and never read here). 4 + 4 count bytes per element.
//   delta_sweep_generic_kernel  every other shape (cols % 4 != 0, misaligned pointers, cols > 16384), the same bits
//                               from scalar accesses: one workgroup per row, a pass for the row maximum and one more
//                               pass over x per candidate (a wave per block for the blockwise ones). The one-read
//                               property holds for the vector route only.
#include "requant_kernels.h"

namespace mi355q {
namespace {

using namespace requant;

constexpr int kMaxCandidates = 8;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;

struct SweepArgs {
  const float* x;
  float* delta;            // candidate k at delta + k * delta_stride
  int64_t delta_stride;
  double* sq;              // null, or [count][rows]
  int64_t rows, cols;
  int32_t count;
  int32_t bits[kMaxCandidates];     // the candidate tables travel with the dispatch packet: scalar loads
  int32_t block[kMaxCandidates];
};

// The integer-valued quantization does not depend on how the quotient is formed (requant_kernels.h: the reciprocal
// route is exact), so each class takes what mi355q_requant_sym_f32 takes for it: IEEE divisions for rows, one
// division per block for the sub-byte blockwise candidates.
template <int BITS, bool BLOCKWISE> constexpr bool kFast = BLOCKWISE && BITS < 8;

__device__ __forceinline__ uint32_t max_xor(uint32_t v, int off) {
  const uint32_t o = static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), off, kWave));
  return o > v ? o : v;
}

__device__ __forceinline__ double wave_sum(double s) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, kWave);
  return s;
}

// x - fl(float(q) * s): the product rounded to float32 once (the build passes -ffp-contract=off), then subtracted.
// The product is made opaque before the subtraction: the compiler otherwise folds the negation into the product,
// x + (-float(q)) * s, which is the same number but not the same NaN: under a NaN scale mi355q_weight_delta_f32's
// subtraction hands back the NaN with its sign flipped, and the sweep has to give that composition's bits.
__device__ __forceinline__ float delta_of(float x, int q, float s) {
  float p = static_cast<float>(q) * s;
  asm volatile("" : "+v"(p));
  return x - p;
}

__device__ __forceinline__ double sq4(float a, float b, float c, float d) {
  const double e0 = a, e1 = b, e2 = c, e3 = d;
  return ((e0 * e0 + e1 * e1) + e2 * e2) + e3 * e3;      // (a float32 squared is exact in float64)
}

// One 16-byte piece of one candidate: quantize, multiply back, subtract, store; returns the piece's sum of squares.
template <int BITS, bool FAST>
__device__ __forceinline__ double delta_piece(float4 v, float s, float r, float* dst) {
  const Quant4<BITS> o = quant4<BITS, FAST>(v, s, r);
  const float d0 = delta_of(v.x, o.a, s), d1 = delta_of(v.y, o.b, s);
  const float d2 = delta_of(v.z, o.c, s), d3 = delta_of(v.w, o.d, s);
  store4<true>(reinterpret_cast<uint32_t*>(dst), f2u(d0), f2u(d1), f2u(d2), f2u(d3));
  return sq4(d0, d1, d2, d3);
}

// One candidate over the lane's pieces of a row. `mb[j]` is the maximum of piece j's block (blockwise candidates),
// `mrow` the row's.
template <int BITS, bool BLOCKWISE, int TPR, int R>
__device__ __forceinline__ double candidate_pieces(const float4 (&v)[R], const uint32_t (&mb)[R], uint32_t mrow,
                                                   float* dst_row, int lane, int cols4) {
  constexpr bool FAST = kFast<BITS, BLOCKWISE>;
  uint16_t hb;
  double acc = 0.0;
  float s = 0.f, r = 0.f;
  if constexpr (!BLOCKWISE) {
    s = make_scale<BITS, false>(mrow, nullptr, 0, &hb);
    r = FAST ? 1.0f / s : 0.f;
  }
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const int c = j * TPR + lane;
    if (c < cols4) {
      if constexpr (BLOCKWISE) {
        s = make_scale<BITS, true>(mb[j], nullptr, 0, &hb);
        r = FAST ? 1.0f / s : 0.f;
      }
      acc += delta_piece<BITS, FAST>(v[j], s, r, dst_row + 4 * static_cast<int64_t>(c));
    }
  }
  return acc;
}

template <int TPR, int R>
__global__ __launch_bounds__(kThreads) void delta_sweep_rows_kernel(SweepArgs a) {
  static_assert(TPR == kWave || TPR == kThreads, "a wave or the whole workgroup owns a row");
  constexpr int RPB = kThreads / TPR;  // rows per block
  const int lane = threadIdx.x % TPR;
  const int64_t row = static_cast<int64_t>(blockIdx.x) * RPB + threadIdx.x / TPR;
  const int cols4 = static_cast<int>(a.cols / 4);
  const bool live = row < a.rows;      // (TPR = 256: one row per block, always live)
  const float4* __restrict__ x4 = reinterpret_cast<const float4*>(a.x) + row * cols4;

  float4 v[R];
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const int c = j * TPR + lane;
    v[j] = (live && c < cols4) ? load4<true>(x4 + c) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  // the butterfly, once: the maxima of 8 / 16 / 32 / 64 adjacent lanes on the way
  uint32_t m8[R], m16[R], m32[R], m64[R];
  uint32_t mrow = 0;
#pragma unroll
  for (int j = 0; j < R; ++j) {
    uint32_t m = absmax4(v[j]);
    m = max_xor(max_xor(max_xor(m, 1), 2), 4);
    m8[j] = m;
    m16[j] = m = max_xor(m, 8);
    m32[j] = m = max_xor(m, 16);
    m64[j] = m = max_xor(m, 32);
    mrow = m > mrow ? m : mrow;
  }
  if constexpr (TPR > kWave) {
    __shared__ uint32_t part[kWaves];
    if ((threadIdx.x & (kWave - 1)) == 0) part[threadIdx.x / kWave] = mrow;
    __syncthreads();
    mrow = max(max(part[0], part[1]), max(part[2], part[3]));
  } else {
    if (!live) return;      // (no workgroup barrier on this route)
  }

  __shared__ double sums[kMaxCandidates][kWaves];
  for (int k = 0; k < a.count; ++k) {
    const int bits = a.bits[k], block = a.block[k];
    float* dst_row = a.delta + static_cast<int64_t>(k) * a.delta_stride + row * a.cols;
    // The maxima a candidate reads are made opaque per iteration: what a channelwise candidate computes depends on
    // (bits, row) alone, and the compiler would otherwise hoist all three bit widths' deltas of the whole row out of
    // the candidate loop and keep them in registers (472 VGPRs at R = 16 against 64 for the row itself).
    uint32_t mb[R], mr = mrow;
    asm volatile("" : "+v"(mr));
#pragma unroll
    for (int j = 0; j < R; ++j) {
      mb[j] = block == 32 ? m8[j] : block == 64 ? m16[j] : block == 128 ? m32[j] : m64[j];
      asm volatile("" : "+v"(mb[j]));
    }
    double acc;
    if (block == 0) {
      if (bits == 8) acc = candidate_pieces<8, false, TPR, R>(v, mb, mr, dst_row, lane, cols4);
      else if (bits == 4) acc = candidate_pieces<4, false, TPR, R>(v, mb, mr, dst_row, lane, cols4);
      else acc = candidate_pieces<2, false, TPR, R>(v, mb, mr, dst_row, lane, cols4);
    } else {
      if (bits == 8) acc = candidate_pieces<8, true, TPR, R>(v, mb, mr, dst_row, lane, cols4);
      else if (bits == 4) acc = candidate_pieces<4, true, TPR, R>(v, mb, mr, dst_row, lane, cols4);
      else acc = candidate_pieces<2, true, TPR, R>(v, mb, mr, dst_row, lane, cols4);
    }
    if (a.sq != nullptr) {      // (the same for the whole grid)
      acc = wave_sum(acc);
      if constexpr (TPR > kWave) {
        if ((threadIdx.x & (kWave - 1)) == 0) sums[k][threadIdx.x / kWave] = acc;      // added up behind the loop
      } else {
        if (lane == 0) a.sq[static_cast<int64_t>(k) * a.rows + row] = acc;
      }
    }
  }
  if constexpr (TPR > kWave) {      // one barrier for all candidates; the waves' partials in index order
    if (a.sq != nullptr) {
      __syncthreads();
      const int k = threadIdx.x;
      if (k < a.count)
        a.sq[static_cast<int64_t>(k) * a.rows + row] = ((sums[k][0] + sums[k][1]) + sums[k][2]) + sums[k][3];
    }
  }
}

// ---------------------------------------------------------------- generic route
__device__ __forceinline__ uint32_t block_max(uint32_t m, uint32_t* part) {
  m = group_max_u32<kWave>(m);
  __syncthreads();      // (part may still be read from the call before)
  if ((threadIdx.x & (kWave - 1)) == 0) part[threadIdx.x / kWave] = m;
  __syncthreads();
  return max(max(part[0], part[1]), max(part[2], part[3]));
}

template <int BITS>
__device__ __forceinline__ double generic_row(const float* __restrict__ xr, float* dr, int64_t cols, uint32_t mrow) {
  uint16_t hb;
  const float s = make_scale<BITS, false>(mrow, nullptr, 0, &hb);
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < cols; i += kThreads) {
    const float x = xr[i];
    const float d = delta_of(x, quant_sym<BITS>(x, s), s);
    dr[i] = d;
    const double e = d;
    acc += e * e;
  }
  return acc;
}

// a wave per block of `block` columns (32 ... 256), the blocks of the row dealt to the four waves in turn
template <int BITS>
__device__ __forceinline__ double generic_blocks(const float* __restrict__ xr, float* dr, int64_t cols, int block) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t groups = cols / block;
  double acc = 0.0;
  for (int64_t g = threadIdx.x / kWave; g < groups; g += kWaves) {
    const float* xg = xr + g * block;
    float* dg = dr + g * block;
    uint32_t m = 0;
    for (int i = lane; i < block; i += kWave) m = max(m, abs_bits(xg[i]));
    m = group_max_u32<kWave>(m);
    uint16_t hb;
    const float s = make_scale<BITS, true>(m, nullptr, 0, &hb);
    for (int i = lane; i < block; i += kWave) {
      const float x = xg[i];
      const float d = delta_of(x, quant_sym<BITS>(x, s), s);
      dg[i] = d;
      const double e = d;
      acc += e * e;
    }
  }
  return acc;
}

__global__ __launch_bounds__(kThreads) void delta_sweep_generic_kernel(SweepArgs a) {
  __shared__ uint32_t part[kWaves];
  __shared__ double sums[kMaxCandidates][kWaves];
  const int64_t row = blockIdx.x;
  const float* __restrict__ xr = a.x + row * a.cols;
  uint32_t m = 0;
  for (int64_t i = threadIdx.x; i < a.cols; i += kThreads) m = max(m, abs_bits(xr[i]));
  const uint32_t mrow = block_max(m, part);
  for (int k = 0; k < a.count; ++k) {
    const int bits = a.bits[k], block = a.block[k];
    float* dr = a.delta + static_cast<int64_t>(k) * a.delta_stride + row * a.cols;
    double acc;
    if (block == 0) {
      acc = bits == 8 ? generic_row<8>(xr, dr, a.cols, mrow) : bits == 4 ? generic_row<4>(xr, dr, a.cols, mrow)
                                                                        : generic_row<2>(xr, dr, a.cols, mrow);
    } else {
      acc = bits == 8 ? generic_blocks<8>(xr, dr, a.cols, block) : bits == 4 ? generic_blocks<4>(xr, dr, a.cols, block)
                                                                            : generic_blocks<2>(xr, dr, a.cols, block);
    }
    if (a.sq != nullptr) {
      acc = wave_sum(acc);
      if ((threadIdx.x & (kWave - 1)) == 0) sums[k][threadIdx.x / kWave] = acc;
    }
  }
  if (a.sq != nullptr) {
    __syncthreads();
    const int k = threadIdx.x;
    if (k < a.count) a.sq[static_cast<int64_t>(k) * a.rows + row] = ((sums[k][0] + sums[k][1]) + sums[k][2]) + sums[k][3];
  }
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace
}  // namespace mi355q

using namespace mi355q;

extern "C" int32_t mi355q_requant_delta_sweep_f32(const float* x, int64_t rows, int64_t cols, int32_t count,
                                                  const int32_t* bits, const int32_t* block, float* delta_out,
                                                  int64_t delta_stride, double* sq_rows_out, void* stream) {
  clear_error();
  if (rows < 0 || cols < 0) return fail(MI355Q_BAD_ARG, "negative shape");
  if (count < 1 || count > kMaxCandidates)
    return fail(MI355Q_BAD_ARG, "count must be in [1, %d] (got %d)", kMaxCandidates, count);
  if (bits == nullptr || block == nullptr) return fail(MI355Q_BAD_ARG, "the candidate tables must not be null");
  SweepArgs a{};
  for (int32_t k = 0; k < count; ++k) {
    if (bits[k] != 8 && bits[k] != 4 && bits[k] != 2)
      return fail(MI355Q_BAD_ARG, "bits must be 8, 4 or 2 (got %d for candidate %d)", bits[k], k);
    if (block[k] != 0 && block[k] != 32 && block[k] != 64 && block[k] != 128 && block[k] != 256)
      return fail(MI355Q_BAD_ARG, "block must be 0, 32, 64, 128 or 256 (got %d for candidate %d)", block[k], k);
    if (block[k] > 0 && cols % block[k] != 0)
      return fail(MI355Q_BAD_ARG, "Quantized dimension %lld is not divisible by block size %d.",
                  static_cast<long long>(cols), block[k]);
    a.bits[k] = bits[k];
    a.block[k] = block[k];
  }
  if (rows == 0 || cols == 0) return MI355Q_OK;
  if (x == nullptr || delta_out == nullptr) return fail(MI355Q_BAD_ARG, "x and delta_out must not be null");
  if (rows > 0x7FFFFFFFLL) return fail(MI355Q_UNSUPPORTED, "rows > 2^31-1");
  if (cols > 0x7FFFFFFFFFFFFFFFLL / rows || delta_stride < rows * cols)
    return fail(MI355Q_BAD_ARG, "delta_stride %lld is smaller than rows * cols", static_cast<long long>(delta_stride));
  a.x = x; a.delta = delta_out; a.delta_stride = delta_stride; a.sq = sq_rows_out;
  a.rows = rows; a.cols = cols; a.count = count;
  hipStream_t st = as_stream(stream);
  const dim3 blk(kThreads);
  const int64_t cols4 = cols / 4;
  const bool vec = cols % 4 == 0 && cols4 <= kThreads * 16 && al16(x) && al16(delta_out) &&
                   (count == 1 || delta_stride % 4 == 0);
  if (vec) {
#define MI355Q_SWEEP(TPR, R)                                                                              \
  hipLaunchKernelGGL((delta_sweep_rows_kernel<TPR, R>),                                                   \
                     dim3(static_cast<unsigned>((rows + (kThreads / TPR) - 1) / (kThreads / TPR))), blk, 0, st, a)
    if (cols4 <= 64) MI355Q_SWEEP(64, 1);
    else if (cols4 <= 128) MI355Q_SWEEP(64, 2);
    else if (cols4 <= 256) MI355Q_SWEEP(64, 4);
    else if (cols4 <= 512) MI355Q_SWEEP(256, 2);
    else if (cols4 <= 1024) MI355Q_SWEEP(256, 4);
    else if (cols4 <= 2048) MI355Q_SWEEP(256, 8);
    else MI355Q_SWEEP(256, 16);
#undef MI355Q_SWEEP
  } else {
    hipLaunchKernelGGL(delta_sweep_generic_kernel, dim3(static_cast<unsigned>(rows)), blk, 0, st, a);
  }
  MI355Q_CHECK_LAUNCH("requant delta sweep launch");
  return MI355Q_OK;
}
