// MSE scale (a14), order-exact: k * sqrt(mean(x^2)) with the sum of squares in the order NumPy adds in (numpy_sum.h).
//
//   ref: algorithms/uniform_quantize/mse.py:100-109   (k * sqrt(mean(x^2)))
#include <cstdlib>

#include "numpy_sum.h"

namespace mi355q {
namespace {

// [outer, channels, inner] view, one wave per channel: NumPy hands each contiguous segment to the inner loop separately
// and keeps one running total per channel (octav_seg_kernel in octav.hip is the masked form).
__global__ void mse_scale_seg_kernel(const float* __restrict__ x, long long outer, long long channels,
                                     int inner, float multiplier, float* __restrict__ scale) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const long long c = static_cast<long long>(blockIdx.x) * (blockDim.x / kWave) + wave;
  if (c >= channels) return;
  float acc = 0.f;
  bool first = true;
  for (long long o = 0; o < outer; ++o) {
    const float* u = x + (o * channels + c) * inner;
    for (int k = 0; k < inner; k += kChunk) {
      const int n = inner - k < kChunk ? inner - k : kChunk;
      const float part = pairwise_sum<true, 8>(u + k, n, lane);
      acc = first ? part : acc + part;
      first = false;
    }
  }
  const float mean = acc / static_cast<float>(outer * inner);
  if (lane == 0) scale[c] = multiplier * __builtin_sqrtf(mean);
}

// Channel-last units, x viewed as [outer, channels]: a plain left-to-right float32 sum over o per channel, one lane per
// channel (octav_cols_kernel in octav.hip is the masked form; tests/numpy_sum_model.py states and checks the order).
constexpr int kColsUnroll = 8;

__global__ __launch_bounds__(256) void mse_scale_cols_kernel(const float* __restrict__ x, long long outer,
                                                            long long channels, float multiplier,
                                                            float* __restrict__ scale) {
  const long long c = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (c >= channels) return;
  const float* p = x + c;
  float acc = 0.f;
  long long o = 0;
  for (; o + kColsUnroll <= outer; o += kColsUnroll) {
    float v[kColsUnroll];
#pragma unroll
    for (int k = 0; k < kColsUnroll; ++k) v[k] = p[static_cast<long long>(k) * channels];
#pragma unroll
    for (int k = 0; k < kColsUnroll; ++k) acc = acc + v[k] * v[k];
    p += kColsUnroll * channels;
  }
  for (; o < outer; ++o, p += channels) acc = acc + (*p) * (*p);
  scale[c] = multiplier * __builtin_sqrtf(acc / static_cast<float>(outer));
}

struct MseArgs {
  const float* x;
  long long units;
  int len;
  int lds_stride;
  float multiplier;
  float* scale;
  // mi355q_mse_requant_f32: the wave that made a unit's scale also quantizes the unit (it has just read it: the second
  // pass comes out of the L2), four int8 per lane and store; null: scales only
  unsigned* q = nullptr;     // [units][len / 4]
  float lo = 0.f, hi = 0.f;
};

// Leaves of NumPy's pairwise recursion over [lo, lo + n), in order (n <= 8192: at most 128).
__device__ void list_leaves(int lo, int n, int* leaf_lo, int* leaf_n, int* count) {
  if (n <= 128) {
    leaf_lo[*count] = lo;
    leaf_n[*count] = n;
    ++*count;
    return;
  }
  int n2 = n / 2;
  n2 -= n2 % 8;
  list_leaves(lo, n2, leaf_lo, leaf_n, count);
  list_leaves(lo + n2, n - n2, leaf_lo, leaf_n, count);
}

// The recursion again with the leaves' sums known (consumed in order).
__device__ float fold_leaves(int n, const float* leaf_sum, int* next) {
  if (n <= 128) return leaf_sum[(*next)++];
  int n2 = n / 2;
  n2 -= n2 % 8;
  const float left = fold_leaves(n2, leaf_sum, next);
  return left + fold_leaves(n - n2, leaf_sum, next);
}

// sum(x*x) of contiguous units in NumPy's order, all lanes busy: a unit is a sequence of
// 8192-element chunks added in order; a chunk is a tree of leaves of <= 128 elements; a leaf is
// eight strided accumulators. One wave per unit; eight lanes share a leaf, one per accumulator
// (a wave step reads eight 32-byte runs straight from global memory, every byte of every cache
// line exactly once), the accumulators fold by an xor butterfly -- ((r0+r1)+(r2+r3))+((r4+r5)+
// (r6+r7)), IEEE addition commutes so both partners agree -- and lane 0 folds the leaf sums in
// the recursion's order. The two leaf tables a unit needs (full chunk, last chunk) are listed
// once per block. This is the general form (any length); mse_scale_balanced_kernel below takes
// the lengths whose tree is complete.
__global__ __launch_bounds__(256) void mse_scale_leaves_kernel(MseArgs a) {
  __shared__ int leaf_lo[2][128], leaf_n[2][128], leaves[2];
  __shared__ float leaf_sum[4][128];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int k = lane & 7, slot = lane >> 3;
  const int last_len = a.len - (a.len - 1) / kChunk * kChunk;  // 1 .. 8192
  if (threadIdx.x == 0 || threadIdx.x == kWave) {
    const int t = threadIdx.x == 0 ? 0 : 1;
    int c = 0;
    list_leaves(0, t == 0 ? (a.len < kChunk ? a.len : kChunk) : last_len, leaf_lo[t], leaf_n[t], &c);
    leaves[t] = c;
  }
  __syncthreads();
  const long long unit = static_cast<long long>(blockIdx.x) * 4 + wave;
  const bool live_unit = unit < a.units;
  const float* u = a.x + (live_unit ? unit : 0) * a.len;
  float acc = 0.f;
  for (int c0 = 0; c0 < a.len; c0 += kChunk) {
    const int n = a.len - c0 < kChunk ? a.len - c0 : kChunk;
    const int t = (c0 + kChunk >= a.len) ? 1 : 0;
    const int count = leaves[t];
    for (int base = 0; base < count; base += 8) {
      const int leaf = base + slot;
      const bool live = leaf < count;
      const float* p = u + c0 + (live ? leaf_lo[t][leaf] : 0);
      const int ln = live ? leaf_n[t][leaf] : 0;
      float res = 0.f;
      if (ln < 8) {  // short leaf (only a chunk shorter than 8 has one): left to right
        for (int i = 0; i < ln; ++i) res = res + p[i] * p[i];
      } else {
        float v[16];  // all loads first, then the ordered adds
#pragma unroll
        for (int q = 0; q < 16; ++q) v[q] = (8 * (q + 1) <= ln) ? p[8 * q + k] : 0.f;
        float r = v[0] * v[0];
#pragma unroll
        for (int q = 1; q < 16; ++q)
          if (8 * (q + 1) <= ln) r = r + v[q] * v[q];
        r = r + __shfl_xor(r, 1, kWave);
        r = r + __shfl_xor(r, 2, kWave);
        r = r + __shfl_xor(r, 4, kWave);
        for (int i = ln & ~7; i < ln; ++i) r = r + p[i] * p[i];
        res = r;
      }
      if (live && k == 0) leaf_sum[wave][leaf] = res;
    }
    __syncthreads();
    if (lane == 0) {
      int next = 0;
      const float part = fold_leaves(n, leaf_sum[wave], &next);
      acc = c0 == 0 ? part : acc + part;
    }
    __syncthreads();
  }
  if (lane == 0 && live_unit) {
    const float mean = acc / static_cast<float>(a.len);
    a.scale[unit] = a.multiplier * __builtin_sqrtf(mean);
  }
}

// The same sum for units whose chunks are balanced (common.h; every full chunk is: 8192 =
// 128 << 6): no
// tables, no LDS, no serial fold. Eight lanes share a leaf as above; leaf index = 8 * step +
// (lane >> 3), so the three lowest tree levels are lane butterflies (xor 8, 16, 32), and the
// levels above pair whole steps, folded as they arrive like a binary counter (the step loop is
// unrolled, so that is straight-line code).
__global__ __launch_bounds__(256) void mse_scale_balanced_kernel(MseArgs a, int last_leaf, int last_depth) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int k = lane & 7, slot = lane >> 3;
  const long long unit = static_cast<long long>(blockIdx.x) * 4 + wave;
  if (unit >= a.units) return;
  const float* u = a.x + unit * a.len;
  float acc = 0.f;
  for (int c0 = 0; c0 < a.len; c0 += kChunk) {
    const bool last = c0 + kChunk >= a.len;
    const int leaf_len = last ? last_leaf : 128, depth = last ? last_depth : 6;
    const int count = 1 << depth;
    const int steps = count > 8 ? count >> 3 : 1;
    float lvl0 = 0.f, lvl1 = 0.f, lvl2 = 0.f, x = 0.f;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      if (s < steps) {
        const int leaf = s * 8 + slot;
        const float* p = u + c0 + static_cast<long long>(leaf < count ? leaf : 0) * leaf_len + k;
        float v[16];  // all loads first, then the ordered adds
#pragma unroll
        for (int q = 0; q < 16; ++q) v[q] = (8 * (q + 1) <= leaf_len) ? p[8 * q] : 0.f;
        float r = v[0] * v[0];
#pragma unroll
        for (int q = 1; q < 16; ++q)
          if (8 * (q + 1) <= leaf_len) r = r + v[q] * v[q];
        r = r + __shfl_xor(r, 1, kWave);  // ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)); addition commutes
        r = r + __shfl_xor(r, 2, kWave);
        r = r + __shfl_xor(r, 4, kWave);
        if (count > 1) r = r + __shfl_xor(r, 8, kWave);   // leaves 2i, 2i+1
        if (count > 2) r = r + __shfl_xor(r, 16, kWave);
        if (count > 4) r = r + __shfl_xor(r, 32, kWave);
        x = r;  // the sum of this step's (up to) eight leaves
        if (s & 1) {
          x = lvl0 + x;
          if (s & 2) {
            x = lvl1 + x;
            if (s & 4) x = lvl2 + x; else lvl2 = x;
          } else {
            lvl1 = x;
          }
        } else {
          lvl0 = x;
        }
      }
    }
    acc = c0 == 0 ? x : acc + x;
  }
  acc = lane_bcast(acc, 0);      // (lane 0's total is the unit's: short last chunks leave other slots with copies of leaf 0)
  const float mean = acc / static_cast<float>(a.len);
  const float scale = a.multiplier * __builtin_sqrtf(mean);
  if (lane == 0) a.scale[unit] = scale;
  if (a.q != nullptr) {
    // uniform_quantize with a zero zero point: rint(x / scale) clipped (ref uniform_quantize_tensor.py:357-360; the reference's
    // `+ zero_point` in float64 changes no value here: it only turns -0.0 into +0.0, and both round to the integer 0)
    const float4* u4 = reinterpret_cast<const float4*>(u);
    unsigned* q = a.q + unit * (a.len / 4);
    for (int i = lane; i < a.len / 4; i += kWave) {
      const float4 v = u4[i];
      const unsigned w = (static_cast<unsigned>(round_clip(v.x / scale, a.lo, a.hi)) & 0xFFu) |
                         ((static_cast<unsigned>(round_clip(v.y / scale, a.lo, a.hi)) & 0xFFu) << 8) |
                         ((static_cast<unsigned>(round_clip(v.z / scale, a.lo, a.hi)) & 0xFFu) << 16) |
                         ((static_cast<unsigned>(round_clip(v.w / scale, a.lo, a.hi)) & 0xFFu) << 24);
      __builtin_nontemporal_store(w, q + i);
    }
  }
}

// What the three entry points check first, in their common order: negative extents, `bits` where the call has it,
// no units (MI355Q_OK), an empty unit, a unit too long for an int (`too_large` names the extent), null pointers.
// The view is [outer, units, len]; outer is 1 for the contiguous forms. false: return *status.
bool mse_begin(int64_t outer, int64_t units, int64_t len, const int32_t* bits, const char* too_large, bool null_pointer,
               int32_t* status) {
  const auto refuse = [status](int32_t st) { *status = st; return false; };
  clear_error();
  if (outer < 0 || units < 0 || len < 0) return refuse(fail(MI355Q_BAD_ARG, "negative shape"));
  if (bits != nullptr && (*bits < 2 || *bits > 8)) return refuse(fail(MI355Q_BAD_ARG, "bits must be in [2, 8]"));
  if (units == 0) return refuse(MI355Q_OK);
  if (outer == 0 || len == 0) return refuse(fail(MI355Q_BAD_SHAPE, "empty reduction unit"));
  if (len > 0x7FFFFFFFLL - 64) return refuse(fail(MI355Q_UNSUPPORTED, "%s", too_large));
  if (null_pointer) return refuse(fail(MI355Q_BAD_ARG, "null pointer"));
  *status = MI355Q_OK;
  return true;
}

}  // namespace
}  // namespace mi355q

using namespace mi355q;

extern "C" int32_t mi355q_mse_scale_nd_f32(const float* x, int64_t outer, int64_t channels,
                                           int64_t inner, float multiplier, float* scale_out,
                                           void* stream) {
  if (outer == 1) return mi355q_mse_scale_f32(x, channels, inner, multiplier, scale_out, stream);
  int32_t status;
  if (!mse_begin(outer, channels, inner, nullptr, "inner too large", !x || !scale_out, &status)) return status;
  if (channels == 1) {  // one channel: NumPy merges the axes and sums ONE contiguous vector (chunks of 8192 across the segments)
    if (outer > (0x7FFFFFFFLL - 64) / inner) return fail(MI355Q_UNSUPPORTED, "one channel too long");
    return mi355q_mse_scale_f32(x, 1, outer * inner, multiplier, scale_out, stream);
  }
  hipStream_t st = as_stream(stream);
  if (inner == 1)
    hipLaunchKernelGGL(mse_scale_cols_kernel, dim3(static_cast<unsigned>((channels + 255) / 256)), dim3(256),
                       0, st, x, static_cast<long long>(outer), static_cast<long long>(channels),
                       multiplier, scale_out);
  else
    hipLaunchKernelGGL(mse_scale_seg_kernel, dim3(static_cast<unsigned>((channels + 3) / 4)), dim3(4 * kWave),
                       0, st, x, static_cast<long long>(outer), static_cast<long long>(channels),
                       static_cast<int>(inner), multiplier, scale_out);
  MI355Q_CHECK_LAUNCH("mse nd launch");
  return MI355Q_OK;
}

extern "C" int32_t mi355q_mse_scale_f32(const float* x, int64_t units, int64_t unit_len,
                                        float multiplier, float* scale_out, void* stream) {
  int32_t status;
  if (!mse_begin(1, units, unit_len, nullptr, "unit_len too large", !x || !scale_out, &status)) return status;
  MseArgs a{x, units, static_cast<int>(unit_len), 0, multiplier, scale_out};
  hipStream_t st = as_stream(stream);
  const dim3 grid(static_cast<unsigned>((units + 3) / 4)), blk(4 * kWave);
  int leaf = 0, depth = 0;
  if (balanced_chunk(a.len - (a.len - 1) / kChunk * kChunk, &leaf, &depth))
    hipLaunchKernelGGL(mse_scale_balanced_kernel, grid, blk, 0, st, a, leaf, depth);
  else
    hipLaunchKernelGGL(mse_scale_leaves_kernel, grid, blk, 0, st, a);
  MI355Q_CHECK_LAUNCH("mse_scale launch");
  return MI355Q_OK;
}

extern "C" int32_t mi355q_mse_requant_f32(const float* x, int64_t units, int64_t unit_len, float multiplier, int32_t bits,
                                          int32_t narrow, float* scale_out, int8_t* q_out, void* stream) {
  int32_t status;
  if (!mse_begin(1, units, unit_len, &bits, "unit_len too large", !x || !scale_out || !q_out, &status)) return status;
  int leaf = 0, depth = 0;
  const int len = static_cast<int>(unit_len);
  const bool one_kernel = unit_len % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(q_out) & 3) == 0 &&
                          balanced_chunk(len - (len - 1) / kChunk * kChunk, &leaf, &depth) && !getenv("MI355Q_MSE_TWO_KERNELS");
  if (!one_kernel) {      // the scale kernel of any length, then the quantizer every other algorithm uses
    const int32_t st = mi355q_mse_scale_f32(x, units, unit_len, multiplier, scale_out, stream);
    if (st != MI355Q_OK) return st;
    return mi355q_quantize_f32(x, 1, units, unit_len, scale_out, 0, nullptr, 1, bits, narrow, 8, q_out, stream);
  }
  MseArgs a{x, units, len, 0, multiplier, scale_out};
  a.q = reinterpret_cast<unsigned*>(q_out);
  a.hi = static_cast<float>((1 << (bits - 1)) - 1);
  a.lo = -static_cast<float>(1 << (bits - 1)) + (narrow ? 1.f : 0.f);
  hipLaunchKernelGGL(mse_scale_balanced_kernel, dim3(static_cast<unsigned>((units + 3) / 4)), dim3(4 * kWave), 0, as_stream(stream), a,
                     leaf, depth);
  MI355Q_CHECK_LAUNCH("mse requant launch");
  return MI355Q_OK;
}
