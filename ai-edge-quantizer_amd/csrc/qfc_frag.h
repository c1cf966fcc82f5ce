// The stored weight of the integer FULLY_CONNECTED kernels: its elements, the per-row / per-block weight sums, and the
// B fragments of the int8 MFMAs. Included by qfc_tile.h (the main loop that qfc.hip, qfc16.hip and qfc_out.hip share).
#pragma once

#include "common.h"
#include "compare_target.h"

namespace mi355q {
namespace {

constexpr int kQfcThreads = 256;

using I32x4 = __attribute__((ext_vector_type(4))) int;

// ---------------------------------------------------------------- stored weight elements
// element e of the flat weight (I4 / I2 packed over the whole tensor, element 0 in the low bits)
__device__ __forceinline__ int weight_element(const uint8_t* w, int kind, long long e) {
  if (kind == MI355Q_CMP_I8) return reinterpret_cast<const int8_t*>(w)[e];
  if (kind == MI355Q_CMP_I4) return packed_element(w[e >> 1], 4, static_cast<int>(e & 1));
  return packed_element(w[e >> 2], 2, static_cast<int>(e & 3));
}

// wsum[seg] = Sum of the `len` elements of segment seg (consecutive in the flat weight); W lanes per segment.
template <int W>
__global__ __launch_bounds__(kQfcThreads) void weight_sums_kernel(const uint8_t* __restrict__ w, int kind, long long segments,
                                                                  long long len, int32_t* __restrict__ wsum) {
  const long long seg = static_cast<long long>(blockIdx.x) * (kQfcThreads / W) + threadIdx.x / W;
  const int sub = threadIdx.x % W;
  int s = 0;
  if (seg < segments)
    for (long long k = sub; k < len; k += W) s += weight_element(w, kind, seg * len + k);
#pragma unroll
  for (int off = W / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, kWave);
  if (seg < segments && sub == 0) wsum[seg] = s;
}

// wsum[segments] of segments of `len` elements each; 8 lanes per segment up to 256 elements, a wave beyond.
inline int32_t launch_weight_sums(const uint8_t* w, int kind, long long segments, long long len, int32_t* wsum,
                                  hipStream_t st) {
  if (len <= 256) {
    const long long blocks = (segments + kQfcThreads / 8 - 1) / (kQfcThreads / 8);
    if (blocks > 0x7FFFFFFFLL) return fail(MI355Q_UNSUPPORTED, "too many weight blocks for one launch");
    hipLaunchKernelGGL(weight_sums_kernel<8>, dim3(static_cast<unsigned>(blocks)), dim3(kQfcThreads), 0, st, w, kind,
                       segments, len, wsum);
  } else {
    const long long blocks = (segments + kQfcThreads / kWave - 1) / (kQfcThreads / kWave);
    if (blocks > 0x7FFFFFFFLL) return fail(MI355Q_UNSUPPORTED, "too many weight blocks for one launch");
    hipLaunchKernelGGL(weight_sums_kernel<kWave>, dim3(static_cast<unsigned>(blocks)), dim3(kQfcThreads), 0, st, w, kind,
                       segments, len, wsum);
  }
  MI355Q_CHECK_LAUNCH("weight sums launch");
  return MI355Q_OK;
}

// ---------------------------------------------------------------- B fragments of the int8 MFMAs
// 8 nibbles of a word -> two words of 4 sign-extended bytes each (nibble 0 in the low byte of the first)
__device__ __forceinline__ void unpack_i4(uint32_t p, int& lo, int& hi) {
  uint32_t e = p & 0x0F0F0F0Fu, o = (p >> 4) & 0x0F0F0F0Fu;       // nibbles 0,2,4,6 and 1,3,5,7
  e |= (e & 0x08080808u) * 0x1Eu;                                 // 0x08 * 0x1E = 0xF0: sign bits, within the byte
  o |= (o & 0x08080808u) * 0x1Eu;
  lo = static_cast<int>((e & 0xFFu) | ((o & 0xFFu) << 8) | ((e & 0xFF00u) << 8) | ((o & 0xFF00u) << 16));
  hi = static_cast<int>(((e >> 16) & 0xFFu) | (((o >> 16) & 0xFFu) << 8) | ((e >> 24) << 16) | ((o >> 24) << 24));
}

// 4 two-bit fields of a byte -> a word of 4 sign-extended bytes (field 0 in the low byte)
__device__ __forceinline__ int unpack_i2(uint32_t b) {
  uint32_t v = (b | (b << 6) | (b << 12) | (b << 18)) & 0x03030303u;
  v |= (v & 0x02020202u) * 0x7Fu;                                 // 0x02 * 0x7F = 0xFE
  return static_cast<int>(v);
}

template <int KSTEP> struct FragOf;
template <> struct FragOf<64> { using T = I32x4; };
template <> struct FragOf<32> { using T = long; };

__device__ __forceinline__ long two_words(int lo, int hi) {
  return static_cast<long>((static_cast<unsigned long>(static_cast<uint32_t>(hi)) << 32) | static_cast<uint32_t>(lo));
}

// The raw bytes of a lane's KSTEP / 4 consecutive weight elements at element offset e (a multiple of KSTEP / 4).
template <int KIND, int KSTEP> struct RawW;
template <> struct RawW<MI355Q_CMP_I8, 64> {
  using T = I32x4;
  static __device__ __forceinline__ T load(const uint8_t* w, long long e) { return *reinterpret_cast<const I32x4*>(w + e); }
  static __device__ __forceinline__ T zero() { return I32x4{0, 0, 0, 0}; }
  static __device__ __forceinline__ I32x4 unpack(T r) { return r; }
};
template <> struct RawW<MI355Q_CMP_I8, 32> {
  using T = long;
  static __device__ __forceinline__ T load(const uint8_t* w, long long e) { return *reinterpret_cast<const long*>(w + e); }
  static __device__ __forceinline__ T zero() { return 0; }
  static __device__ __forceinline__ long unpack(T r) { return r; }
};
template <> struct RawW<MI355Q_CMP_I4, 64> {
  using T = unsigned long;
  static __device__ __forceinline__ T load(const uint8_t* w, long long e) {
    return *reinterpret_cast<const unsigned long*>(w + (e >> 1));
  }
  static __device__ __forceinline__ T zero() { return 0; }
  static __device__ __forceinline__ I32x4 unpack(T r) {
    int a, b, c, d;
    unpack_i4(static_cast<uint32_t>(r), a, b);
    unpack_i4(static_cast<uint32_t>(r >> 32), c, d);
    return I32x4{a, b, c, d};
  }
};
template <> struct RawW<MI355Q_CMP_I4, 32> {
  using T = uint32_t;
  static __device__ __forceinline__ T load(const uint8_t* w, long long e) {
    return *reinterpret_cast<const uint32_t*>(w + (e >> 1));
  }
  static __device__ __forceinline__ T zero() { return 0; }
  static __device__ __forceinline__ long unpack(T r) {
    int a, b;
    unpack_i4(r, a, b);
    return two_words(a, b);
  }
};
template <> struct RawW<MI355Q_CMP_I2, 64> {
  using T = uint32_t;
  static __device__ __forceinline__ T load(const uint8_t* w, long long e) {
    return *reinterpret_cast<const uint32_t*>(w + (e >> 2));
  }
  static __device__ __forceinline__ T zero() { return 0; }
  static __device__ __forceinline__ I32x4 unpack(T r) {
    return I32x4{unpack_i2(r & 0xFFu), unpack_i2((r >> 8) & 0xFFu), unpack_i2((r >> 16) & 0xFFu), unpack_i2(r >> 24)};
  }
};
template <> struct RawW<MI355Q_CMP_I2, 32> {
  using T = uint16_t;
  static __device__ __forceinline__ T load(const uint8_t* w, long long e) {
    return *reinterpret_cast<const uint16_t*>(w + (e >> 2));
  }
  static __device__ __forceinline__ T zero() { return 0; }
  static __device__ __forceinline__ long unpack(T r) { return two_words(unpack_i2(r & 0xFFu), unpack_i2(r >> 8)); }
};

}  // namespace
}  // namespace mi355q
