// Block-diagonal Hadamard rotation (K6): out = reshape(x, (-1, h)) @ (H_h / sqrt(h)).
//
//   ref: algorithms/uniform_quantize/hadamard_rotation.py:48-90 (Sylvester H / sqrt(h), FP32)
//   ref: algorithms/uniform_quantize/hadamard_rotation.py:93-134 (reshape(-1, h) @ H)
//
// The reference multiplies by the dense matrix with sgemm (O(h) work per output);
// here every length-h vector is transformed in LDS with a fast Walsh-Hadamard
// butterfly (log2 h stages), which is the same linear map because the Sylvester
// (Kronecker) order is the natural-order WHT and H is symmetric. Each input is
// first multiplied by fl(1/fl(sqrt(h))) -- the value of every |H entry| in the
// reference -- so only the order of the FP32 additions differs from sgemm
// (tolerance class T2).
//
// What is exact, whatever the order: an impulse +-2^j at p gives +-2^j r (-1)^popcount(p & q) for every h (one product,
// then additions of zeros); dense integers |x| < 2^(23 - log2 h) give the integer Sylvester product for h = 4^m (r is
// a power of two and every partial sum fits float32). Dense floats equal, bit for bit, r-scaled inputs sent through
// (u + v, u - v) stages over index bits in the order of the route (tests/hadamard_route_cases.py):
//   fwht_kernel             0, 1, ..., L-1      h < 256, or x / out not 16-byte aligned (any h; one vector per block
//                                               from h = 2048 on, 64 KiB of dynamic LDS at h = 16384)
//   fwht_tile_kernel<12>    0, 1, 10, 11, 2..9  256 <= h <= 4096 (bits >= L skipped: the fwht_kernel order up to 1024)
//   fwht_tile_kernel<13>    0, 1, 11, 12, 2..9, 10       h = 8192
//   fwht_tile_kernel<14>    0, 1, 12, 13, 2..9, 10, 11   h = 16384
// So from h = 2048 on the misaligned fallback differs in bits from the tile kernels (another order of the same
// additions); mi355q_weight_delta_transformed_f32 takes its network from h alone.
//
// Both kernels are templates over a source (element e, or the four elements e .. e+3) and a sink (which receives
// them). mi355q_hadamard_rotate_f32 instantiates plain float loads and stores. The effective-weight delta of the layer
// output error, mi355q_weight_delta_transformed_f32, instantiates the SAME networks with a target dequantized in
// registers (compare_target.h) as the source and `reference[e] - v` as the sink: out = W - rotate_h(dequant(W^)) in
// one pass, with the arithmetic that rotated the weight when it was quantized. Its multiply form,
// out = W - dequant(W^) * m, is the grid-stride kernel at the end.
#include "common.h"
#include "compare_target.h"

namespace mi355q {
namespace {

struct FloatSource {
  const float* __restrict__ x;
  __device__ __forceinline__ bool vec(long long e) const { return (reinterpret_cast<uintptr_t>(x + e) & 15) == 0; }
  __device__ __forceinline__ float4 load4(long long e) const { return *reinterpret_cast<const float4*>(x + e); }
  __device__ __forceinline__ float load(long long e) const { return x[e]; }
};

struct FloatSink {
  float* __restrict__ out;
  __device__ __forceinline__ bool vec(long long e) const { return (reinterpret_cast<uintptr_t>(out + e) & 15) == 0; }
  __device__ __forceinline__ void store4(long long e, float4 v) const { *reinterpret_cast<float4*>(out + e) = v; }
  __device__ __forceinline__ void store(long long e, float v) const { out[e] = v; }
};

// A comparison target dequantized in registers. `packed`: an I8 / I4 / I2 target whose pointer is 4-byte aligned and
// whose elements e .. e+3 (e % 4 == 0) share one scale entry (one channel, or inner % 4 == 0): the four are read with
// one load of 4 / 2 / 1 bytes and dequantized by compare_target.h's rule. Everything else takes load_target element
// by element.
struct TargetSource {
  mi355q_compare_pair p;
  int packed;
  __device__ __forceinline__ bool vec(long long e) const { return (e & 3) == 0; }
  __device__ __forceinline__ float load(long long e) const { return load_target(p, e); }
  __device__ __forceinline__ float4 load4(long long e) const {
    if (!packed) return make_float4(load_target(p, e), load_target(p, e + 1), load_target(p, e + 2), load_target(p, e + 3));
    const uint8_t* bytes = static_cast<const uint8_t*>(p.target);
    uint32_t word;
    int bits;
    if (p.target_kind == MI355Q_CMP_I8) {
      word = *reinterpret_cast<const uint32_t*>(bytes + e);
      bits = 8;
    } else if (p.target_kind == MI355Q_CMP_I4) {
      word = *reinterpret_cast<const uint16_t*>(bytes + (e >> 1));   // element 0 in the low nibble
      bits = 4;
    } else {
      word = bytes[e >> 2];
      bits = 2;
    }
    const int64_t c = p.channels == 1 ? 0 : (e / p.inner) % p.channels;
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = dequantize_target(p, packed_element(word, bits, k), c);
    return make_float4(v[0], v[1], v[2], v[3]);
  }
};

// out[e] = reference[e] - v: 16-byte accesses where both pointers allow them, scalar ones otherwise.
struct DeltaSink {
  const float* __restrict__ reference;
  float* __restrict__ out;
  __device__ __forceinline__ bool vec(long long e) const {
    return ((reinterpret_cast<uintptr_t>(reference + e) | reinterpret_cast<uintptr_t>(out + e)) & 15) == 0;
  }
  __device__ __forceinline__ void store4(long long e, float4 v) const {
    const float4 w = *reinterpret_cast<const float4*>(reference + e);
    *reinterpret_cast<float4*>(out + e) = make_float4(w.x - v.x, w.y - v.y, w.z - v.z, w.w - v.w);
  }
  __device__ __forceinline__ void store(long long e, float v) const { out[e] = reference[e] - v; }
};

// One block transforms `vecs` vectors of length h (vecs * h floats in LDS).
template <class Source, class Sink>
__global__ __launch_bounds__(256) void fwht_kernel(Source src, Sink snk, long long n_vec, int h, int log2h, int vecs,
                                                  float r) {
  extern __shared__ __attribute__((aligned(16))) float buf[];
  const int tile = vecs * h;
  const long long first = static_cast<long long>(blockIdx.x) * vecs;
  const long long remain = (n_vec - first) * h;
  const int valid = remain < tile ? static_cast<int>(remain) : tile;
  const long long e0 = first * h;
  if (src.vec(e0) && (valid & 3) == 0) {
    float4* b4 = reinterpret_cast<float4*>(buf);
    for (int i = threadIdx.x; i < valid / 4; i += 256) {
      float4 v = src.load4(e0 + 4 * i);
      b4[i] = make_float4(v.x * r, v.y * r, v.z * r, v.w * r);
    }
  } else {
    for (int i = threadIdx.x; i < valid; i += 256) buf[i] = src.load(e0 + i) * r;
  }
  __syncthreads();
  const int pairs = valid / 2;
  for (int s = 0; s < log2h; ++s) {
    const int half = 1 << s;
    for (int i = threadIdx.x; i < pairs; i += 256) {
      const int lo = ((i >> s) << (s + 1)) | (i & (half - 1));
      const float u = buf[lo], v = buf[lo + half];
      buf[lo] = u + v;
      buf[lo + half] = u - v;
    }
    __syncthreads();
  }
  if (snk.vec(e0) && (valid & 3) == 0) {
    const float4* b4 = reinterpret_cast<const float4*>(buf);
    for (int i = threadIdx.x; i < valid / 4; i += 256) snk.store4(e0 + 4 * i, b4[i]);
  } else {
    for (int i = threadIdx.x; i < valid; i += 256) snk.store(e0 + i, buf[i]);
  }
}

// ---- h >= 256: radix-16 passes over a tile of 4096 / 8192 / 16384 elements --------------------
// The radix-2 kernel above sends every element through LDS twice per stage (12 stages at
// h = 4096: 24 LDS accesses per element for 2 HBM accesses) and is LDS-bound at ~2.6 TB/s. Here a
// thread keeps 16 elements in registers and does up to four butterfly stages at once over a tile
// of T = 2^LOG2T elements (T / 16 threads):
//   pass 1  index bits {0, 1, LOG2T-2, LOG2T-1}: straight from the coalesced float4 global loads
//   pass 2  index bits {2..5}      (LDS read + write)
//   pass 3  index bits {6..9}      (LDS read; for T = 4096 the results go to HBM as 256-byte rows)
//   pass 4  index bits {10..LOG2T-3} (T = 8192: bit 10, T = 16384: bits 10 and 11; then HBM)
// i.e. 4 (T = 4096) or 6 LDS accesses per element. Stages above log2(h) are skipped (those bits
// select the vector inside the tile). The LDS index is XOR-swizzled (bits 2-4 ^= bits 6-8) so
// that pass 2, whose lanes differ in bits {0,1,6..}, still spreads over all banks.
constexpr int kTile = 4096;

__device__ __forceinline__ int swz(int i) { return i ^ (((i >> 6) & 7) << 2); }

template <int NBITS>   // butterflies over the low NBITS bits of the register index, radix 2
__device__ __forceinline__ void butterflies(float (&v)[16], int first_bit, int log2h) {
#pragma unroll
  for (int b = 0; b < NBITS; ++b) {
    if (first_bit + b < log2h) {  // uniform
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        if ((k >> b) & 1) continue;
        const float u = v[k], w = v[k | (1 << b)];
        v[k] = u + w;
        v[k | (1 << b)] = u - w;
      }
    }
  }
}

template <int LOG2T, class Source, class Sink>
__global__ __launch_bounds__((1 << LOG2T) / 16) void fwht_tile_kernel(Source src, Sink snk, long long total, int log2h,
                                                                      float r) {
  constexpr int T = 1 << LOG2T, NT = T / 16;
  __shared__ __attribute__((aligned(16))) float buf[T];
  const int t = threadIdx.x;
  const long long base = static_cast<long long>(blockIdx.x) * T;
  const long long left = total - base;
  const int valid = left < T ? static_cast<int>(left) : T;   // a multiple of h (and of 4)
  float v[16];
  // pass 1: register index k = c | (j << 2)  <->  tile index bits (0,1) and (LOG2T-2, LOG2T-1)
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int f4 = t + NT * j;
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (f4 * 4 < valid) q = src.load4(base + 4 * f4);
    v[j * 4 + 0] = q.x * r; v[j * 4 + 1] = q.y * r; v[j * 4 + 2] = q.z * r; v[j * 4 + 3] = q.w * r;
  }
  butterflies<2>(v, 0, log2h);            // bits 0, 1 (always below log2h: h >= 256)
  {                                       // the two top bits = register bits 2, 3
    float hi[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) hi[k] = v[((k & 3) << 2) | (k >> 2)];   // transpose c <-> j
    butterflies<2>(hi, LOG2T - 2, log2h);
#pragma unroll
    for (int k = 0; k < 16; ++k) v[((k & 3) << 2) | (k >> 2)] = hi[k];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = 4 * (t + NT * j);
    *reinterpret_cast<float4*>(&buf[swz(i)]) = make_float4(v[j * 4], v[j * 4 + 1], v[j * 4 + 2], v[j * 4 + 3]);
  }
  __syncthreads();
  // pass 2: bits 2..5 in registers; thread bits -> index bits {0,1} and {6..LOG2T-1}
  {
    const int fixed = (t & 3) | ((t >> 2) << 6);
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = buf[swz(fixed | (k << 2))];
    butterflies<4>(v, 2, log2h);
#pragma unroll
    for (int k = 0; k < 16; ++k) buf[swz(fixed | (k << 2))] = v[k];
  }
  __syncthreads();
  // pass 3: bits 6..9 in registers; thread bits -> index bits {0..5} and {10..LOG2T-1}
  {
    const int fixed = (t & 63) | ((t >> 6) << 10);
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = buf[swz(fixed | (k << 6))];
    butterflies<4>(v, 6, log2h);
    if constexpr (LOG2T == 12) {
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int i = fixed | (k << 6);
        if (i < valid) snk.store(base + i, v[k]);
      }
    } else {
#pragma unroll
      for (int k = 0; k < 16; ++k) buf[swz(fixed | (k << 6))] = v[k];
    }
  }
  if constexpr (LOG2T > 12) {
    __syncthreads();
    // pass 4: the remaining bits 10 .. LOG2T-3. Registers <-> index bits {LOG2T-4 .. LOG2T-1} (for
    // T = 8192 that is {9, 10, 11, 12}: bit 9 only picks a second group), thread bits <-> the rest.
    constexpr int kLow = LOG2T - 4;               // the threads cover index bits 0 .. kLow-1
    const int fixed = t;                          // NT = 2^kLow threads
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = buf[swz(fixed | (k << kLow))];
    {
      // register bit (10 - kLow) is index bit 10
      constexpr int shift = 10 - kLow;            // 1 for T = 8192, 0 for T = 16384
      float w[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) w[k] = v[((k << shift) | (k >> (4 - shift))) & 15];   // rotate index bit 10 down to bit 0
      butterflies<LOG2T - 12>(w, 10, log2h);
#pragma unroll
      for (int k = 0; k < 16; ++k) v[((k << shift) | (k >> (4 - shift))) & 15] = w[k];
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int i = fixed | (k << kLow);
      if (i < valid) snk.store(base + i, v[k]);
    }
  }
}

// ---- out = reference - dequant(target) * multiplier[e % d] (MUL), or the plain delta ------------------------------
// Grid-stride. `vec`: d % 4 == 0 and reference, multiplier and out are 16-byte aligned, so a thread takes whole quads
// (which never straddle a row): one packed target load where the scale view allows (TargetSource), 16-byte loads of
// the reference and the multiplier, one 16-byte store. The float32 product is rounded, then subtracted
// (-ffp-contract=off: two operations).
template <bool MUL>
__global__ __launch_bounds__(256) void weight_delta_scaled_kernel(TargetSource src, DeltaSink snk,
                                                                 const float* __restrict__ multiplier, long long d,
                                                                 int vec) {
  const long long step = static_cast<long long>(gridDim.x) * 256;
  const long long first = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  const long long n = src.p.n;
  if (vec) {
    for (long long e = 4 * first; e < n; e += 4 * step) {
      float4 v = src.load4(e);
      if (MUL) {
        const float4 m = *reinterpret_cast<const float4*>(multiplier + e % d);
        v = make_float4(v.x * m.x, v.y * m.y, v.z * m.z, v.w * m.w);
      }
      snk.store4(e, v);
    }
  } else {
    for (long long e = first; e < n; e += step) {
      float v = src.load(e);
      if (MUL) v = v * multiplier[e % d];
      snk.store(e, v);
    }
  }
}

}  // namespace
}  // namespace mi355q

using namespace mi355q;

extern "C" int32_t mi355q_hadamard_rotate_f32(const float* x, int64_t n_vec, int32_t h, float* out,
                                              void* stream) {
  clear_error();
  if (n_vec < 0) return fail(MI355Q_BAD_ARG, "negative vector count");
  if (h <= 0 || (h & (h - 1)) != 0)
    return fail(MI355Q_BAD_ARG, "Hadamard matrix size must be a power of 2. ");
  if (h > 16384) return fail(MI355Q_UNSUPPORTED, "hadamard size > 16384 does not fit one LDS tile");
  if (n_vec == 0) return MI355Q_OK;
  if (!x || !out) return fail(MI355Q_BAD_ARG, "null pointer");
  int log2h = 0;
  while ((1 << log2h) < h) ++log2h;
  // |H entry| of the reference: int8(1) / np.sqrt(h, dtype=float32)
  const float r = 1.0f / __builtin_sqrtf(static_cast<float>(h));
  const long long total = n_vec * static_cast<long long>(h);
  const FloatSource src{x};
  const FloatSink snk{out};
  if (h >= 256 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0) {
    const int tile = h <= kTile ? kTile : h;   // 4096, 8192 or 16384 elements per workgroup
    const long long tiles = (total + tile - 1) / tile;
    if (tiles > 0x7FFFFFFFLL) return fail(MI355Q_UNSUPPORTED, "too many vectors");
    const dim3 grid(static_cast<unsigned>(tiles));
    if (tile == 4096)
      hipLaunchKernelGGL((fwht_tile_kernel<12, FloatSource, FloatSink>), grid, dim3(256), 0, as_stream(stream), src, snk, total, log2h, r);
    else if (tile == 8192)
      hipLaunchKernelGGL((fwht_tile_kernel<13, FloatSource, FloatSink>), grid, dim3(512), 0, as_stream(stream), src, snk, total, log2h, r);
    else
      hipLaunchKernelGGL((fwht_tile_kernel<14, FloatSource, FloatSink>), grid, dim3(1024), 0, as_stream(stream), src, snk, total, log2h, r);
    MI355Q_CHECK_LAUNCH("hadamard launch");
    return MI355Q_OK;
  }
  int vecs = h >= 2048 ? 1 : 2048 / h;
  if (vecs > n_vec) vecs = static_cast<int>(n_vec);
  const size_t smem = static_cast<size_t>(vecs) * h * sizeof(float);
  const long long blocks = (n_vec + vecs - 1) / vecs;
  if (blocks > 0x7FFFFFFFLL) return fail(MI355Q_UNSUPPORTED, "too many vectors");
  hipLaunchKernelGGL((fwht_kernel<FloatSource, FloatSink>), dim3(static_cast<unsigned>(blocks)), dim3(256), smem,
                     as_stream(stream), src, snk, static_cast<long long>(n_vec), h, log2h, vecs, r);
  MI355Q_CHECK_LAUNCH("hadamard launch");
  return MI355Q_OK;
}

extern "C" int32_t mi355q_weight_delta_transformed_f32(const float* reference, const void* target, int64_t n,
                                                       int32_t target_kind, int32_t diff_bits, int64_t channels,
                                                       int64_t inner, const float* scale, const int32_t* zero_point,
                                                       int64_t d, const float* multiplier, int32_t hadamard_size,
                                                       float* delta_out, void* stream) {
  clear_error();
  if (n < 0) return fail(MI355Q_BAD_ARG, "negative element count");
  if (d < 1) return fail(MI355Q_BAD_ARG, "d must be >= 1");
  if (n % d != 0) return fail(MI355Q_BAD_ARG, "the element count is not a multiple of the row length d");
  const int32_t h = hadamard_size;
  if (h < 0 || (h & (h - 1)) != 0) return fail(MI355Q_BAD_ARG, "Hadamard matrix size must be a power of 2. ");
  if (h > 1 && multiplier) return fail(MI355Q_UNSUPPORTED, "a multiplier and a rotation at once");
  if (h > 16384) return fail(MI355Q_BAD_ARG, "hadamard size > 16384 does not fit one LDS tile");
  if (h > 1 && d % h != 0) return fail(MI355Q_BAD_ARG, "the Hadamard size does not divide the row length d");
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
  TargetSource src{};
  src.p.reference = reference; src.p.target = target; src.p.n = n; src.p.target_kind = target_kind;
  src.p.diff_bits = diff_bits; src.p.channels = channels; src.p.inner = inner; src.p.scale = scale;
  src.p.zero_point = zero_point;
  src.packed = (target_kind == MI355Q_CMP_I8 || target_kind == MI355Q_CMP_I4 || target_kind == MI355Q_CMP_I2) &&
               (channels == 1 || inner % 4 == 0) && (reinterpret_cast<uintptr_t>(target) & 3) == 0;
  const DeltaSink snk{reference, delta_out};
  hipStream_t st = as_stream(stream);
  if (h <= 1) {
    const int vec = d % 4 == 0 && ((reinterpret_cast<uintptr_t>(reference) | reinterpret_cast<uintptr_t>(delta_out) |
                                    reinterpret_cast<uintptr_t>(multiplier)) & 15) == 0;
    const int64_t work = vec ? n / 4 : n, blocks = (work + 255) / 256;
    const dim3 grid(static_cast<unsigned>(blocks < (1 << 20) ? blocks : (1 << 20)));
    if (multiplier)
      hipLaunchKernelGGL(weight_delta_scaled_kernel<true>, grid, dim3(256), 0, st, src, snk, multiplier,
                         static_cast<long long>(d), vec);
    else
      hipLaunchKernelGGL(weight_delta_scaled_kernel<false>, grid, dim3(256), 0, st, src, snk, multiplier,
                         static_cast<long long>(d), vec);
    MI355Q_CHECK_LAUNCH("transformed weight delta launch");
    return MI355Q_OK;
  }
  // The route depends on h alone (the network that rotated the weight): alignment only picks the access width.
  int log2h = 0;
  while ((1 << log2h) < h) ++log2h;
  const float r = 1.0f / __builtin_sqrtf(static_cast<float>(h));
  const long long total = n, n_vec = n / h;
  if (h >= 256) {
    const int tile = h <= kTile ? kTile : h;
    const long long tiles = (total + tile - 1) / tile;
    if (tiles > 0x7FFFFFFFLL) return fail(MI355Q_UNSUPPORTED, "too many vectors");
    const dim3 grid(static_cast<unsigned>(tiles));
    if (tile == 4096)
      hipLaunchKernelGGL((fwht_tile_kernel<12, TargetSource, DeltaSink>), grid, dim3(256), 0, st, src, snk, total, log2h, r);
    else if (tile == 8192)
      hipLaunchKernelGGL((fwht_tile_kernel<13, TargetSource, DeltaSink>), grid, dim3(512), 0, st, src, snk, total, log2h, r);
    else
      hipLaunchKernelGGL((fwht_tile_kernel<14, TargetSource, DeltaSink>), grid, dim3(1024), 0, st, src, snk, total, log2h, r);
    MI355Q_CHECK_LAUNCH("transformed weight delta launch");
    return MI355Q_OK;
  }
  int vecs = 2048 / h;
  if (vecs > n_vec) vecs = static_cast<int>(n_vec);
  const size_t smem = static_cast<size_t>(vecs) * h * sizeof(float);
  const long long blocks = (n_vec + vecs - 1) / vecs;
  if (blocks > 0x7FFFFFFFLL) return fail(MI355Q_UNSUPPORTED, "too many vectors");
  hipLaunchKernelGGL((fwht_kernel<TargetSource, DeltaSink>), dim3(static_cast<unsigned>(blocks)), dim3(256), smem, st,
                     src, snk, n_vec, h, log2h, vecs, r);
  MI355Q_CHECK_LAUNCH("transformed weight delta launch");
  return MI355Q_OK;
}
