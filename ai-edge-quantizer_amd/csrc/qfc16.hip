// Integer execution of a FULLY_CONNECTED op that reads an INT16 activation (include/mi355q.h, "Integer execution,
// int16 activations"): acc = Xq W^^T exact in int64, y = fl32(double(acc) * double(fl32(s_x * s_w))).
//
// gfx950 has no int16 matrix instruction, so an activation is split into two int8 planes in registers:
//   x = 256 h + l_u,  h = x >> 8 (arithmetic, -128 .. 127),  l_u = x & 255,  l_s = int8(l_u ^ 0x80) = l_u - 128
//   acc = 256 Sum h w + Sum l_s w + 128 Sum_k w
// Each of the first two sums stays within 65536 * 128 * 128 = 2^30 for d <= 65536 and runs on the int8 matrix cores;
// the third is weight_sums_kernel's (qfc_frag.h), per row or per block, and the three meet in int64 in the epilogue.
//
//   qfc16_mfma_kernel     a lane's A fragment is 16 consecutive int16 of a row of Xq (two 16-byte loads), split into a
//                         high-byte and a biased low-byte fragment with two v_perm_b32 per word pair; its B fragment is
//                         what qfc.hip's is, read and unpacked ONCE per step and fed to both planes. A wave owns
//                         32 tokens x 64 output channels = 2 x 4 MFMA tiles in two planes: 2 + 4 fragment loads feed
//                         16 v_mfma_i32_16x16x64_i8 (v_mfma_i32_16x16x32_i8 for block 32); a workgroup is 64 x 128.
//   qfc16_generic_kernel  one thread per output with an int64 accumulator: every other shape and alignment, same bits.
#include "common.h"
#include "compare_target.h"
#include "qfc_frag.h"

namespace mi355q {
namespace {

constexpr int kThreads = kQfcThreads;
constexpr int kMaxD = 65536;           // each int32 plane: d * 128 * 128 <= 2^30

struct Fwd16Args {
  const int16_t* xq;       // [n, d]
  const uint8_t* w;        // [rows, d] stored
  const float* x_scale;    // 1 or n
  const float* w_scale;    // 1, rows or rows * nblocks
  const int32_t* wsum;     // [rows, nblocks]
  float* y;                // [n, rows]
  long long* acc;          // [n, rows] or null
  long long n, rows, d;
  int x_per_row;           // x_scale has n entries
  int w_mode;              // 0 per tensor, 1 per channel, 2 blockwise
  int nblocks;             // blocks per weight row (1 unless blockwise)
  int block;               // elements per block (d unless blockwise)
  int kind;
};

// fl32(double(acc) * double(sc)): the int64 accumulator is exact in float64 (|acc| < 2^39)
__device__ __forceinline__ float rescale(long long acc, float sc) {
  return static_cast<float>(static_cast<double>(acc) * static_cast<double>(sc));
}

// The two int32 planes and the weight sum as one exact integer.
__device__ __forceinline__ long long combine(int hi, int lo, int wsum) {
  return 256LL * hi + lo + 128LL * wsum;
}

// Words x0 = (v0, v1), x1 = (v2, v3) of four consecutive int16 (the earlier one in the low half) -> the word of their
// four high bytes, and the word of their four low bytes with the top bit flipped (l_u - 128 as int8). One v_perm_b32 each.
// (v_perm_b32 D, S0, S1, sel: selector values 0 .. 3 pick the bytes of S1, 4 .. 7 those of S0.)
__device__ __forceinline__ int high_bytes(int x0, int x1) {
  return static_cast<int>(__builtin_amdgcn_perm(static_cast<uint32_t>(x1), static_cast<uint32_t>(x0), 0x07050301u));
}
__device__ __forceinline__ int low_bytes_biased(int x0, int x1) {
  return static_cast<int>(__builtin_amdgcn_perm(static_cast<uint32_t>(x1), static_cast<uint32_t>(x0), 0x06040200u) ^
                          0x80808080u);
}

// A lane's KSTEP / 4 consecutive int16 activations and their two int8 fragments.
template <int KSTEP> struct X16;
template <> struct X16<64> {
  struct T { I32x4 a, b; };      // k = 0 .. 7 and 8 .. 15 of the lane's 16
  static __device__ __forceinline__ T load(const int16_t* p) {
    const I32x4* q = reinterpret_cast<const I32x4*>(p);
    return T{q[0], q[1]};
  }
  static __device__ __forceinline__ T zero() { return T{I32x4{0, 0, 0, 0}, I32x4{0, 0, 0, 0}}; }
  static __device__ __forceinline__ I32x4 mfma(I32x4 a, I32x4 b, I32x4 c) {
    return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ void split(const T& r, I32x4& hi, I32x4& lo) {
    hi = I32x4{high_bytes(r.a[0], r.a[1]), high_bytes(r.a[2], r.a[3]), high_bytes(r.b[0], r.b[1]), high_bytes(r.b[2], r.b[3])};
    lo = I32x4{low_bytes_biased(r.a[0], r.a[1]), low_bytes_biased(r.a[2], r.a[3]), low_bytes_biased(r.b[0], r.b[1]),
               low_bytes_biased(r.b[2], r.b[3])};
  }
};
template <> struct X16<32> {
  using T = I32x4;               // the lane's 8
  static __device__ __forceinline__ T load(const int16_t* p) { return *reinterpret_cast<const I32x4*>(p); }
  static __device__ __forceinline__ T zero() { return I32x4{0, 0, 0, 0}; }
  static __device__ __forceinline__ I32x4 mfma(long a, long b, I32x4 c) {
    return __builtin_amdgcn_mfma_i32_16x16x32_i8(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ void split(const T& r, long& hi, long& lo) {
    hi = two_words(high_bytes(r[0], r[1]), high_bytes(r[2], r[3]));
    lo = two_words(low_bytes_biased(r[0], r[1]), low_bytes_biased(r[2], r[3]));
  }
};

constexpr int MF = 16;             // MFMA tile edge
constexpr int TA = 2;              // MFMA tiles per wave along tokens (each in two planes)
constexpr int TB = 4;              // MFMA tiles per wave along output channels
constexpr int WTA = TA * MF;       // a wave's tokens (32)
constexpr int WTB = TB * MF;       // a wave's output channels (64)
constexpr int BTA = 2 * WTA;       // a workgroup's tokens (2 x 2 waves)
constexpr int BTB = 2 * WTB;       // a workgroup's output channels

// MFMA route: d % KSTEP == 0, xq and w 16-byte aligned (so every fragment load is aligned to its own size).
// grid: x = output-channel tiles, y = token tiles.
template <int KIND, int KSTEP, bool BLOCKWISE>
__global__ __launch_bounds__(kThreads) void qfc16_mfma_kernel(Fwd16Args g) {
  using XF = X16<KSTEP>;
  using RW = RawW<KIND, KSTEP>;
  using Frag = typename FragOf<KSTEP>::T;
  constexpr int E = KSTEP / 4;     // consecutive elements per lane and step
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const long long t0 = static_cast<long long>(blockIdx.y) * BTA + (wave >> 1) * WTA;
  const long long r0 = static_cast<long long>(blockIdx.x) * BTB + (wave & 1) * WTB;
  if (t0 >= g.n || r0 >= g.rows) return;     // (the whole wave; the kernel has no barrier)
  const int fr = lane & 15, fg = lane >> 4;

  const int16_t* xp[TA];
  long long we[TB];
  bool xok[TA], wok[TB];
#pragma unroll
  for (int a = 0; a < TA; ++a) {
    const long long t = t0 + a * MF + fr;
    xok[a] = t < g.n;
    xp[a] = g.xq + (xok[a] ? t : 0) * g.d + fg * E;
  }
#pragma unroll
  for (int b = 0; b < TB; ++b) {
    const long long r = r0 + b * MF + fr;
    wok[b] = r < g.rows;
    we[b] = (wok[b] ? r : 0) * g.d + fg * E;
  }

  I32x4 ah[TA][TB], al[TA][TB];
  float yf[TA][TB][4];
#pragma unroll
  for (int a = 0; a < TA; ++a)
#pragma unroll
    for (int b = 0; b < TB; ++b) {
      ah[a][b] = I32x4{0, 0, 0, 0};
      al[a][b] = I32x4{0, 0, 0, 0};
#pragma unroll
      for (int i = 0; i < 4; ++i) yf[a][b][i] = 0.0f;
    }
  float sx[TA][4];
  if (BLOCKWISE) {
#pragma unroll
    for (int a = 0; a < TA; ++a)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long long t = t0 + a * MF + fg * 4 + i;
        sx[a][i] = t < g.n ? g.x_scale[g.x_per_row ? t : 0] : 0.0f;
      }
  }

  const int steps = static_cast<int>(g.d / KSTEP);
  const int steps_per_block = BLOCKWISE ? g.block / KSTEP : steps;
  typename XF::T xc[TA], xn[TA];
  typename RW::T wc[TB], wn[TB];
#pragma unroll
  for (int a = 0; a < TA; ++a) xc[a] = xok[a] ? XF::load(xp[a]) : XF::zero();
#pragma unroll
  for (int b = 0; b < TB; ++b) wc[b] = wok[b] ? RW::load(g.w, we[b]) : RW::zero();
  int in_block = 0, bi = 0;
  for (int s = 0; s < steps; ++s) {
    if (s + 1 < steps) {     // the next step's fragments fly while this step's MFMAs run
      const long long k = static_cast<long long>(s + 1) * KSTEP;
#pragma unroll
      for (int a = 0; a < TA; ++a) xn[a] = xok[a] ? XF::load(xp[a] + k) : XF::zero();
#pragma unroll
      for (int b = 0; b < TB; ++b) wn[b] = wok[b] ? RW::load(g.w, we[b] + k) : RW::zero();
    }
    Frag wf[TB], xh[TA], xl[TA];
#pragma unroll
    for (int b = 0; b < TB; ++b) wf[b] = RW::unpack(wc[b]);      // once, for both planes
#pragma unroll
    for (int a = 0; a < TA; ++a) XF::split(xc[a], xh[a], xl[a]);
#pragma unroll
    for (int a = 0; a < TA; ++a)
#pragma unroll
      for (int b = 0; b < TB; ++b) {
        ah[a][b] = XF::mfma(xh[a], wf[b], ah[a][b]);
        al[a][b] = XF::mfma(xl[a], wf[b], al[a][b]);
      }
#pragma unroll
    for (int a = 0; a < TA; ++a) xc[a] = xn[a];
#pragma unroll
    for (int b = 0; b < TB; ++b) wc[b] = wn[b];
    if (BLOCKWISE && ++in_block == steps_per_block) {
      // p_b = fl32(double(acc_b) * double(fl(s_x * s_w[r, b]))), y = y + p_b: blocks in ascending order, no FMA
#pragma unroll
      for (int b = 0; b < TB; ++b) {
        const long long r = r0 + b * MF + fr;
        const bool rok = r < g.rows;
        const float sw = rok ? g.w_scale[r * g.nblocks + bi] : 0.0f;
        const int ws = rok ? g.wsum[r * g.nblocks + bi] : 0;
#pragma unroll
        for (int a = 0; a < TA; ++a)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float sc = sx[a][i] * sw;
            const float p = rescale(combine(ah[a][b][i], al[a][b][i], ws), sc);
            yf[a][b][i] = yf[a][b][i] + p;
            ah[a][b][i] = 0;
            al[a][b][i] = 0;
          }
      }
      in_block = 0;
      ++bi;
    }
  }

  // C / D map of the 16x16 MFMAs: column (output channel) = lane & 15, row (token) = 4 (lane >> 4) + register
#pragma unroll
  for (int b = 0; b < TB; ++b) {
    const long long r = r0 + b * MF + fr;
    if (r >= g.rows) continue;
    float sw = 0.0f;
    int ws = 0;
    if (!BLOCKWISE) {
      sw = g.w_scale[g.w_mode == 1 ? r : 0];
      ws = g.wsum[r];
    }
#pragma unroll
    for (int a = 0; a < TA; ++a)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long long t = t0 + a * MF + fg * 4 + i;
        if (t >= g.n) continue;
        if (BLOCKWISE) {
          g.y[t * g.rows + r] = yf[a][b][i];
        } else {
          const long long v = combine(ah[a][b][i], al[a][b][i], ws);
          const float sc = g.x_scale[g.x_per_row ? t : 0] * sw;
          g.y[t * g.rows + r] = rescale(v, sc);
          if (g.acc) g.acc[t * g.rows + r] = v;
        }
      }
  }
}

// Generic route: one thread per output element, one weight element at a time, the accumulator in int64.
__global__ __launch_bounds__(kThreads) void qfc16_generic_kernel(Fwd16Args g) {
  const long long total = g.n * g.rows, step = static_cast<long long>(gridDim.x) * kThreads;
  for (long long o = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; o < total; o += step) {
    const long long t = o / g.rows, r = o % g.rows;
    const int16_t* xr = g.xq + t * g.d;
    const float s_x = g.x_scale[g.x_per_row ? t : 0];
    float y = 0.0f;
    for (int b = 0; b < g.nblocks; ++b) {
      long long acc = 0;
      const long long k0 = static_cast<long long>(b) * g.block;
      for (long long k = k0; k < k0 + g.block; ++k)
        acc += static_cast<long long>(static_cast<int>(xr[k]) * weight_element(g.w, g.kind, r * g.d + k));
      if (g.w_mode == 2) {
        const float sc = s_x * g.w_scale[r * g.nblocks + b];
        const float p = rescale(acc, sc);
        y = y + p;
      } else {
        const float sc = s_x * g.w_scale[g.w_mode == 1 ? r : 0];
        y = rescale(acc, sc);
        if (g.acc) g.acc[o] = acc;
      }
    }
    g.y[o] = y;
  }
}

size_t fwd16_workspace(int64_t rows, int64_t d, int32_t block) {
  const size_t nblocks = block > 0 ? static_cast<size_t>(d / block) : 1;
  return (static_cast<size_t>(rows) * nblocks * sizeof(int32_t) + 255) & ~static_cast<size_t>(255);
}

template <int KIND>
void launch_mfma16(const Fwd16Args& g, bool blockwise, dim3 grid, hipStream_t st) {
  if (!blockwise) hipLaunchKernelGGL((qfc16_mfma_kernel<KIND, 64, false>), grid, dim3(kThreads), 0, st, g);
  else if (g.block == 32) hipLaunchKernelGGL((qfc16_mfma_kernel<KIND, 32, true>), grid, dim3(kThreads), 0, st, g);
  else hipLaunchKernelGGL((qfc16_mfma_kernel<KIND, 64, true>), grid, dim3(kThreads), 0, st, g);
}

}  // namespace
}  // namespace mi355q

using namespace mi355q;

extern "C" size_t mi355q_qfc_forward_i16_workspace_bytes(int64_t rows, int64_t d, int32_t block) {
  if (rows <= 0 || d <= 0 || block < 0 || (block > 0 && d % block)) return 0;
  return fwd16_workspace(rows, d, block);
}

extern "C" int32_t mi355q_qfc_forward_i16(const int16_t* xq, int64_t n, int64_t d, const float* x_scale,
                                          int64_t x_scale_count, const void* w, int32_t w_kind, int64_t rows,
                                          const float* w_scale, int64_t w_scale_count, int32_t block, float* y_out,
                                          int64_t* acc_out, void* workspace, size_t workspace_bytes, void* stream) {
  clear_error();
  if (n < 0 || d < 0 || rows < 0) return fail(MI355Q_BAD_ARG, "negative shape");
  if (!xq || !x_scale || !w || !w_scale || !y_out) return fail(MI355Q_BAD_ARG, "null pointer");
  if (w_kind != MI355Q_CMP_I8 && w_kind != MI355Q_CMP_I4 && w_kind != MI355Q_CMP_I2)
    return fail(MI355Q_BAD_ARG, "weight kind %d is not I8, I4 or I2", w_kind);
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
  if (d > kMaxD)
    return fail(MI355Q_UNSUPPORTED, "d = %lld exceeds %d (the int32 planes of the accumulator)", static_cast<long long>(d), kMaxD);
  // the weight sums are a term of every accumulator: the workspace is always read
  const size_t need = (rows > 0 && d > 0) ? fwd16_workspace(rows, d, blockwise ? block : 0) : 0;
  if (need > 0 && (!workspace || workspace_bytes < need))
    return fail(MI355Q_BAD_ARG, "workspace of %zu bytes is smaller than the %zu needed", workspace ? workspace_bytes : size_t{0}, need);
  if (n == 0 || rows == 0) return MI355Q_OK;
  if (d == 0) return fail(MI355Q_BAD_ARG, "d must be >= 1");
  const int64_t row_tiles = (rows + BTB - 1) / BTB, tok_tiles = (n + BTA - 1) / BTA;
  if (row_tiles > 0x7FFFFFFFLL || tok_tiles > 65535) return fail(MI355Q_UNSUPPORTED, "too many tiles for one launch");

  Fwd16Args g{};
  g.xq = xq; g.w = static_cast<const uint8_t*>(w); g.x_scale = x_scale; g.w_scale = w_scale;
  g.wsum = static_cast<const int32_t*>(workspace); g.y = y_out; g.acc = reinterpret_cast<long long*>(acc_out);
  g.n = n; g.rows = rows; g.d = d; g.x_per_row = x_scale_count != 1 ? 1 : 0;
  g.w_mode = blockwise ? 2 : (w_scale_count == rows && rows != 1) ? 1 : 0;
  g.nblocks = blockwise ? static_cast<int>(nblocks) : 1;
  g.block = blockwise ? block : static_cast<int>(d);
  g.kind = w_kind;
  hipStream_t st = as_stream(stream);

  const int kstep = blockwise && block == 32 ? 32 : 64;
  const bool mfma = d % kstep == 0 && reinterpret_cast<uintptr_t>(xq) % 16 == 0 && reinterpret_cast<uintptr_t>(w) % 16 == 0;
  if (mfma) {
    const int32_t st_sums = launch_weight_sums(g.w, w_kind, rows * g.nblocks, static_cast<long long>(g.block),
                                               static_cast<int32_t*>(workspace), st);
    if (st_sums != MI355Q_OK) return st_sums;
    const dim3 grid(static_cast<unsigned>(row_tiles), static_cast<unsigned>(tok_tiles));
    if (w_kind == MI355Q_CMP_I8) launch_mfma16<MI355Q_CMP_I8>(g, blockwise, grid, st);
    else if (w_kind == MI355Q_CMP_I4) launch_mfma16<MI355Q_CMP_I4>(g, blockwise, grid, st);
    else launch_mfma16<MI355Q_CMP_I2>(g, blockwise, grid, st);
  } else {      // (the generic kernel's int64 accumulator needs no weight sums)
    const long long total = n * rows, blocks = (total + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(qfc16_generic_kernel, dim3(static_cast<unsigned>(blocks < (1 << 20) ? blocks : (1 << 20))),
                       dim3(kThreads), 0, st, g);
  }
  MI355Q_CHECK_LAUNCH("int16 fully-connected launch");
  return MI355Q_OK;
}
