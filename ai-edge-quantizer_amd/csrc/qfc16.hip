// Integer execution of a FULLY_CONNECTED op that reads an INT16 activation (include/mi355q.h, "Integer execution,
// int16 activations"): acc = Xq W^^T exact in int64, y = fl32(double(acc) * double(fl32(s_x * s_w))).
//
//   qfc16_mfma_kernel     the main loop of qfc_tile.h, written out for int16 activations: a lane's A fragment is 16 consecutive
//                         int16 of a row of Xq (two 16-byte loads), split there into a high-byte and a biased low-byte
//                         int8 fragment; its B fragment is what qfc.hip's is, read and unpacked ONCE per step and fed
//                         to both planes. A wave owns 32 tokens x 64 output channels = 2 x 4 MFMA tiles in two planes,
//                         a workgroup 64 x 128. This file adds the epilogue: the two int32 planes and 128 Sum_k w
//                         (weight_sums_kernel's, qfc_frag.h, per row or per block) meet in int64, then the rescale.
//   qfc16_generic_kernel  one thread per output with an int64 accumulator: every other shape and alignment, same bits.
#include "common.h"
#include "compare_target.h"
#include "qfc_tile.h"

namespace mi355q {
namespace {

constexpr int kThreads = kQfcThreads;

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

// qfc_tile.h's main loop, written out for the two int16 planes (ah, al): compiled through qfc_main_loop the code
// around the loop came out differently and qfc_output_i16 measured 6.8 % slower at 4096 x 4096, so this kernel and
// qfc_out16_mfma_kernel keep the text that compiles to what they were. grid: x = output-channel tiles, y = token tiles.
template <int KIND, int KSTEP, bool BLOCKWISE>
__global__ __launch_bounds__(kThreads) void qfc16_mfma_kernel(Fwd16Args g) {
  using XF = Act<int16_t, KSTEP>;
  using T = QfcTile<int16_t>;
  constexpr int TA = T::TA;
  using RW = RawW<KIND, KSTEP>;
  using Frag = typename FragOf<KSTEP>::T;
  constexpr int E = KSTEP / 4;     // consecutive elements per lane and step
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const long long t0 = static_cast<long long>(blockIdx.y) * T::BTA + (wave >> 1) * T::WTA;
  const long long r0 = static_cast<long long>(blockIdx.x) * T::BTB + (wave & 1) * T::WTB;
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
  typename XF::Raw xc[TA], xn[TA];
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
    Frag wf[TB], xs[TA][2];      // xs[a]: the high and the biased low plane
#pragma unroll
    for (int b = 0; b < TB; ++b) wf[b] = RW::unpack(wc[b]);      // once, for both planes
#pragma unroll
    for (int a = 0; a < TA; ++a) XF::frags(xc[a], xs[a]);
#pragma unroll
    for (int a = 0; a < TA; ++a)
#pragma unroll
      for (int b = 0; b < TB; ++b) {
        ah[a][b] = mfma_i8<KSTEP>(xs[a][0], wf[b], ah[a][b]);
        al[a][b] = mfma_i8<KSTEP>(xs[a][1], wf[b], al[a][b]);
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
    const float s_x = g.x_scale[g.x_per_row ? t : 0];
    float y = 0.0f;
    for (int b = 0; b < g.nblocks; ++b) {
      const long long acc =
          qfc_dot<long long>(g.xq + t * g.d, g.w, g.kind, r * g.d, static_cast<long long>(b) * g.block, g.block, 0);
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
  return wsum_workspace(rows, block > 0 ? d / block : 1);
}

extern "C" int32_t mi355q_qfc_forward_i16(const int16_t* xq, int64_t n, int64_t d, const float* x_scale,
                                          int64_t x_scale_count, const void* w, int32_t w_kind, int64_t rows,
                                          const float* w_scale, int64_t w_scale_count, int32_t block, float* y_out,
                                          int64_t* acc_out, void* workspace, size_t workspace_bytes, void* stream) {
  clear_error();
  if (n < 0 || d < 0 || rows < 0) return fail(MI355Q_BAD_ARG, "negative shape");
  if (!xq || !x_scale || !w || !w_scale || !y_out) return fail(MI355Q_BAD_ARG, "null pointer");
  if (const int32_t bad = check_weight_kind(w_kind)) return bad;
  if (const int32_t bad = check_block(block, d)) return bad;
  bool blockwise;
  if (const int32_t bad = check_scale_counts(n, rows, d, block, x_scale_count, w_scale_count, acc_out != nullptr, &blockwise))
    return bad;
  if (d > kQfcMaxD)
    return fail(MI355Q_UNSUPPORTED, "d = %lld exceeds %d (the int32 planes of the accumulator)", static_cast<long long>(d), kQfcMaxD);
  // the weight sums are a term of every accumulator: the workspace is always read
  const int64_t nblocks = blockwise ? d / block : 1;
  if (const int32_t bad = check_workspace(workspace, workspace_bytes, (rows > 0 && d > 0) ? wsum_workspace(rows, nblocks) : 0))
    return bad;
  if (n == 0 || rows == 0) return MI355Q_OK;
  if (d == 0) return fail(MI355Q_BAD_ARG, "d must be >= 1");
  dim3 grid;
  if (const int32_t bad = tile_grid<int16_t>(n, rows, &grid)) return bad;

  Fwd16Args g{};
  g.xq = xq; g.w = static_cast<const uint8_t*>(w); g.x_scale = x_scale; g.w_scale = w_scale;
  g.wsum = static_cast<const int32_t*>(workspace); g.y = y_out; g.acc = reinterpret_cast<long long*>(acc_out);
  g.n = n; g.rows = rows; g.d = d; g.x_per_row = x_scale_count != 1 ? 1 : 0;
  g.w_mode = blockwise ? 2 : (w_scale_count == rows && rows != 1) ? 1 : 0;
  g.nblocks = static_cast<int>(nblocks);
  g.block = blockwise ? block : static_cast<int>(d);
  g.kind = w_kind;
  hipStream_t st = as_stream(stream);

  if (mfma_route(xq, w, d, blockwise && block == 32 ? 32 : 64)) {
    const int32_t st_sums = launch_weight_sums(g.w, w_kind, rows * g.nblocks, static_cast<long long>(g.block),
                                               static_cast<int32_t*>(workspace), st);
    if (st_sums != MI355Q_OK) return st_sums;
    dispatch_kind(w_kind, [&](auto kind) { launch_mfma16<decltype(kind)::value>(g, blockwise, grid, st); });
  } else {      // (the generic kernel's int64 accumulator needs no weight sums)
    hipLaunchKernelGGL(qfc16_generic_kernel, dim3(generic_blocks(n * rows)), dim3(kThreads), 0, st, g);
  }
  MI355Q_CHECK_LAUNCH("int16 fully-connected launch");
  return MI355Q_OK;
}
