// Integer execution of a static FULLY_CONNECTED op through to its stored output (include/mi355q.h, "Integer
// execution, through to the stored output"): accumulator + bias, fixed-point multiplier, output zero point, the fused
// activation's integer range, int8 / int16 store. No [n, rows] accumulator or float array exists: the MFMA kernels
// run the epilogue on the accumulator tile in registers and store q_out alone.
//
//   qfc_out_mfma_kernel       the main loop of qfc_tile.h with int8 activations (K = 64, one accumulator per output): a
//                             wave owns 64 tokens x 64 channels = 4 x 4 tiles of v_mfma_i32_16x16x64_i8. In the C / D map a
//                             lane's 4 x 4 x 4 values all belong to the channels r0 + 16 b + (lane & 15), b = 0 .. 3: bias,
//                             multiplier and shift are read once per b and serve 16 outputs each.
//   qfc_out16_mfma_kernel     the same loop for int16 activations (two int8 planes, 32 tokens x 64 channels per
//                             wave), written out here as in qfc16.hip; combined with 128 Sum w in int64 in the epilogue.
//   qfc_out_generic_kernel,
//   qfc_out16_generic_kernel  one thread per output, element by element: every other shape and alignment, same bits.
// The two fixed-point epilogues are qfc_epilogue.h's (dwconv.hip runs them too); qfc.hip and qfc16.hip hold the float ones.
#include "common.h"
#include "compare_target.h"
#include "qfc_epilogue.h"
#include "qfc_tile.h"

namespace mi355q {
namespace {

constexpr int kThreads = kQfcThreads;

// ---------------------------------------------------------------- int8 activations
template <int KIND>
__global__ __launch_bounds__(kThreads) void qfc_out_mfma_kernel(OutArgs g) {
  QfcWave wv;
  if (!qfc_wave<int8_t>(wv, g.n, g.rows)) return;
  I32x4 acc[QfcTile<int8_t>::TM][TB];
  qfc_main_loop<int8_t, KIND, 64>(wv, static_cast<const int8_t*>(g.xq), g.w, g.n, g.rows, g.d, acc);

  struct Chan {
    Chan8 c;
    int corr;      // zp_x * Sum_k q_w[r][k]
  };
  int8_t* q = static_cast<int8_t*>(g.q);
  qfc_walk_outputs<int8_t>(
      wv, g.n, g.rows, [=](long long r) { return Chan{chan8(g, r), g.zp_x != 0 ? g.zp_x * g.wsum[r] : 0}; },
      [=, &acc](const Chan& c, int a, int b, int i, long long t, long long r) {
        q[t * g.rows + r] = output8(acc[a][b][i] - c.corr, c.c, g);
      });
}

// Generic route: one thread per output element, one weight element at a time.
__global__ __launch_bounds__(kThreads) void qfc_out_generic_kernel(OutArgs g) {
  const long long total = g.n * g.rows, step = static_cast<long long>(gridDim.x) * kThreads;
  const int8_t* xq = static_cast<const int8_t*>(g.xq);
  int8_t* q = static_cast<int8_t*>(g.q);
  for (long long o = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; o < total; o += step) {
    const long long t = o / g.rows, r = o % g.rows;
    q[o] = output8(qfc_dot<int>(xq + t * g.d, g.w, g.kind, r * g.d, 0, g.d, g.zp_x), chan8(g, r), g);
  }
}

// ---------------------------------------------------------------- int16 activations
// (the main loop written out, as in qfc16.hip's qfc16_mfma_kernel, which says why)
template <int KIND>
__global__ __launch_bounds__(kThreads) void qfc_out16_mfma_kernel(OutArgs g) {
  using RW = RawW<KIND, 64>;
  using XF = Act<int16_t, 64>;
  using T = QfcTile<int16_t>;
  constexpr int TA = T::TA;
  constexpr int KSTEP = 64, E = KSTEP / 4;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const long long t0 = static_cast<long long>(blockIdx.y) * T::BTA + (wave >> 1) * T::WTA;
  const long long r0 = static_cast<long long>(blockIdx.x) * T::BTB + (wave & 1) * T::WTB;
  if (t0 >= g.n || r0 >= g.rows) return;     // (the whole wave; the kernel has no barrier)
  const int fr = lane & 15, fg = lane >> 4;
  const int16_t* xq = static_cast<const int16_t*>(g.xq);

  const int16_t* xp[TA];
  long long we[TB];
  bool xok[TA], wok[TB];
#pragma unroll
  for (int a = 0; a < TA; ++a) {
    const long long t = t0 + a * MF + fr;
    xok[a] = t < g.n;
    xp[a] = xq + (xok[a] ? t : 0) * g.d + fg * E;
  }
#pragma unroll
  for (int b = 0; b < TB; ++b) {
    const long long r = r0 + b * MF + fr;
    wok[b] = r < g.rows;
    we[b] = (wok[b] ? r : 0) * g.d + fg * E;
  }

  I32x4 ah[TA][TB], al[TA][TB];
#pragma unroll
  for (int a = 0; a < TA; ++a)
#pragma unroll
    for (int b = 0; b < TB; ++b) {
      ah[a][b] = I32x4{0, 0, 0, 0};
      al[a][b] = I32x4{0, 0, 0, 0};
    }

  const int steps = static_cast<int>(g.d / KSTEP);
  typename XF::Raw xc[TA], xn[TA];
  typename RW::T wc[TB], wn[TB];
#pragma unroll
  for (int a = 0; a < TA; ++a) xc[a] = xok[a] ? XF::load(xp[a]) : XF::zero();
#pragma unroll
  for (int b = 0; b < TB; ++b) wc[b] = wok[b] ? RW::load(g.w, we[b]) : RW::zero();
  for (int s = 0; s < steps; ++s) {
    if (s + 1 < steps) {     // the next step's fragments fly while this step's MFMAs run
      const long long k = static_cast<long long>(s + 1) * KSTEP;
#pragma unroll
      for (int a = 0; a < TA; ++a) xn[a] = xok[a] ? XF::load(xp[a] + k) : XF::zero();
#pragma unroll
      for (int b = 0; b < TB; ++b) wn[b] = wok[b] ? RW::load(g.w, we[b] + k) : RW::zero();
    }
    I32x4 wf[TB], xs[TA][2];      // xs[a]: the high and the biased low plane
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
  }

  // C / D map of the 16x16 MFMAs: column (output channel) = lane & 15, row (token) = 4 (lane >> 4) + register
  int16_t* q = static_cast<int16_t*>(g.q);
#pragma unroll
  for (int b = 0; b < TB; ++b) {
    const long long r = r0 + b * MF + fr;
    if (r >= g.rows) continue;
    const Chan16 c = chan16(g, r);
    const long long ws = 128LL * g.wsum[r];
#pragma unroll
    for (int a = 0; a < TA; ++a)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long long t = t0 + a * MF + fg * 4 + i;
        if (t >= g.n) continue;
        q[t * g.rows + r] = output16(256LL * ah[a][b][i] + al[a][b][i] + ws, c, g);
      }
  }
}

// Generic route: one thread per output element, the accumulator in int64 (no weight sums).
__global__ __launch_bounds__(kThreads) void qfc_out16_generic_kernel(OutArgs g) {
  const long long total = g.n * g.rows, step = static_cast<long long>(gridDim.x) * kThreads;
  const int16_t* xq = static_cast<const int16_t*>(g.xq);
  int16_t* q = static_cast<int16_t*>(g.q);
  for (long long o = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; o < total; o += step) {
    const long long t = o / g.rows, r = o % g.rows;
    q[o] = output16(qfc_dot<long long>(xq + t * g.d, g.w, g.kind, r * g.d, 0, g.d, 0), chan16(g, r), g);
  }
}

// What both entries refuse first, in one order.
int32_t check_common(const void* xq, int64_t n, int64_t d, const void* w, int32_t w_kind, int64_t rows,
                     const int32_t* multiplier, const int32_t* shift, int64_t mcount, const void* q_out) {
  if (n < 0 || d < 0 || rows < 0) return fail(MI355Q_BAD_ARG, "negative shape");
  if (!xq || !w || !multiplier || !shift || !q_out) return fail(MI355Q_BAD_ARG, "null pointer");
  if (const int32_t bad = check_weight_kind(w_kind)) return bad;
  if (mcount != 1 && mcount != rows)
    return fail(MI355Q_BAD_ARG, "mcount must be 1 or rows = %lld (got %lld)", static_cast<long long>(rows),
                static_cast<long long>(mcount));
  return MI355Q_OK;
}

}  // namespace
}  // namespace mi355q

using namespace mi355q;

extern "C" size_t mi355q_qfc_output_workspace_bytes(int64_t rows, int64_t d) {
  if (rows <= 0 || d <= 0) return 0;
  return wsum_workspace(rows, 1);
}

extern "C" int32_t mi355q_qfc_output_i8(const int8_t* xq, int64_t n, int64_t d, int32_t x_zero_point, const void* w,
                                        int32_t w_kind, int64_t rows, const int32_t* bias, const int32_t* multiplier,
                                        const int32_t* shift, int64_t mcount, int32_t out_zero_point, int32_t act_min,
                                        int32_t act_max, int8_t* q_out, void* workspace, size_t workspace_bytes,
                                        void* stream) {
  clear_error();
  if (const int32_t bad = check_common(xq, n, d, w, w_kind, rows, multiplier, shift, mcount, q_out)) return bad;
  if (x_zero_point < -128 || x_zero_point > 127)
    return fail(MI355Q_BAD_ARG, "activation zero point %d is outside int8", x_zero_point);
  if (out_zero_point < -128 || out_zero_point > 127)
    return fail(MI355Q_BAD_ARG, "output zero point %d is outside int8", out_zero_point);
  if (act_min > act_max || act_min < -128 || act_max > 127)
    return fail(MI355Q_BAD_ARG, "activation range [%d, %d] is no range within int8", act_min, act_max);
  if (d > kQfcMaxD)
    return fail(MI355Q_UNSUPPORTED, "d = %lld exceeds %d (the int32 accumulator)", static_cast<long long>(d), kQfcMaxD);
  const size_t need = (rows > 0 && d > 0 && x_zero_point != 0) ? wsum_workspace(rows, 1) : 0;
  if (const int32_t bad = check_workspace(workspace, workspace_bytes, need)) return bad;
  if (n == 0 || rows == 0) return MI355Q_OK;
  if (d == 0) return fail(MI355Q_BAD_ARG, "d must be >= 1");
  dim3 grid;
  if (const int32_t bad = tile_grid<int8_t>(n, rows, &grid)) return bad;

  OutArgs g{};
  g.xq = xq; g.w = static_cast<const uint8_t*>(w); g.bias = bias; g.mult = multiplier; g.shift = shift;
  g.wsum = static_cast<const int32_t*>(workspace); g.q = q_out;
  g.n = n; g.rows = rows; g.d = d; g.per_channel = (mcount == rows && rows != 1) ? 1 : 0;
  g.zp_x = x_zero_point; g.zp_y = out_zero_point; g.act_min = act_min; g.act_max = act_max; g.kind = w_kind;
  hipStream_t st = as_stream(stream);

  if (mfma_route(xq, w, d, 64)) {
    if (x_zero_point != 0) {
      const int32_t st_sums = launch_weight_sums(g.w, w_kind, rows, static_cast<long long>(d), static_cast<int32_t*>(workspace), st);
      if (st_sums != MI355Q_OK) return st_sums;
    }
    dispatch_kind(w_kind, [&](auto kind) {
      hipLaunchKernelGGL(qfc_out_mfma_kernel<decltype(kind)::value>, grid, dim3(kThreads), 0, st, g);
    });
  } else {      // (the generic kernel subtracts the zero point element by element: no weight sums)
    hipLaunchKernelGGL(qfc_out_generic_kernel, dim3(generic_blocks(n * rows)), dim3(kThreads), 0, st, g);
  }
  MI355Q_CHECK_LAUNCH("integer fully-connected output launch");
  return MI355Q_OK;
}

extern "C" int32_t mi355q_qfc_output_i16(const int16_t* xq, int64_t n, int64_t d, const void* w, int32_t w_kind,
                                         int64_t rows, const int64_t* bias, const int32_t* multiplier,
                                         const int32_t* shift, int64_t mcount, int32_t act_min, int32_t act_max,
                                         int16_t* q_out, void* workspace, size_t workspace_bytes, void* stream) {
  clear_error();
  if (const int32_t bad = check_common(xq, n, d, w, w_kind, rows, multiplier, shift, mcount, q_out)) return bad;
  if (act_min > act_max || act_min < -32768 || act_max > 32767)
    return fail(MI355Q_BAD_ARG, "activation range [%d, %d] is no range within int16", act_min, act_max);
  if (d > kQfcMaxD)
    return fail(MI355Q_UNSUPPORTED, "d = %lld exceeds %d (the int32 planes of the accumulator)", static_cast<long long>(d), kQfcMaxD);
  // the weight sums are a term of every accumulator of the MFMA route: the workspace is always required
  if (const int32_t bad = check_workspace(workspace, workspace_bytes, (rows > 0 && d > 0) ? wsum_workspace(rows, 1) : 0))
    return bad;
  if (n == 0 || rows == 0) return MI355Q_OK;
  if (d == 0) return fail(MI355Q_BAD_ARG, "d must be >= 1");
  dim3 grid;
  if (const int32_t bad = tile_grid<int16_t>(n, rows, &grid)) return bad;

  OutArgs g{};
  g.xq = xq; g.w = static_cast<const uint8_t*>(w); g.bias = bias; g.mult = multiplier; g.shift = shift;
  g.wsum = static_cast<const int32_t*>(workspace); g.q = q_out;
  g.n = n; g.rows = rows; g.d = d; g.per_channel = (mcount == rows && rows != 1) ? 1 : 0;
  g.act_min = act_min; g.act_max = act_max; g.kind = w_kind;
  hipStream_t st = as_stream(stream);

  if (mfma_route(xq, w, d, 64)) {
    const int32_t st_sums = launch_weight_sums(g.w, w_kind, rows, static_cast<long long>(d), static_cast<int32_t*>(workspace), st);
    if (st_sums != MI355Q_OK) return st_sums;
    dispatch_kind(w_kind, [&](auto kind) {
      hipLaunchKernelGGL(qfc_out16_mfma_kernel<decltype(kind)::value>, grid, dim3(kThreads), 0, st, g);
    });
  } else {
    hipLaunchKernelGGL(qfc_out16_generic_kernel, dim3(generic_blocks(n * rows)), dim3(kThreads), 0, st, g);
  }
  MI355Q_CHECK_LAUNCH("int16 fully-connected output launch");
  return MI355Q_OK;
}
