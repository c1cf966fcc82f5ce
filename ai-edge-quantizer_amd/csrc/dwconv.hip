// Direct depthwise convolution (include/mi355q.h, "Direct depthwise convolution"): the DEPTHWISE_CONV_2D op of a float
// or quantized model on an NHWC activation, channels along the lanes. A depthwise filter [KH, KW, O] has no reduction
// over channels: output channel oc reads input channel oc / M and KH KW taps, so there is no GEMM to share and the
// kernel lives on loads: 2 KH KW of them per unit against one store (DESIGN 3e has the measurements). Three element
// types (float32; int8 with an int32 accumulator; int16 with an int64 accumulator) and two ends (the rescaled float32
// product, or the fixed-point epilogue of qfc_epilogue.h on the accumulator in registers, storing q_out alone).
//
// One kernel template, one UNIT per lane. A unit is 4 consecutive output channels of one output pixel on the vector
// route (M == 1, C % 4 == 0, every pointer 16-byte aligned: then a unit's activations, its filter taps and its outputs
// are each one aligned piece of 4 elements) and one output element otherwise. Lane i of the launch owns unit i of the
// [row_count, O] output, so consecutive lanes take consecutive channel groups of a pixel and then the next pixel: per
// tap the activation loads, the filter loads and the final stores are each contiguous across the wave. The filter
// (KH KW O elements, the same for every pixel) is read through the caches, where it stays. The unit index is 32-bit
// where the launch fits, 64-bit with a grid stride otherwise; every address is 64-bit. A tap outside the image is
// skipped: it adds nothing and nothing is read for it.
#include "common.h"
#include "qfc_epilogue.h"

namespace mi355q {
namespace {

constexpr int kThreads = 256;
constexpr int64_t kMaxTaps = 65536;      // 65536 * 255 * 128 < 2^31: the int32 accumulator of the int8 entries
constexpr uint32_t kWideBlocks = 1u << 20;

enum { kForward = 0, kOutput = 1 };

struct DwArgs {
  const void* x;           // [N, H, W, C]
  const void* w;           // [KH, KW, O]
  const float* x_scale;    // 1 or N
  const float* w_scale;    // 1 or O
  float* y;                // [row_count, O]
  void* acc_out;           // int32 / int64 [row_count, O] or null
  int64_t H, W, C;
  uint64_t total;          // units to compute: row_count * row_units
  uint32_t O, row_units;   // units per output row: O / 4 on the vector route, O otherwise
  uint32_t M, KH, KW, OW, OHW, first_row;
  int32_t stride_h, stride_w, dil_h, dil_w, pad_top, pad_left;
  int32_t xs_per_image, ws_per_channel;
  int32_t zp_x;
  OutArgs ep;              // bias, mult, shift, per_channel, zp_y, act_min, act_max, q
};

template <class T, int ALIGN>
struct alignas(ALIGN) Pack4 {
  T v[4];
};

template <class TX>
struct Elem;
template <>
struct Elem<float> {
  using W = float;
  using Acc = float;
};
template <>
struct Elem<int8_t> {
  using W = int8_t;
  using Acc = int;
};
template <>
struct Elem<int16_t> {
  using W = int8_t;
  using Acc = long long;
};

template <class TX>
__device__ __forceinline__ void tap(typename Elem<TX>::Acc& acc, TX x, typename Elem<TX>::W w, int zp) {
  if constexpr (sizeof(TX) == 4) {
    acc = __fadd_rn(acc, __fmul_rn(x, w));      // every product rounded, never contracted
  } else if constexpr (sizeof(TX) == 1) {
    acc += (static_cast<int>(x) - zp) * static_cast<int>(w);
  } else {
    acc += static_cast<long long>(static_cast<int>(x) * static_cast<int>(w));      // (|x w| <= 2^22)
  }
}

template <class TX, int MODE, bool VEC, class IdxT>
__device__ __forceinline__ void unit(const DwArgs& g, IdxT i) {
  using TW = typename Elem<TX>::W;
  using Acc = typename Elem<TX>::Acc;
  constexpr int V = VEC ? 4 : 1;
  const IdxT row = i / static_cast<IdxT>(g.row_units);
  const uint32_t u = static_cast<uint32_t>(i - row * g.row_units);
  const uint32_t oc = u * V;
  const uint32_t ic = VEC ? oc : oc / g.M;
  const uint32_t t = g.first_row + static_cast<uint32_t>(row);      // < N OH OW <= INT32_MAX
  const uint32_t n = t / g.OHW, pix = t - n * g.OHW;
  const uint32_t oh = pix / g.OW, ow = pix - oh * g.OW;
  const int64_t ih0 = static_cast<int64_t>(oh) * g.stride_h - g.pad_top;
  const int64_t iw0 = static_cast<int64_t>(ow) * g.stride_w - g.pad_left;
  const TX* x = static_cast<const TX*>(g.x);
  const TW* w = static_cast<const TW*>(g.w);

  Acc acc[V];
#pragma unroll
  for (int j = 0; j < V; ++j) acc[j] = 0;
  for (uint32_t kh = 0; kh < g.KH; ++kh) {
    const int64_t ih = ih0 + static_cast<int64_t>(kh) * g.dil_h;
    if (ih < 0 || ih >= g.H) continue;
    const int64_t xrow = (static_cast<int64_t>(n) * g.H + ih) * g.W;
    for (uint32_t kw = 0; kw < g.KW; ++kw) {
      const int64_t iw = iw0 + static_cast<int64_t>(kw) * g.dil_w;
      if (iw < 0 || iw >= g.W) continue;
      const int64_t xo = (xrow + iw) * g.C + ic;
      const int64_t wo = (static_cast<int64_t>(kh) * g.KW + kw) * g.O + oc;
      if constexpr (VEC) {
        const auto xv = *reinterpret_cast<const Pack4<TX, 4 * sizeof(TX)>*>(x + xo);
        const auto wv = *reinterpret_cast<const Pack4<TW, 4 * sizeof(TW)>*>(w + wo);
#pragma unroll
        for (int j = 0; j < 4; ++j) tap<TX>(acc[j], xv.v[j], wv.v[j], g.zp_x);
      } else {
        tap<TX>(acc[0], x[xo], w[wo], g.zp_x);
      }
    }
  }

  const int64_t o = static_cast<int64_t>(row) * g.O + oc;
  if constexpr (MODE == kForward) {
    float y[V];
    if constexpr (sizeof(TX) == 4) {
#pragma unroll
      for (int j = 0; j < V; ++j) y[j] = acc[j];
    } else {
      const float xs = g.x_scale[g.xs_per_image ? n : 0];
      float ws[V];
      if constexpr (VEC) {
        if (g.ws_per_channel) {
          const auto wsv = *reinterpret_cast<const Pack4<float, 16>*>(g.w_scale + oc);
#pragma unroll
          for (int j = 0; j < 4; ++j) ws[j] = wsv.v[j];
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) ws[j] = g.w_scale[0];
        }
      } else {
        ws[0] = g.w_scale[g.ws_per_channel ? oc : 0];
      }
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float sc = xs * ws[j];      // rounded to float32 (-ffp-contract=off)
        if constexpr (sizeof(TX) == 1) {
          y[j] = static_cast<float>(acc[j]) * sc;
        } else {
          y[j] = static_cast<float>(static_cast<double>(acc[j]) * static_cast<double>(sc));
        }
      }
    }
    if constexpr (VEC) {
      Pack4<float, 16> yv;
#pragma unroll
      for (int j = 0; j < 4; ++j) yv.v[j] = y[j];
      *reinterpret_cast<Pack4<float, 16>*>(g.y + o) = yv;
      if constexpr (sizeof(TX) != 4) {
        if (g.acc_out) {
          Pack4<Acc, 16> av;
#pragma unroll
          for (int j = 0; j < 4; ++j) av.v[j] = acc[j];
          *reinterpret_cast<Pack4<Acc, 16>*>(static_cast<Acc*>(g.acc_out) + o) = av;
        }
      }
    } else {
      g.y[o] = y[0];
      if constexpr (sizeof(TX) != 4) {
        if (g.acc_out) static_cast<Acc*>(g.acc_out)[o] = acc[0];
      }
    }
  } else {
    using TQ = TX;      // int8 in, int8 out; int16 in, int16 out
    TQ q[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      if constexpr (sizeof(TX) == 1) {
        q[j] = output8(acc[j], chan8(g.ep, static_cast<long long>(oc) + j), g.ep);
      } else {
        q[j] = output16(acc[j], chan16(g.ep, static_cast<long long>(oc) + j), g.ep);
      }
    }
    if constexpr (VEC) {
      Pack4<TQ, 4 * sizeof(TQ)> qv;
#pragma unroll
      for (int j = 0; j < 4; ++j) qv.v[j] = q[j];
      *reinterpret_cast<Pack4<TQ, 4 * sizeof(TQ)>*>(static_cast<TQ*>(g.ep.q) + o) = qv;
    } else {
      static_cast<TQ*>(g.ep.q)[o] = q[0];
    }
  }
}

// A launch holds fewer than 2^32 work-items. Below that one lane computes one unit and the index is 32-bit; from there
// on a grid of kWideBlocks workgroups strides over the units with a 64-bit index (conv_patches.hip's rule).
template <class TX, int MODE, bool VEC, class IdxT>
__global__ __launch_bounds__(kThreads) void dwconv_kernel(DwArgs g) {
  IdxT i = static_cast<IdxT>(blockIdx.x) * kThreads + threadIdx.x;
  if constexpr (sizeof(IdxT) == 4) {
    if (i < static_cast<IdxT>(g.total)) unit<TX, MODE, VEC, IdxT>(g, i);
  } else {
    for (; i < g.total; i += static_cast<IdxT>(kWideBlocks) * kThreads) unit<TX, MODE, VEC, IdxT>(g, i);
  }
}

template <class TX, int MODE, bool VEC>
void launch_route(const DwArgs& g, hipStream_t st) {
  if (g.total <= 0xFFFFFFFFull - kThreads) {
    const uint32_t blocks = static_cast<uint32_t>((g.total + kThreads - 1) / kThreads);      // blocks * kThreads < 2^32
    hipLaunchKernelGGL((dwconv_kernel<TX, MODE, VEC, uint32_t>), dim3(blocks), dim3(kThreads), 0, st, g);
  } else {
    hipLaunchKernelGGL((dwconv_kernel<TX, MODE, VEC, uint64_t>), dim3(kWideBlocks), dim3(kThreads), 0, st, g);
  }
}

template <class TX, int MODE>
void launch(DwArgs& g, int64_t row_count, bool vec, hipStream_t st) {
  g.row_units = vec ? g.O / 4 : g.O;
  g.total = static_cast<uint64_t>(row_count) * g.row_units;
  if (vec) launch_route<TX, MODE, true>(g, st);
  else launch_route<TX, MODE, false>(g, st);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

struct Geometry {
  int64_t N, H, W, C;
  int32_t KH, KW, M, stride_h, stride_w, dil_h, dil_w, pad_top, pad_left;
  int64_t OH, OW, first_row, row_count;
};

// What every entry refuses first, in one order; *O = C M.
int32_t check_geometry(const Geometry& s, int elem_bytes, int64_t* O) {
  if (s.N <= 0 || s.H <= 0 || s.W <= 0 || s.C <= 0 || s.KH <= 0 || s.KW <= 0 || s.OH <= 0 || s.OW <= 0)
    return fail(MI355Q_BAD_ARG, "every dimension must be positive (N %lld, H %lld, W %lld, C %lld, KH %d, KW %d, OH %lld, OW %lld)",
                static_cast<long long>(s.N), static_cast<long long>(s.H), static_cast<long long>(s.W),
                static_cast<long long>(s.C), s.KH, s.KW, static_cast<long long>(s.OH), static_cast<long long>(s.OW));
  if (s.M <= 0) return fail(MI355Q_BAD_ARG, "the depth multiplier must be positive (got %d)", s.M);
  if (s.stride_h <= 0 || s.stride_w <= 0)
    return fail(MI355Q_BAD_ARG, "strides must be positive (got %d, %d)", s.stride_h, s.stride_w);
  if (s.dil_h <= 0 || s.dil_w <= 0) return fail(MI355Q_BAD_ARG, "dilations must be positive (got %d, %d)", s.dil_h, s.dil_w);
  if (s.first_row < 0 || s.row_count < 0) return fail(MI355Q_BAD_ARG, "negative row window");
  if (static_cast<int64_t>(s.KH) * s.KW > kMaxTaps)
    return fail(MI355Q_UNSUPPORTED, "KH KW exceeds %lld taps (the int32 accumulator)", static_cast<long long>(kMaxTaps));
  if (s.OH > INT32_MAX || s.OW > INT32_MAX || s.N > INT32_MAX || s.OH * s.OW > INT32_MAX || s.OH * s.OW * s.N > INT32_MAX)
    return fail(MI355Q_UNSUPPORTED, "N OH OW exceeds INT32_MAX output rows");
  const int64_t rows_all = s.OH * s.OW * s.N;
  if (s.first_row > rows_all || s.row_count > rows_all - s.first_row)
    return fail(MI355Q_BAD_ARG, "rows [%lld, %lld + %lld) are outside the %lld output rows", static_cast<long long>(s.first_row),
                static_cast<long long>(s.first_row), static_cast<long long>(s.row_count), static_cast<long long>(rows_all));
  const unsigned __int128 pixels = static_cast<unsigned __int128>(s.N) * static_cast<uint64_t>(s.H) * static_cast<uint64_t>(s.W);
  if (s.H > INT32_MAX || s.W > INT32_MAX || s.C > (static_cast<int64_t>(1) << 60) ||
      pixels * static_cast<uint64_t>(s.C * elem_bytes) > (static_cast<unsigned __int128>(1) << 62))
    return fail(MI355Q_UNSUPPORTED, "the activation exceeds 2^62 bytes");
  if (s.C > INT32_MAX || s.C * s.M > INT32_MAX) return fail(MI355Q_UNSUPPORTED, "O = C M exceeds INT32_MAX output channels");
  *O = s.C * s.M;
  return MI355Q_OK;
}

int32_t check_forward_scales(const Geometry& s, int64_t O, int32_t w_kind, int64_t x_scale_count, int64_t w_scale_count) {
  if (w_kind != MI355Q_CMP_I8) return fail(MI355Q_BAD_ARG, "weight kind %d is not I8 (a depthwise filter is int8)", w_kind);
  if (x_scale_count != 1 && x_scale_count != s.N)
    return fail(MI355Q_BAD_ARG, "x_scale_count must be 1 or N = %lld (got %lld)", static_cast<long long>(s.N),
                static_cast<long long>(x_scale_count));
  if (w_scale_count != 1 && w_scale_count != O)
    return fail(MI355Q_BAD_ARG, "w_scale_count must be 1 or O = %lld (got %lld)", static_cast<long long>(O),
                static_cast<long long>(w_scale_count));
  return MI355Q_OK;
}

int32_t check_output_tables(int64_t O, int32_t w_kind, int64_t mcount, int32_t act_min, int32_t act_max, int bits) {
  if (w_kind != MI355Q_CMP_I8) return fail(MI355Q_BAD_ARG, "weight kind %d is not I8 (a depthwise filter is int8)", w_kind);
  if (mcount != 1 && mcount != O)
    return fail(MI355Q_BAD_ARG, "mcount must be 1 or O = %lld (got %lld)", static_cast<long long>(O), static_cast<long long>(mcount));
  const int32_t lo = bits == 8 ? -128 : -32768, hi = bits == 8 ? 127 : 32767;
  if (act_min > act_max || act_min < lo || act_max > hi)
    return fail(MI355Q_BAD_ARG, "activation range [%d, %d] is no range within int%d", act_min, act_max, bits);
  return MI355Q_OK;
}

DwArgs make_args(const Geometry& s, int64_t O, const void* x, const void* w) {
  DwArgs g{};
  g.x = x; g.w = w; g.H = s.H; g.W = s.W; g.C = s.C;
  g.O = static_cast<uint32_t>(O); g.M = static_cast<uint32_t>(s.M);
  g.KH = static_cast<uint32_t>(s.KH); g.KW = static_cast<uint32_t>(s.KW);
  g.OW = static_cast<uint32_t>(s.OW); g.OHW = static_cast<uint32_t>(s.OH * s.OW);
  g.first_row = static_cast<uint32_t>(s.first_row);
  g.stride_h = s.stride_h; g.stride_w = s.stride_w; g.dil_h = s.dil_h; g.dil_w = s.dil_w;
  g.pad_top = s.pad_top; g.pad_left = s.pad_left;
  return g;
}

// M == 1 and C % 4 == 0; the pointers are the caller's to check.
inline bool vector_shape(const Geometry& s) { return s.M == 1 && s.C % 4 == 0; }

}  // namespace
}  // namespace mi355q

using namespace mi355q;

#define MI355Q_DW_GEOMETRY \
  Geometry { N, H, W, C, KH, KW, M, stride_h, stride_w, dil_h, dil_w, pad_top, pad_left, OH, OW, first_row, row_count }

extern "C" int32_t mi355q_dwconv_forward_f32(const float* x, int64_t N, int64_t H, int64_t W, int64_t C, const float* w,
                                             int32_t KH, int32_t KW, int32_t M, int32_t stride_h, int32_t stride_w,
                                             int32_t dil_h, int32_t dil_w, int32_t pad_top, int32_t pad_left, int64_t OH,
                                             int64_t OW, int64_t first_row, int64_t row_count, float* y_out, void* stream) {
  clear_error();
  const Geometry s = MI355Q_DW_GEOMETRY;
  int64_t O = 0;
  if (const int32_t bad = check_geometry(s, 4, &O)) return bad;
  if (row_count == 0) return MI355Q_OK;
  if (!x || !w || !y_out) return fail(MI355Q_BAD_ARG, "null pointer");
  DwArgs g = make_args(s, O, x, w);
  g.y = y_out;
  launch<float, kForward>(g, row_count, vector_shape(s) && aligned16(x) && aligned16(w) && aligned16(y_out), as_stream(stream));
  MI355Q_CHECK_LAUNCH("depthwise convolution launch");
  return MI355Q_OK;
}

extern "C" int32_t mi355q_dwconv_forward_i8(const int8_t* xq, int64_t N, int64_t H, int64_t W, int64_t C,
                                            const float* x_scale, int64_t x_scale_count, int32_t x_zero_point,
                                            const void* w, int32_t w_kind, int32_t KH, int32_t KW, int32_t M,
                                            const float* w_scale, int64_t w_scale_count, int32_t stride_h, int32_t stride_w,
                                            int32_t dil_h, int32_t dil_w, int32_t pad_top, int32_t pad_left, int64_t OH,
                                            int64_t OW, int64_t first_row, int64_t row_count, float* y_out,
                                            int32_t* acc_out, void* stream) {
  clear_error();
  const Geometry s = MI355Q_DW_GEOMETRY;
  int64_t O = 0;
  if (const int32_t bad = check_geometry(s, 1, &O)) return bad;
  if (const int32_t bad = check_forward_scales(s, O, w_kind, x_scale_count, w_scale_count)) return bad;
  if (x_zero_point < -128 || x_zero_point > 127)
    return fail(MI355Q_BAD_ARG, "activation zero point %d is outside int8", x_zero_point);
  if (row_count == 0) return MI355Q_OK;
  if (!xq || !x_scale || !w || !w_scale || !y_out) return fail(MI355Q_BAD_ARG, "null pointer");
  DwArgs g = make_args(s, O, xq, w);
  g.x_scale = x_scale; g.w_scale = w_scale; g.y = y_out; g.acc_out = acc_out; g.zp_x = x_zero_point;
  g.xs_per_image = (x_scale_count == N && N != 1) ? 1 : 0;
  g.ws_per_channel = (w_scale_count == O && O != 1) ? 1 : 0;
  const bool vec = vector_shape(s) && aligned16(xq) && aligned16(w) && aligned16(y_out) && aligned16(acc_out) &&
                   (!g.ws_per_channel || aligned16(w_scale));
  launch<int8_t, kForward>(g, row_count, vec, as_stream(stream));
  MI355Q_CHECK_LAUNCH("integer depthwise convolution launch");
  return MI355Q_OK;
}

extern "C" int32_t mi355q_dwconv_forward_i16(const int16_t* xq, int64_t N, int64_t H, int64_t W, int64_t C,
                                             const float* x_scale, int64_t x_scale_count, const void* w, int32_t w_kind,
                                             int32_t KH, int32_t KW, int32_t M, const float* w_scale, int64_t w_scale_count,
                                             int32_t stride_h, int32_t stride_w, int32_t dil_h, int32_t dil_w,
                                             int32_t pad_top, int32_t pad_left, int64_t OH, int64_t OW, int64_t first_row,
                                             int64_t row_count, float* y_out, int64_t* acc_out, void* stream) {
  clear_error();
  const Geometry s = MI355Q_DW_GEOMETRY;
  int64_t O = 0;
  if (const int32_t bad = check_geometry(s, 2, &O)) return bad;
  if (const int32_t bad = check_forward_scales(s, O, w_kind, x_scale_count, w_scale_count)) return bad;
  if (row_count == 0) return MI355Q_OK;
  if (!xq || !x_scale || !w || !w_scale || !y_out) return fail(MI355Q_BAD_ARG, "null pointer");
  DwArgs g = make_args(s, O, xq, w);
  g.x_scale = x_scale; g.w_scale = w_scale; g.y = y_out; g.acc_out = acc_out;
  g.xs_per_image = (x_scale_count == N && N != 1) ? 1 : 0;
  g.ws_per_channel = (w_scale_count == O && O != 1) ? 1 : 0;
  const bool vec = vector_shape(s) && aligned16(xq) && aligned16(w) && aligned16(y_out) && aligned16(acc_out) &&
                   (!g.ws_per_channel || aligned16(w_scale));
  launch<int16_t, kForward>(g, row_count, vec, as_stream(stream));
  MI355Q_CHECK_LAUNCH("int16 depthwise convolution launch");
  return MI355Q_OK;
}

extern "C" int32_t mi355q_dwconv_output_i8(const int8_t* xq, int64_t N, int64_t H, int64_t W, int64_t C,
                                           int32_t x_zero_point, const void* w, int32_t w_kind, int32_t KH, int32_t KW,
                                           int32_t M, const int32_t* bias, const int32_t* multiplier, const int32_t* shift,
                                           int64_t mcount, int32_t out_zero_point, int32_t act_min, int32_t act_max,
                                           int32_t stride_h, int32_t stride_w, int32_t dil_h, int32_t dil_w,
                                           int32_t pad_top, int32_t pad_left, int64_t OH, int64_t OW, int64_t first_row,
                                           int64_t row_count, int8_t* q_out, void* stream) {
  clear_error();
  const Geometry s = MI355Q_DW_GEOMETRY;
  int64_t O = 0;
  if (const int32_t bad = check_geometry(s, 1, &O)) return bad;
  if (const int32_t bad = check_output_tables(O, w_kind, mcount, act_min, act_max, 8)) return bad;
  if (x_zero_point < -128 || x_zero_point > 127)
    return fail(MI355Q_BAD_ARG, "activation zero point %d is outside int8", x_zero_point);
  if (out_zero_point < -128 || out_zero_point > 127)
    return fail(MI355Q_BAD_ARG, "output zero point %d is outside int8", out_zero_point);
  if (row_count == 0) return MI355Q_OK;
  if (!xq || !w || !multiplier || !shift || !q_out) return fail(MI355Q_BAD_ARG, "null pointer");
  DwArgs g = make_args(s, O, xq, w);
  g.zp_x = x_zero_point;
  g.ep.bias = bias; g.ep.mult = multiplier; g.ep.shift = shift; g.ep.q = q_out;
  g.ep.per_channel = (mcount == O && O != 1) ? 1 : 0;
  g.ep.zp_y = out_zero_point; g.ep.act_min = act_min; g.ep.act_max = act_max;
  const bool vec = vector_shape(s) && aligned16(xq) && aligned16(w) && aligned16(q_out) && aligned16(bias) &&
                   (!g.ep.per_channel || (aligned16(multiplier) && aligned16(shift)));
  launch<int8_t, kOutput>(g, row_count, vec, as_stream(stream));
  MI355Q_CHECK_LAUNCH("integer depthwise convolution output launch");
  return MI355Q_OK;
}

extern "C" int32_t mi355q_dwconv_output_i16(const int16_t* xq, int64_t N, int64_t H, int64_t W, int64_t C, const void* w,
                                            int32_t w_kind, int32_t KH, int32_t KW, int32_t M, const int64_t* bias,
                                            const int32_t* multiplier, const int32_t* shift, int64_t mcount,
                                            int32_t act_min, int32_t act_max, int32_t stride_h, int32_t stride_w,
                                            int32_t dil_h, int32_t dil_w, int32_t pad_top, int32_t pad_left, int64_t OH,
                                            int64_t OW, int64_t first_row, int64_t row_count, int16_t* q_out,
                                            void* stream) {
  clear_error();
  const Geometry s = MI355Q_DW_GEOMETRY;
  int64_t O = 0;
  if (const int32_t bad = check_geometry(s, 2, &O)) return bad;
  if (const int32_t bad = check_output_tables(O, w_kind, mcount, act_min, act_max, 16)) return bad;
  if (row_count == 0) return MI355Q_OK;
  if (!xq || !w || !multiplier || !shift || !q_out) return fail(MI355Q_BAD_ARG, "null pointer");
  DwArgs g = make_args(s, O, xq, w);
  g.ep.bias = bias; g.ep.mult = multiplier; g.ep.shift = shift; g.ep.q = q_out;
  g.ep.per_channel = (mcount == O && O != 1) ? 1 : 0;
  g.ep.act_min = act_min; g.ep.act_max = act_max;
  const bool vec = vector_shape(s) && aligned16(xq) && aligned16(w) && aligned16(q_out) && aligned16(bias) &&
                   (!g.ep.per_channel || (aligned16(multiplier) && aligned16(shift)));
  launch<int16_t, kOutput>(g, row_count, vec, as_stream(stream));
  MI355Q_CHECK_LAUNCH("int16 depthwise convolution output launch");
  return MI355Q_OK;
}
