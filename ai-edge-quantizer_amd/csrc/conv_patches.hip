// The patch gather in front of the integer CONV_2D execution (include/mi355q.h, "Patch gather for CONV_2D"): an NHWC
// activation becomes the [N OH OW, KH KW C] rows that qfc.hip, qfc16.hip and qfc_out.hip read, a padded tap holding the
// caller's pad element. A byte copy: no value is interpreted, so a NaN keeps its payload.
//
// One kernel template, one UNIT per lane. A unit is 16 bytes on the vector route (C * elem_bytes % 16 == 0 and both
// pointers 16-byte aligned: then a tap is a whole number of units, a unit never straddles two taps, and rows of `out`
// are 16-byte aligned) and one element otherwise. Lane i of the launch writes unit i of `out`, so consecutive lanes
// store consecutive units (a wave stores 1 KB in one piece on the vector route); the loads are contiguous within a
// tap and the input is re-read KH KW / (stride_h stride_w) times, from L2. The unit index is 32-bit where the launch
// fits (the divisions are the kernel's only arithmetic), 64-bit with a grid stride otherwise; every address is 64-bit.
//
// The gather in front of TRANSPOSE_CONV ("Patch gather for TRANSPOSE_CONV") is the same kernel: one sub-pixel phase of
// a transposed convolution is a stride-1 gather whose taps walk the image backwards (a = qy + base - ti), which is
// move_unit with stride 1, a dilation of -1 and pad_top = -base. The host entry works the phase's tap counts and bases
// out; the kernel divides by no stride. mi355q_conv_patches_nhwc itself still refuses a dilation below 1.
#include "common.h"

namespace mi355q {
namespace {

constexpr int kThreads = 256;
constexpr int64_t kMaxK = 65536;      // the forward entries' limit on the reduction dimension

struct PatchArgs {
  const void* x;
  void* out;
  int64_t H, W;
  uint64_t total;                     // units to write: row_count * row_units
  uint32_t row_units, tap_units;      // units per patch row (K elem_bytes / unit) and per tap (C elem_bytes / unit)
  uint32_t KW, OW, OHW;
  uint32_t first_row;
  int32_t stride_h, stride_w, dil_h, dil_w, pad_top, pad_left;
};

template <typename T, typename IdxT>
__device__ __forceinline__ void move_unit(const PatchArgs& g, T pad, IdxT i) {
  const IdxT row = i / static_cast<IdxT>(g.row_units);
  const uint32_t p = static_cast<uint32_t>(i - row * g.row_units);
  const uint32_t t = g.first_row + static_cast<uint32_t>(row);      // < N OH OW <= INT32_MAX
  const uint32_t n = t / g.OHW, pix = t - n * g.OHW;
  const uint32_t oh = pix / g.OW, ow = pix - oh * g.OW;
  const uint32_t tap = p / g.tap_units, in_tap = p - tap * g.tap_units;
  const uint32_t kh = tap / g.KW, kw = tap - kh * g.KW;
  const int64_t ih = static_cast<int64_t>(oh) * g.stride_h - g.pad_top + static_cast<int64_t>(kh) * g.dil_h;
  const int64_t iw = static_cast<int64_t>(ow) * g.stride_w - g.pad_left + static_cast<int64_t>(kw) * g.dil_w;
  T v = pad;
  if (ih >= 0 && ih < g.H && iw >= 0 && iw < g.W)
    v = static_cast<const T*>(g.x)[((static_cast<int64_t>(n) * g.H + ih) * g.W + iw) * g.tap_units + in_tap];
  static_cast<T*>(g.out)[i] = v;
}

// A launch holds fewer than 2^32 work-items (the dispatch packet's grid size is 32-bit). Below that one lane moves one
// unit and the index is 32-bit; from there on a grid of kWideBlocks workgroups strides over the units with a 64-bit index.
constexpr uint32_t kWideBlocks = 1u << 20;

template <typename T, typename IdxT>
__global__ __launch_bounds__(kThreads) void conv_patches_kernel(PatchArgs g, T pad) {
  IdxT i = static_cast<IdxT>(blockIdx.x) * kThreads + threadIdx.x;
  if constexpr (sizeof(IdxT) == 4) {
    if (i < static_cast<IdxT>(g.total)) move_unit<T, IdxT>(g, pad, i);
  } else {
    for (; i < g.total; i += static_cast<IdxT>(kWideBlocks) * kThreads) move_unit<T, IdxT>(g, pad, i);
  }
}

template <typename T>
void launch(const PatchArgs& g, T pad, hipStream_t st) {
  if (g.total <= 0xFFFFFFFFull - kThreads) {
    const uint32_t blocks = static_cast<uint32_t>((g.total + kThreads - 1) / kThreads);      // blocks * kThreads < 2^32
    hipLaunchKernelGGL((conv_patches_kernel<T, uint32_t>), dim3(blocks), dim3(kThreads), 0, st, g, pad);
  } else {
    hipLaunchKernelGGL((conv_patches_kernel<T, uint64_t>), dim3(kWideBlocks), dim3(kThreads), 0, st, g, pad);
  }
}

// What both entries do once their arguments are checked: pick the route by C and the two addresses, count the units and
// launch. `g` holds the geometry (H, W, KW, OW, OHW, first_row, strides, dilations, paddings); K = taps C.
void enqueue(PatchArgs g, const void* x, void* out, int32_t elem_bytes, int64_t C, int64_t K, int64_t row_count,
             const void* pad_element, hipStream_t st) {
  const bool vec = (C * elem_bytes) % 16 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  const int unit = vec ? 16 : elem_bytes;
  g.x = x; g.out = out;
  g.row_units = static_cast<uint32_t>(K * elem_bytes / unit);
  g.tap_units = static_cast<uint32_t>(C * elem_bytes / unit);
  g.total = static_cast<uint64_t>(row_count) * g.row_units;
  if (vec) {
    uint4 pad;
    unsigned char* b = reinterpret_cast<unsigned char*>(&pad);
    for (int i = 0; i < 16; ++i) b[i] = static_cast<const unsigned char*>(pad_element)[i % elem_bytes];
    launch<uint4>(g, pad, st);
  } else if (elem_bytes == 1) {
    launch<uint8_t>(g, *static_cast<const uint8_t*>(pad_element), st);
  } else if (elem_bytes == 2) {
    uint16_t pad;
    __builtin_memcpy(&pad, pad_element, 2);
    launch<uint16_t>(g, pad, st);
  } else {
    uint32_t pad;
    __builtin_memcpy(&pad, pad_element, 4);
    launch<uint32_t>(g, pad, st);
  }
}

}  // namespace
}  // namespace mi355q

using namespace mi355q;

extern "C" int32_t mi355q_conv_patches_nhwc(const void* x, int32_t elem_bytes, int64_t N, int64_t H, int64_t W, int64_t C,
                                            int32_t KH, int32_t KW, int32_t stride_h, int32_t stride_w, int32_t dil_h,
                                            int32_t dil_w, int32_t pad_top, int32_t pad_left, int64_t OH, int64_t OW,
                                            int64_t first_row, int64_t row_count, const void* pad_element, void* out,
                                            void* stream) {
  clear_error();
  if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4)
    return fail(MI355Q_BAD_ARG, "elem_bytes must be 1, 2 or 4 (got %d)", elem_bytes);
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || KH <= 0 || KW <= 0 || OH <= 0 || OW <= 0)
    return fail(MI355Q_BAD_ARG, "every dimension must be positive (N %lld, H %lld, W %lld, C %lld, KH %d, KW %d, OH %lld, OW %lld)",
                static_cast<long long>(N), static_cast<long long>(H), static_cast<long long>(W), static_cast<long long>(C),
                KH, KW, static_cast<long long>(OH), static_cast<long long>(OW));
  if (stride_h <= 0 || stride_w <= 0) return fail(MI355Q_BAD_ARG, "strides must be positive (got %d, %d)", stride_h, stride_w);
  if (dil_h <= 0 || dil_w <= 0) return fail(MI355Q_BAD_ARG, "dilations must be positive (got %d, %d)", dil_h, dil_w);
  if (first_row < 0 || row_count < 0) return fail(MI355Q_BAD_ARG, "negative row window");
  // (every factor is positive and below 2^63, and every product is checked before the next factor enters)
  const int64_t taps = static_cast<int64_t>(KH) * KW;
  if (taps > kMaxK || C > kMaxK || taps * C > kMaxK)
    return fail(MI355Q_UNSUPPORTED, "K = KH KW C exceeds %lld (the forward entries' limit)", static_cast<long long>(kMaxK));
  const int64_t K = taps * C;
  if (OH > INT32_MAX || OW > INT32_MAX || N > INT32_MAX || OH * OW > INT32_MAX || OH * OW * N > INT32_MAX)
    return fail(MI355Q_UNSUPPORTED, "N OH OW exceeds INT32_MAX patch rows");
  const int64_t rows_all = OH * OW * N;
  if (first_row > rows_all || row_count > rows_all - first_row)
    return fail(MI355Q_BAD_ARG, "rows [%lld, %lld + %lld) are outside the %lld patch rows", static_cast<long long>(first_row),
                static_cast<long long>(first_row), static_cast<long long>(row_count), static_cast<long long>(rows_all));
  const unsigned __int128 in_bytes = static_cast<unsigned __int128>(N) * static_cast<uint64_t>(H) * static_cast<uint64_t>(W);
  if (H > INT32_MAX || W > INT32_MAX || in_bytes * static_cast<uint64_t>(C * elem_bytes) > (static_cast<unsigned __int128>(1) << 62))
    return fail(MI355Q_UNSUPPORTED, "the activation exceeds 2^62 bytes");
  if (row_count == 0) return MI355Q_OK;
  if (!x || !out || !pad_element) return fail(MI355Q_BAD_ARG, "null pointer");

  PatchArgs g{};
  g.H = H; g.W = W;
  g.KW = static_cast<uint32_t>(KW); g.OW = static_cast<uint32_t>(OW); g.OHW = static_cast<uint32_t>(OH * OW);
  g.first_row = static_cast<uint32_t>(first_row);
  g.stride_h = stride_h; g.stride_w = stride_w; g.dil_h = dil_h; g.dil_w = dil_w; g.pad_top = pad_top; g.pad_left = pad_left;
  enqueue(g, x, out, elem_bytes, C, K, row_count, pad_element, as_stream(stream));
  MI355Q_CHECK_LAUNCH("conv patch gather launch");
  return MI355Q_OK;
}

namespace {

// One axis of a TRANSPOSE_CONV geometry: the forward convolution (kernel K, stride s, no dilation) from the OUTPUT
// size `out` back to the input size `in`, by TFLite's rule, with pad_before = `pad`. SAME: in = ceil(out / s);
// VALID: in = (out + s - K) / s; pad_before = max(0, (in - 1) s + K - out) / 2 under both.
bool forward_axis_ok(int64_t in, int64_t out, int64_t K, int64_t s, int64_t pad) {
  const bool same = in == (out + s - 1) / s;
  const bool valid = out + s - K >= s && in == (out + s - K) / s;
  const int64_t total = (in - 1) * s + K - out;      // (in, out <= INT32_MAX and K, s are int32: no overflow)
  return (same || valid) && pad == (total > 0 ? total : 0) / 2;
}

// The taps of one phase along one axis: ky = r, r + s, ... < K with r = (phase + pad) % s, in ascending order. Tap ti
// reads input a = q + base - ti with base = (phase + pad) / s, so the kernel divides by no stride.
struct PhaseAxis {
  int64_t taps, base, rows;      // rows: the q with q s + phase < out
};

PhaseAxis phase_axis(int64_t out, int64_t K, int64_t s, int64_t pad, int64_t phase) {
  const int64_t r = (phase + pad) % s;
  PhaseAxis a;
  a.taps = r < K ? (K - r + s - 1) / s : 0;
  a.base = (phase + pad) / s;
  a.rows = phase < out ? (out - phase + s - 1) / s : 0;
  return a;
}

}  // namespace

extern "C" int32_t mi355q_tconv_patches_nhwc(const void* x, int32_t elem_bytes, int64_t N, int64_t IH, int64_t IW, int64_t C,
                                             int32_t KH, int32_t KW, int32_t stride_h, int32_t stride_w, int32_t pad_top,
                                             int32_t pad_left, int64_t OH, int64_t OW, int32_t phase_h, int32_t phase_w,
                                             int64_t first_row, int64_t row_count, const void* pad_element, void* out,
                                             void* stream) {
  clear_error();
  if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4)
    return fail(MI355Q_BAD_ARG, "elem_bytes must be 1, 2 or 4 (got %d)", elem_bytes);
  if (N <= 0 || IH <= 0 || IW <= 0 || C <= 0 || KH <= 0 || KW <= 0 || OH <= 0 || OW <= 0)
    return fail(MI355Q_BAD_ARG, "every dimension must be positive (N %lld, IH %lld, IW %lld, C %lld, KH %d, KW %d, OH %lld, OW %lld)",
                static_cast<long long>(N), static_cast<long long>(IH), static_cast<long long>(IW), static_cast<long long>(C),
                KH, KW, static_cast<long long>(OH), static_cast<long long>(OW));
  if (stride_h <= 0 || stride_w <= 0) return fail(MI355Q_BAD_ARG, "strides must be positive (got %d, %d)", stride_h, stride_w);
  if (phase_h < 0 || phase_h >= stride_h || phase_w < 0 || phase_w >= stride_w)
    return fail(MI355Q_BAD_ARG, "phase (%d, %d) is outside the strides (%d, %d)", phase_h, phase_w, stride_h, stride_w);
  if (first_row < 0 || row_count < 0) return fail(MI355Q_BAD_ARG, "negative row window");
  if (OH > INT32_MAX || OW > INT32_MAX || N > INT32_MAX || IH > INT32_MAX || IW > INT32_MAX)
    return fail(MI355Q_UNSUPPORTED, "N, IH, IW, OH or OW exceeds INT32_MAX");
  if (pad_top < 0 || pad_left < 0 || !forward_axis_ok(IH, OH, KH, stride_h, pad_top) || !forward_axis_ok(IW, OW, KW, stride_w, pad_left))
    return fail(MI355Q_BAD_ARG, "the forward convolution (kernel %d x %d, strides %d, %d, paddings %d, %d) does not map the output"
                " %lld x %lld to the input %lld x %lld", KH, KW, stride_h, stride_w, pad_top, pad_left,
                static_cast<long long>(OH), static_cast<long long>(OW), static_cast<long long>(IH), static_cast<long long>(IW));
  const PhaseAxis ph = phase_axis(OH, KH, stride_h, pad_top, phase_h), pw = phase_axis(OW, KW, stride_w, pad_left, phase_w);
  if (ph.taps == 0 || pw.taps == 0)
    return fail(MI355Q_UNSUPPORTED, "phase (%d, %d) has no tap (a stride exceeds the kernel)", phase_h, phase_w);
  const int64_t taps = ph.taps * pw.taps;      // (each <= INT32_MAX)
  if (taps > kMaxK || C > kMaxK || taps * C > kMaxK)
    return fail(MI355Q_UNSUPPORTED, "K = taps C of the phase exceeds %lld (the forward entries' limit)", static_cast<long long>(kMaxK));
  const int64_t K = taps * C;
  if (ph.rows * pw.rows > INT32_MAX || ph.rows * pw.rows * N > INT32_MAX)
    return fail(MI355Q_UNSUPPORTED, "N QH QW exceeds INT32_MAX patch rows");
  const int64_t rows_all = ph.rows * pw.rows * N;
  if (first_row > rows_all || row_count > rows_all - first_row)
    return fail(MI355Q_BAD_ARG, "rows [%lld, %lld + %lld) are outside the %lld patch rows of the phase", static_cast<long long>(first_row),
                static_cast<long long>(first_row), static_cast<long long>(row_count), static_cast<long long>(rows_all));
  // (N IH IW <= 2 N QH QW + N: with C <= 65536 the activation stays far below the CONV_2D entry's 2^62 bytes)
  if (row_count == 0) return MI355Q_OK;
  if (!x || !out || !pad_element) return fail(MI355Q_BAD_ARG, "null pointer");

  // The phase as a stride-1 gather that walks the image backwards: a = qy + base_h - ti is move_unit's
  // oh stride_h - pad_top + kh dil_h with stride 1, pad_top = -base_h and dil_h = -1.
  PatchArgs g{};
  g.H = IH; g.W = IW;
  g.KW = static_cast<uint32_t>(pw.taps); g.OW = static_cast<uint32_t>(pw.rows); g.OHW = static_cast<uint32_t>(ph.rows * pw.rows);
  g.first_row = static_cast<uint32_t>(first_row);
  g.stride_h = 1; g.stride_w = 1; g.dil_h = -1; g.dil_w = -1;
  g.pad_top = -static_cast<int32_t>(ph.base); g.pad_left = -static_cast<int32_t>(pw.base);
  enqueue(g, x, out, elem_bytes, C, K, row_count, pad_element, as_stream(stream));
  MI355Q_CHECK_LAUNCH("transposed conv patch gather launch");
  return MI355Q_OK;
}
