// The MFMA route of the integer FULLY_CONNECTED kernels: qfc.hip (int8 activations, float output), qfc16.hip (int16
// activations, float output) and qfc_out.hip (both widths, stored output) include this header and add their own
// epilogues and `extern "C"` entries. (qfc_frag.h, included here, holds the stored weight: its elements, its sums and
// the B fragments.) The two int8 kernels (qfc_mfma_kernel, qfc_out_mfma_kernel) run qfc_main_loop and
// qfc_walk_outputs. The two int16 kernels take the tile constants, the activation policy with its split, the MFMA
// builtin, qfc_dot and the host side from here, but keep the loop written out in their own text: through the template
// the loop itself compiled to the same loads, waits and MFMAs, the code around it did not, and qfc_output_i16 measured
// 6.8 % slower at 4096 x 4096 (profiles/qfc_unify_ab.json tells both runs). As written they compile to the
// instructions they had. The template is kept generic over the width (it passed the int16 suites bit for bit).
//
// A wave owns 4 x 4 MFMA tiles of 16 x 16: four A fragments against four B fragments, 16 MFMAs per step of KSTEP
// elements of the reduction dimension, the next step's fragments in flight while they run. Both operands are contiguous
// along that dimension, so a lane's fragment is KSTEP / 4 consecutive elements of one row. What the activation width
// changes is in Act<Elem, KSTEP> and QfcTile<Elem>:
//   int8   4 token tiles x 1 plane:  a wave owns 64 tokens x 64 output channels, a workgroup (2 x 2 waves) 128 x 128;
//   int16  2 token tiles x 2 planes: gfx950 has no int16 matrix instruction, so x = 256 h + l_u is split in registers,
//          h = x >> 8 (arithmetic), l_s = int8(l_u ^ 0x80) = l_u - 128, acc = 256 Sum h w + Sum l_s w + 128 Sum w.
//          A wave owns 32 tokens x 64 output channels, a workgroup 64 x 128. acc[2 a] is the high plane of token
//          tile a, acc[2 a + 1] its low plane; each stays within 65536 * 128 * 128 = 2^30.
//
//   qfc_wave          which tile the wave owns, or that it owns none;
//   qfc_main_loop     acc = the wave's tile of Xq W^^T, with an optional call-out at the end of every scale block;
//   qfc_walk_outputs  the C / D map of the accumulators: per-channel constants once per column, f once per output;
//   qfc_dot           the generic route's product of one output over a segment, element by element;
//   host              the refusals, the routing, the grids and the workspace size that the entries share.
#pragma once

#include <type_traits>

#include "qfc_frag.h"

namespace mi355q {
namespace {

constexpr int kQfcMaxD = 65536;    // int8: d * 255 * 128 < 2^31; int16: each int32 plane d * 128 * 128 <= 2^30

// ---------------------------------------------------------------- the tile
constexpr int MF = 16;             // MFMA tile edge
constexpr int TB = 4;              // MFMA tiles per wave along output channels

template <class Elem> struct QfcTile {
  static constexpr int PLANES = sizeof(Elem);      // int8 planes of one activation
  static constexpr int TA = 4 / PLANES;            // MFMA tiles per wave along tokens (each in PLANES planes)
  static constexpr int TM = TA * PLANES;           // A fragments per step = rows of the accumulator tile
  static_assert(TM == TB, "a wave's tile is 4 x 4 MFMAs");
  static constexpr int WTA = TA * MF;              // a wave's tokens
  static constexpr int WTB = TB * MF;              // a wave's output channels
  static constexpr int BTA = 2 * WTA;              // a workgroup's tokens (2 x 2 waves)
  static constexpr int BTB = 2 * WTB;              // a workgroup's output channels
};

template <int KSTEP>
__device__ __forceinline__ I32x4 mfma_i8(typename FragOf<KSTEP>::T a, typename FragOf<KSTEP>::T b, I32x4 c) {
  if constexpr (KSTEP == 64) return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_i32_16x16x32_i8(a, b, c, 0, 0, 0);
}

// ---------------------------------------------------------------- activations
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

// A lane's KSTEP / 4 consecutive activations as loaded (Raw), and their PLANES int8 fragments.
template <class Elem, int KSTEP> struct Act;
template <> struct Act<int8_t, 64> {
  using Raw = I32x4;
  static __device__ __forceinline__ Raw load(const int8_t* p) { return *reinterpret_cast<const I32x4*>(p); }
  static __device__ __forceinline__ Raw zero() { return I32x4{0, 0, 0, 0}; }
  static __device__ __forceinline__ void frags(const Raw& r, I32x4* f) { f[0] = r; }
};
template <> struct Act<int8_t, 32> {
  using Raw = long;
  static __device__ __forceinline__ Raw load(const int8_t* p) { return *reinterpret_cast<const long*>(p); }
  static __device__ __forceinline__ Raw zero() { return 0; }
  static __device__ __forceinline__ void frags(const Raw& r, long* f) { f[0] = r; }
};
template <> struct Act<int16_t, 64> {
  struct Raw { I32x4 a, b; };    // k = 0 .. 7 and 8 .. 15 of the lane's 16
  static __device__ __forceinline__ Raw load(const int16_t* p) {
    const I32x4* q = reinterpret_cast<const I32x4*>(p);
    return Raw{q[0], q[1]};
  }
  static __device__ __forceinline__ Raw zero() { return Raw{I32x4{0, 0, 0, 0}, I32x4{0, 0, 0, 0}}; }
  static __device__ __forceinline__ void frags(const Raw& r, I32x4* f) {
    f[0] = I32x4{high_bytes(r.a[0], r.a[1]), high_bytes(r.a[2], r.a[3]), high_bytes(r.b[0], r.b[1]), high_bytes(r.b[2], r.b[3])};
    f[1] = I32x4{low_bytes_biased(r.a[0], r.a[1]), low_bytes_biased(r.a[2], r.a[3]), low_bytes_biased(r.b[0], r.b[1]),
                 low_bytes_biased(r.b[2], r.b[3])};
  }
};
template <> struct Act<int16_t, 32> {
  using Raw = I32x4;             // the lane's 8
  static __device__ __forceinline__ Raw load(const int16_t* p) { return *reinterpret_cast<const I32x4*>(p); }
  static __device__ __forceinline__ Raw zero() { return I32x4{0, 0, 0, 0}; }
  static __device__ __forceinline__ void frags(const Raw& r, long* f) {
    f[0] = two_words(high_bytes(r[0], r[1]), high_bytes(r[2], r[3]));
    f[1] = two_words(low_bytes_biased(r[0], r[1]), low_bytes_biased(r[2], r[3]));
  }
};

// ---------------------------------------------------------------- the wave's tile
// grid: x = output-channel tiles, y = token tiles; kQfcThreads = 2 x 2 waves.
struct QfcWave {
  long long t0, r0;    // the tile's first token and output channel
  int fr, fg;          // lane & 15 and lane >> 4: a fragment's row, and its group of KSTEP / 4 elements
};

// false: the wave's tile lies outside the problem (the whole wave returns; the kernels have no barrier)
template <class Elem>
__device__ __forceinline__ bool qfc_wave(QfcWave& wv, long long n, long long rows) {
  using T = QfcTile<Elem>;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  wv.t0 = static_cast<long long>(blockIdx.y) * T::BTA + (wave >> 1) * T::WTA;
  wv.r0 = static_cast<long long>(blockIdx.x) * T::BTB + (wave & 1) * T::WTB;
  wv.fr = lane & 15;
  wv.fg = lane >> 4;
  return wv.t0 < n && wv.r0 < rows;
}

// ---------------------------------------------------------------- the main loop
struct NoBlockEnd {};

// acc = the wave's tile of Xq W^^T. MFMA route: d % KSTEP == 0, xq and w 16-byte aligned (so every fragment load is
// aligned to its own size). With a BlockEnd, block_end(b) is called after the last step of every block b of
// steps_per_block steps, in ascending order; it reads the block's sums out of acc and clears them.
template <class Elem, int KIND, int KSTEP, class BlockEnd = NoBlockEnd>
__device__ __forceinline__ void qfc_main_loop(const QfcWave& wv, const Elem* xq, const uint8_t* w, long long n,
                                              long long rows, long long d, I32x4 (&acc)[QfcTile<Elem>::TM][TB],
                                              int steps_per_block = 0, BlockEnd block_end = BlockEnd{}) {
  using XA = Act<Elem, KSTEP>;
  using RW = RawW<KIND, KSTEP>;
  using Frag = typename FragOf<KSTEP>::T;
  constexpr int TA = QfcTile<Elem>::TA, PLANES = QfcTile<Elem>::PLANES, TM = QfcTile<Elem>::TM;
  constexpr int E = KSTEP / 4;     // consecutive elements per lane and step

  const Elem* xp[TA];
  long long we[TB];
  bool xok[TA], wok[TB];
#pragma unroll
  for (int a = 0; a < TA; ++a) {
    const long long t = wv.t0 + a * MF + wv.fr;
    xok[a] = t < n;
    xp[a] = xq + (xok[a] ? t : 0) * d + wv.fg * E;
  }
#pragma unroll
  for (int b = 0; b < TB; ++b) {
    const long long r = wv.r0 + b * MF + wv.fr;
    wok[b] = r < rows;
    we[b] = (wok[b] ? r : 0) * d + wv.fg * E;
  }
#pragma unroll
  for (int m = 0; m < TM; ++m)
#pragma unroll
    for (int b = 0; b < TB; ++b) acc[m][b] = I32x4{0, 0, 0, 0};

  const int steps = static_cast<int>(d / KSTEP);
  typename XA::Raw xc[TA], xn[TA];
  typename RW::T wc[TB], wn[TB];
#pragma unroll
  for (int a = 0; a < TA; ++a) xc[a] = xok[a] ? XA::load(xp[a]) : XA::zero();
#pragma unroll
  for (int b = 0; b < TB; ++b) wc[b] = wok[b] ? RW::load(w, we[b]) : RW::zero();
  [[maybe_unused]] int in_block = 0, bi = 0;
  for (int s = 0; s < steps; ++s) {
    if (s + 1 < steps) {     // the next step's fragments fly while this step's MFMAs run
      const long long k = static_cast<long long>(s + 1) * KSTEP;
#pragma unroll
      for (int a = 0; a < TA; ++a) xn[a] = xok[a] ? XA::load(xp[a] + k) : XA::zero();
#pragma unroll
      for (int b = 0; b < TB; ++b) wn[b] = wok[b] ? RW::load(w, we[b] + k) : RW::zero();
    }
    Frag wf[TB], xf[TM];
#pragma unroll
    for (int b = 0; b < TB; ++b) wf[b] = RW::unpack(wc[b]);      // once, for every plane
#pragma unroll
    for (int a = 0; a < TA; ++a) XA::frags(xc[a], &xf[a * PLANES]);
#pragma unroll
    for (int a = 0; a < TA; ++a)
#pragma unroll
      for (int b = 0; b < TB; ++b)
#pragma unroll
        for (int p = 0; p < PLANES; ++p) acc[a * PLANES + p][b] = mfma_i8<KSTEP>(xf[a * PLANES + p], wf[b], acc[a * PLANES + p][b]);
#pragma unroll
    for (int a = 0; a < TA; ++a) xc[a] = xn[a];
#pragma unroll
    for (int b = 0; b < TB; ++b) wc[b] = wn[b];
    if constexpr (!std::is_same<BlockEnd, NoBlockEnd>::value) {
      if (++in_block == steps_per_block) {
        block_end(bi);
        in_block = 0;
        ++bi;
      }
    }
  }
}

// The C / D map of the 16x16 MFMAs: column (output channel) = lane & 15, row (token) = 4 (lane >> 4) + register. For
// every output channel r < rows of the lane, c = chan(r) once; then f(c, a, b, i, t, r) for each of its tokens t < n,
// whose accumulators are acc[a * PLANES + p][b][i]. (The callers' lambdas capture the kernel's arguments by value:
// behind a reference the compiler takes every store for a possible change of them and derives them again per output.)
template <class Elem, class Chan, class F>
__device__ __forceinline__ void qfc_walk_outputs(const QfcWave& wv, long long n, long long rows, Chan chan, F f) {
#pragma unroll
  for (int b = 0; b < TB; ++b) {
    const long long r = wv.r0 + b * MF + wv.fr;
    if (r >= rows) continue;
    const auto c = chan(r);
#pragma unroll
    for (int a = 0; a < QfcTile<Elem>::TA; ++a)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long long t = wv.t0 + a * MF + wv.fg * 4 + i;
        if (t >= n) continue;
        f(c, a, b, i, t, r);
      }
  }
}

// ---------------------------------------------------------------- the generic route
// Sum over k in [k0, k0 + len) of (xr[k] - zp) * W^[r][k], one weight element at a time; wr = r * d.
template <class Acc, class Elem>
__device__ __forceinline__ Acc qfc_dot(const Elem* xr, const uint8_t* w, int kind, long long wr, long long k0,
                                       long long len, int zp) {
  Acc acc = 0;
  for (long long k = k0; k < k0 + len; ++k)
    acc += static_cast<Acc>((static_cast<int>(xr[k]) - zp) * weight_element(w, kind, wr + k));
  return acc;
}

// ---------------------------------------------------------------- host side
// The checks return MI355Q_OK or the status of the refusal they recorded.
inline int32_t check_weight_kind(int32_t w_kind) {
  if (w_kind != MI355Q_CMP_I8 && w_kind != MI355Q_CMP_I4 && w_kind != MI355Q_CMP_I2)
    return fail(MI355Q_BAD_ARG, "weight kind %d is not I8, I4 or I2", w_kind);
  return MI355Q_OK;
}

inline int32_t check_block(int32_t block, int64_t d) {
  if (block != 0 && block != 32 && block != 64 && block != 128 && block != 256)
    return fail(MI355Q_BAD_ARG, "block must be 0, 32, 64, 128 or 256 (got %d)", block);
  if (block > 0 && d % block)
    return fail(MI355Q_BAD_SHAPE, "Quantized dimension %lld is not divisible by block size %d.",
                static_cast<long long>(d), block);
  return MI355Q_OK;
}

// The scale counts of a forward entry; *blockwise = one weight scale per row and block.
inline int32_t check_scale_counts(int64_t n, int64_t rows, int64_t d, int32_t block, int64_t x_scale_count,
                                  int64_t w_scale_count, bool wants_acc, bool* blockwise) {
  if (x_scale_count != 1 && x_scale_count != n)
    return fail(MI355Q_BAD_ARG, "x_scale_count must be 1 or n = %lld (got %lld)", static_cast<long long>(n),
                static_cast<long long>(x_scale_count));
  *blockwise = block > 0 && w_scale_count == rows * (d / block);      // (block = 0 with per-tensor / per-channel scales)
  if (!*blockwise && w_scale_count != 1 && w_scale_count != rows)
    return fail(MI355Q_BAD_ARG, "w_scale_count must be 1, rows = %lld or rows * d / block (got %lld)",
                static_cast<long long>(rows), static_cast<long long>(w_scale_count));
  if (*blockwise && wants_acc) return fail(MI355Q_BAD_ARG, "acc_out is not available with blockwise scales");
  return MI355Q_OK;
}

// rows * nblocks int32 weight sums
inline size_t wsum_workspace(int64_t rows, int64_t nblocks) {
  return (static_cast<size_t>(rows) * static_cast<size_t>(nblocks) * sizeof(int32_t) + 255) & ~static_cast<size_t>(255);
}

inline int32_t check_workspace(const void* workspace, size_t workspace_bytes, size_t need) {
  if (need > 0 && (!workspace || workspace_bytes < need))
    return fail(MI355Q_BAD_ARG, "workspace of %zu bytes is smaller than the %zu needed", workspace ? workspace_bytes : size_t{0}, need);
  return MI355Q_OK;
}

inline bool mfma_route(const void* xq, const void* w, int64_t d, int kstep) {
  return d % kstep == 0 && reinterpret_cast<uintptr_t>(xq) % 16 == 0 && reinterpret_cast<uintptr_t>(w) % 16 == 0;
}

// The MFMA route's grid for activations of type Elem.
template <class Elem>
inline int32_t tile_grid(int64_t n, int64_t rows, dim3* grid) {
  using T = QfcTile<Elem>;
  const int64_t row_tiles = (rows + T::BTB - 1) / T::BTB, tok_tiles = (n + T::BTA - 1) / T::BTA;
  if (row_tiles > 0x7FFFFFFFLL || tok_tiles > 65535) return fail(MI355Q_UNSUPPORTED, "too many tiles for one launch");
  *grid = dim3(static_cast<unsigned>(row_tiles), static_cast<unsigned>(tok_tiles));
  return MI355Q_OK;
}

// The generic route's grid: one thread per output, grid-strided beyond 2^20 workgroups.
inline unsigned generic_blocks(long long total) {
  const long long blocks = (total + kQfcThreads - 1) / kQfcThreads;
  return static_cast<unsigned>(blocks < (1 << 20) ? blocks : (1 << 20));
}

// f(std::integral_constant<int, KIND>) for a checked w_kind
template <class F>
inline void dispatch_kind(int32_t w_kind, F f) {
  if (w_kind == MI355Q_CMP_I8) f(std::integral_constant<int, MI355Q_CMP_I8>{});
  else if (w_kind == MI355Q_CMP_I4) f(std::integral_constant<int, MI355Q_CMP_I4>{});
  else f(std::integral_constant<int, MI355Q_CMP_I2>{});
}

}  // namespace
}  // namespace mi355q
