// Store variants of the row-wise requant kernel that tools/kbench times and the library does not use.
#pragma once

#include "requant_kernels.h"

namespace mi355q {
namespace requant {

// A wave holds the words of its contiguous run of the row, word j * 64 + lane in lane's w[j]. They go through the
// wave-private slab (written at j * 64 + lane: conflict-free) and come back so that every lane stores 16-byte
// pieces: piece k of lane L is the bytes [(k * 64 + L) * 16, + 16) of the run, so every store instruction of the
// wave writes 1 KiB contiguous (for R * WB == 16 lane L simply holds the R consecutive words [L * R, L * R + R)).
// `dst` is the first byte of the run and must be 16-byte aligned; the lane whose piece straddles `nvalid` (the
// words of the run that lie inside the row) stores its valid words one by one, and nothing behind them.

template <int WB, int R, bool NT, bool NTW>
__device__ __forceinline__ void exchange_store_ragged(lds_u32* slab32, const uint32_t (&w)[R], uint8_t* dst, int nvalid,
                                               int lane) {
  static_assert(R * WB >= 16 && R * WB % 16 == 0, "whole 16-byte pieces");
  using W = typename WordOf<WB>::type;
  constexpr int PW = 16 / WB;        // words per piece
  constexpr int NP = R * WB / 16;    // pieces per lane
  typedef __attribute__((address_space(3))) W lds_w;
  typedef __attribute__((address_space(3))) u32x4_t lds_u32x4;
  lds_w* slab = (lds_w*)slab32;
#pragma unroll
  for (int j = 0; j < R; ++j) slab[j * kWave + lane] = static_cast<W>(w[j]);
  wave_lds_order();
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const int o = (k * kWave + lane) * PW;   // first word of the piece
    uint8_t* at = dst + static_cast<int64_t>(o) * WB;
    if (o + PW <= nvalid) {
      const u32x4_t p = *(lds_u32x4*)(slab + o);
      gstore4<NT>(at, p);
    } else {
#pragma unroll
      for (int i = 0; i < PW; ++i)
        if (o + i < nvalid) store_word<WB, NTW>(at + i * WB, slab[o + i]);
    }
  }
  wave_lds_order();   // the next exchange reuses the slab
}

// ------------------------------------------------------------------------
// The rows kernel (csrc/requant_kernels.h, (B)) with the store variants that were timed and not taken, and with
// the exchange of (B') for every width: cols4 <= TPR * R, ragged row ends included.
//
// WIDE chooses what a lane owns and how the integers leave (tools/kbench times the three):
//   0  float4 j * TPR + lane; one word (dword of int8 / 16 bits of int4 / byte of int2) per store;
//   1  "pairs": wave w owns the contiguous run [w * 64 R, (w + 1) * 64 R) of the row and a lane two adjacent
//      float4 per step (2 * lane, 2 * lane + 1, + 128 j'), stored together (emit<BITS, 2>): 8-byte q stores;
//   2  "exchange": every wave owns a contiguous run of the row and loads it at run + j * 64 + lane (every load
//      instruction 1 KiB contiguous, as in 0); the words of an output go through a wave-private LDS slab and leave
//      as 16-byte stores (exchange_store). The runs are `steps` = ceil(cols4 / 256) load steps long, not R, so
//      that a row shorter than the kernel's widest keeps all four waves loading. Outputs whose lane piece is
//      shorter than 16 bytes (R < 4; packed int4 below R = 8, int2 below R = 16) keep the store per word:
//      8-byte stores were slower than it at every width timed. On rows that leave lanes of a wave without a piece
//      (3072, 11008 columns) it lost to 0, so the library has it for rows that fill the kernel only.
// 1 and 2 take their wide stores only where the tensor's output pointer and the row pitch are aligned to them
// (decided per tensor, in the kernel: the batched forms promise no more than out_align() of requant.hip), and
// the store per word of 0 otherwise. NTS: non-temporal wide stores; loads and word stores follow NT.
// ------------------------------------------------------------------------
template <int BITS, int TPR, int R, bool FAST, bool BATCHED, bool NT = false, typename ARGS = RequantArgs,
          int WIDE = 0, bool NTS = NT>
__global__ __launch_bounds__(256) void rows_variants_kernel(ARGS a) {
  static_assert(TPR == 256 || (TPR <= kWave && (TPR & (TPR - 1)) == 0),
                "a row is owned by part of a wave, one wave, or the whole 256-thread block");
  static_assert(WIDE == 0 || TPR >= kWave, "the wide stores work on whole waves");
  static_assert(WIDE >= 0 && WIDE <= 2, "0: word stores, 1: pairs, 2: LDS exchange");
  static_assert(WIDE != 1 || R == 1 || R % 2 == 0, "pairs need an even number of float4 per lane");
  constexpr int RPB = 256 / TPR;  // rows per block
  constexpr int MODE = (WIDE == 1 && R < 2) || (WIDE == 2 && R < 4) ? 0 : WIDE;   // too little per lane to widen
  const int t = BATCHED ? blockIdx.y : 0;
  const float4* __restrict__ x = pick<BATCHED, const float4>(a.x, t);
  int8_t* q = pick<BATCHED, int8_t>(a.q, t);
  uint8_t* packed = pick<BATCHED, uint8_t>(a.packed, t);
  float* scale = pick<BATCHED, float>(a.scale, t);
  const float* clip = BATCHED ? nullptr : a.clip;

  const int lane = threadIdx.x % TPR;
  const int64_t row = static_cast<int64_t>(blockIdx.x) * RPB + threadIdx.x / TPR;
  const int cols4 = static_cast<int>(a.cols / 4);
  const bool live = row < a.rows;
  const int64_t row4 = row * cols4;
  // the lane in its wave, the load steps of a wave's run and where the run starts in the row (MODE != 0)
  const int wl = threadIdx.x & (kWave - 1);
  const int steps = (MODE == 2 && TPR > kWave) ? (cols4 + TPR - 1) / TPR : R;
  const int run = TPR > kWave ? (lane / kWave) * (kWave * steps) : 0;
  auto col4 = [&](int j) -> int {   // the float4 of the row that v[j] holds
    if constexpr (MODE == 0) return j * TPR + lane;
    else if constexpr (MODE == 1) return run + (j / 2) * (2 * kWave) + 2 * wl + (j & 1);
    else return run + j * kWave + wl;
  };
  auto holds = [&](int j) -> bool { return (MODE != 2 || j < steps) && col4(j) < cols4; };

  float4 v[R][1];
#pragma unroll
  for (int j = 0; j < R; ++j) {
    v[j][0] = (live && holds(j)) ? gload4<NT>(x + row4 + col4(j)) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  uint32_t m = 0;
#pragma unroll
  for (int j = 0; j < R; ++j) m = max(m, absmax4(v[j][0]));
  m = group_max_u32<(TPR < kWave ? TPR : kWave)>(m);
  if constexpr (TPR > kWave) {
    __shared__ uint32_t part[256 / kWave];
    if ((threadIdx.x & (kWave - 1)) == 0) part[threadIdx.x / kWave] = m;
    __syncthreads();
    m = max(max(part[0], part[1]), max(part[2], part[3]));
  }
  if (!live) return;
  uint16_t hb;
  const float s = make_scale<BITS, false>(m, clip, row, &hb);
  if (lane == 0) *(MI355Q_GLOBAL float*)(scale + row) = s;

  constexpr int SUBB = BITS / 2;   // bytes of packed output per float4 (4, 2, 1)
  const bool same = BITS == 8 && reinterpret_cast<int8_t*>(packed) == q;
  if (same) packed = nullptr;      // the same bytes: written once
  if constexpr (MODE == 1) {
    const bool q_ok = ((reinterpret_cast<uintptr_t>(q) | a.cols) & 7) == 0;
    const bool p_ok = ((reinterpret_cast<uintptr_t>(packed) | (a.cols / 4 * SUBB)) & (2 * SUBB - 1)) == 0;
    if (q_ok && p_ok) {
#pragma unroll
      for (int j = 0; j < R; j += 2) {
        const int c = col4(j);
        if (c + 1 < cols4) {
          const float4 pair[2] = {v[j][0], v[j + 1][0]};
          emit<BITS, 2, FAST, NTS>(pair, s, row4 + c, q, packed);
        } else if (c < cols4) {
          emit<BITS, 1, FAST, NTS>(v[j], s, row4 + c, q, packed);
        }
      }
      return;
    }
  }
  if constexpr (MODE == 2) {
    constexpr bool kSubWide = BITS == 8 || R * SUBB >= 16;   // packed sub-byte pieces of 16 bytes
    const bool wide_q = q != nullptr && wide_ok(q, a.cols);
    const bool wide_p = kSubWide && packed != nullptr && wide_ok(packed, a.cols / 4 * SUBB);
    if (wide_q || wide_p) {
      __shared__ __attribute__((aligned(16))) uint32_t slabs[256 / kWave][kWave * R];
      lds_u32* slab = (lds_u32*)slabs[threadIdx.x / kWave];
      const float r = FAST ? 1.0f / s : 0.f;
      uint32_t w8[R], subw[R];
#pragma unroll
      for (int j = 0; j < R; ++j) quant_words<BITS, FAST>(v[j][0], s, r, &w8[j], &subw[j]);
      const int nvalid = min(max(cols4 - run, 0), kWave * steps);
      // each output on its own: the exchange where it may, a store per word where not
      auto out = [&](auto wb, const uint32_t (&w)[R], uint8_t* base, bool wide) {
        constexpr int WB = decltype(wb)::value;
        if constexpr (R * WB >= 16) {
          if (wide) {
            exchange_store_ragged<WB, R, NTS, NT>(slab, w, base + (row4 + run) * WB, nvalid, wl);
            return;
          }
        }
#pragma unroll
        for (int j = 0; j < R; ++j)
          if (holds(j)) store_word<WB, NT>(base + (row4 + col4(j)) * WB, w[j]);
      };
      if (q != nullptr) out(std::integral_constant<int, 4>{}, w8, reinterpret_cast<uint8_t*>(q), wide_q);
      if (packed != nullptr) {
        if constexpr (BITS == 8) out(std::integral_constant<int, 4>{}, w8, packed, wide_p);
        else out(std::integral_constant<int, SUBB>{}, subw, packed, wide_p);
      }
      return;
    }
  }
#pragma unroll
  for (int j = 0; j < R; ++j)
    if (holds(j)) emit<BITS, 1, FAST, NT>(v[j], s, row4 + col4(j), q, packed);
}

}  // namespace requant
}  // namespace mi355q
