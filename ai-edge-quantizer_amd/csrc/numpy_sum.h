// Order-exact float32 sums in NumPy's order: what the OCTAV clipping search (K5) and the MSE scale (a14) share.
//
//   ref: algorithms/uniform_quantize/octav.py:30-112  (_guess_clipping_with_octav)
//   ref: algorithms/uniform_quantize/mse.py:100-109   (k * sqrt(mean(x^2)))
//
// Both reductions are float32 sums whose value depends on the order NumPy adds
// in. That order is deterministic (verified against NumPy 2.2 in
// tests/test_numpy_sum_model.py) and is reproduced here so the clipping
// constants / scales are BIT-IDENTICAL to the reference, not merely close:
//   * a reduction unit (row, block, or the whole tensor) is consumed in chunks
//     of 8192 elements (the nditer buffer);
//   * inside a chunk every maximal run of consecutive selected elements is summed
//     with NumPy's pairwise routine (n < 8: left to right; n <= 128: eight strided
//     accumulators combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) then the tail;
//     larger: split at n/2 rounded down to a multiple of 8) and the run sum is
//     added to the running total:  acc = acc + pairwise(run).
//
// One wave owns one unit. The unit is staged once into LDS (one HBM read for all
// 10 Newton iterations); selections are wave ballots, runs are found with scalar
// bit scans, and short runs are summed from registers with v_readlane.
#pragma once

#include "common.h"

namespace mi355q {

constexpr int kChunk = 8192;  // NumPy nditer buffer size (elements)

__device__ __forceinline__ float lane_bcast(float v, int src_lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src_lane));
}

// lane L receives lane L-1's value, lane 0 receives 0 (v_mov_b32_dpp wave_shr:1)
__device__ __forceinline__ float wave_shr1(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138, 0xF, 0xF, false));
}

template <bool SQUARE>
__device__ __forceinline__ float tr(float v) {
  if constexpr (SQUARE) return v * v;
  return v;
}

// NumPy pairwise leaf, 8 <= m <= 128: lanes 0..7 are the eight accumulators.
template <bool SQUARE>
__device__ __forceinline__ float leaf_sum(const float* a, int m, int lane) {
  const int full = m & ~7;
  float r = 0.f;
  if (lane < 8) {
    r = tr<SQUARE>(a[lane]);
    for (int i = 8; i < full; i += 8) r = r + tr<SQUARE>(a[i + lane]);
  }
  const float r0 = lane_bcast(r, 0), r1 = lane_bcast(r, 1), r2 = lane_bcast(r, 2),
              r3 = lane_bcast(r, 3), r4 = lane_bcast(r, 4), r5 = lane_bcast(r, 5),
              r6 = lane_bcast(r, 6), r7 = lane_bcast(r, 7);
  float res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
  for (int i = full; i < m; ++i) res = res + tr<SQUARE>(a[i]);
  return res;
}

// pairwise(a[0:n]) for n <= 8192; recursion depth is bounded by DEPTH.
template <bool SQUARE, int DEPTH>
__device__ __noinline__ float pairwise_sum(const float* a, int n, int lane) {
  if (n < 8) {
    float res = 0.f;
    for (int i = 0; i < n; ++i) res = res + tr<SQUARE>(a[i]);
    return res;
  }
  if (n <= 128) return leaf_sum<SQUARE>(a, n, lane);
  if constexpr (DEPTH > 0) {
    int n2 = n / 2;
    n2 -= n2 % 8;
    const float left = pairwise_sum<SQUARE, DEPTH - 1>(a, n2, lane);
    const float right = pairwise_sum<SQUARE, DEPTH - 1>(a + n2, n - n2, lane);
    return left + right;
  } else {
    return leaf_sum<SQUARE>(a, n, lane);  // unreachable for n <= 8192
  }
}

// Running masked sum in NumPy order. All members are wave-uniform.
struct RunSum {
  float acc = 0.f;
  unsigned count = 0;
  int pend_start = 0;    // a run that touches the end of the last batch and may continue
  int pend_len = 0;
  float pend_sum = 0.f;  // its left-to-right sum so far; meaningful while pend_len < 8

  // A run shorter than 8 is summed left to right from 0, so the part seen so far is a valid
  // prefix of that chain as long as the run stays shorter than 8; a run that reaches 8 switches
  // to the eight-accumulator scheme and is summed from memory once its end is known.
  __device__ __forceinline__ void flush(const float* a, int lane) {
    if (pend_len > 0) {
      acc = acc + (pend_len < 8 ? pend_sum : pairwise_sum<false, 8>(a + pend_start, pend_len, lane));
      pend_len = 0;
    }
  }

  // m: ballot of the selected lanes of the batch starting at element `base`;
  // v: this lane's element (lane l <-> element base + l); a: the unit.
  //
  // Fast path (no run of 8+ lanes in the batch; a run pending from the previous batch either
  // ended there or continues here and still stays shorter than 8): all runs are summed at once,
  // lane-parallel, by rounds of "left neighbour's partial sum + mine" (v_mov_b32_dpp
  // wave_shr:1; lane 0 continues the pending chain), then the run totals are added to the
  // running total in lane order. A run that touches the batch end stays pending with its partial
  // sum. Everything else takes the general per-run path.
  __device__ __forceinline__ void feed(unsigned long long m, int base, float v, const float* a,
                                       int lane) {
    if ((base % kChunk) == 0 || (m & 1ull) == 0) flush(a, lane);
    count += static_cast<unsigned>(__builtin_popcountll(m));
    if (m == 0) return;
    const unsigned long long m4 = m & (m >> 1) & (m >> 2) & (m >> 3);
    if ((m4 & (m4 >> 4)) != 0 || (pend_len > 0 && pend_len + __builtin_ctzll(~m) >= 8)) {
      feed_runs(m, base, v, a, lane);
      return;
    }
    const float carry = pend_len > 0 ? pend_sum : 0.f;  // lane 0 continues the pending chain
    pend_len = 0;
    const bool sel = ((m >> lane) & 1ull) != 0;
    float partial = sel ? (lane == 0 ? carry : 0.f) + v : 0.f;
    const unsigned long long m2 = m & (m >> 1);
    if (m2 != 0) {  // some run is longer than one element
      // every lane repeats "left neighbour's partial + mine" (run starts keep their first sum): a
      // lane at position p of its run is final after p rounds and a further round recomputes
      // the same value, so the round count only has to reach the longest run
      const bool cont = (((m2 << 1) >> lane) & 1ull) != 0;  // my left neighbour is in my run
      const int rounds = (m2 & (m >> 2)) == 0 ? 1 : (m4 == 0 ? 2 : 6);
      for (int t = 0; t < rounds; ++t) {
        const float left = wave_shr1(partial);
        if (cont) partial = left + v;
      }
    }
    unsigned long long mf = m;
    if (m >> 63) {  // trailing run (1..7 lanes): it may continue in the next batch
      const int t = __builtin_clzll(~m);
      mf = m & (~0ull >> t);
      pend_start = base + 64 - t;
      pend_len = t;
      pend_sum = lane_bcast(partial, 63);
    }
    unsigned long long ends = mf & ~(mf >> 1);  // last lane of every finished run
    const int k = __builtin_popcountll(ends);
    if (k <= 3) {
      while (ends != 0) {
        acc = acc + lane_bcast(partial, __builtin_ctzll(ends));
        ends &= ends - 1ull;
      }
      return;
    }
    // acc = (..((acc + R0) + R1)..) + R(k-1) without a scalar loop over set bits: the run totals
    // are compacted to lanes 0..k-1 (one ds_permute; the other lanes park theirs above k), then
    // every lane repeats x = left neighbour's x + R (lane 0's neighbour is acc). Lane j is final
    // after j + 1 rounds and stays final, so k rounds (rounded up to the unroll) leave the
    // total in lane k - 1.
    const bool is_end = ((ends >> lane) & 1ull) != 0;
    const int rank = __builtin_amdgcn_mbcnt_hi(static_cast<unsigned>(ends >> 32),
                                               __builtin_amdgcn_mbcnt_lo(static_cast<unsigned>(ends), 0));
    const int dest = is_end ? rank : k + lane - rank;
    const float r = __int_as_float(__builtin_amdgcn_ds_permute(dest << 2, __float_as_int(partial)));
    float x = r;
    for (int t = 0; t < k; t += 4) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float left = __int_as_float(__builtin_amdgcn_update_dpp(
            __float_as_int(acc), __float_as_int(x), 0x138, 0xF, 0xF, false));
        x = left + r;
      }
    }
    acc = lane_bcast(x, k - 1);
  }

  // left-to-right sum of lanes s .. s+len-1 on top of `start` (len < 8)
  __device__ __forceinline__ float chain(float start, float v, int s, int len) {
    float rs = start;
    for (int i = 0; i < len; ++i) rs = rs + lane_bcast(v, s + i);
    return rs;
  }

  // General path: runs one by one (runs of 8+, runs that grow to 8+ across batches).
  __device__ __forceinline__ void feed_runs(unsigned long long m, int base, float v, const float* a,
                                            int lane) {
    while (m != 0) {
      const int s = __builtin_ctzll(m);
      const unsigned long long t = m >> s;
      const int len = (~t == 0) ? 64 - s : __builtin_ctzll(~t);
      if (s + len == 64) {  // touches the batch end: may continue in the next batch
        if (pend_len > 0) {  // (only when s == 0: the whole batch belongs to the pending run)
          pend_len += len;
        } else {
          pend_start = base + s;
          pend_len = len;
          if (len < 8) pend_sum = chain(0.f, v, s, len);
        }
        return;
      }
      if (pend_len > 0) {  // run that started in an earlier batch ends here (s == 0)
        if (pend_len + len < 8) {
          acc = acc + chain(pend_sum, v, 0, len);
          pend_len = 0;
        } else {
          pend_len += len;
          flush(a, lane);
        }
      } else if (len < 8) {  // sum straight from registers
        acc = acc + chain(0.f, v, s, len);
      } else {
        acc = acc + pairwise_sum<false, 8>(a + base + s, len, lane);
      }
      m &= ~(((1ull << len) - 1ull) << s);  // len < 64 here
    }
  }
};

// Copy a unit into this wave's LDS slice (or return the global pointer).
template <bool USE_LDS>
__device__ __forceinline__ const float* stage_unit(const float* g, int len, float* lds, int lane) {
  if constexpr (!USE_LDS) return g;
  if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
    const int n4 = len / 4;
    const float4* g4 = reinterpret_cast<const float4*>(g);
    float4* l4 = reinterpret_cast<float4*>(lds);
    for (int i = lane; i < n4; i += kWave) l4[i] = g4[i];
    for (int i = n4 * 4 + lane; i < len; i += kWave) lds[i] = g[i];
  } else {
    for (int i = lane; i < len; i += kWave) lds[i] = g[i];
  }
  return lds;
}

}  // namespace mi355q
