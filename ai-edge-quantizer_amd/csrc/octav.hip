// OCTAV clipping search (K5): the entry points and the route choice, the kernels in which ONE wave owns a unit
// (octav_kernel, octav_tail_kernel, octav_seg_kernel; octav_cols_kernel: a lane per channel), octav_pick_kernel, and
// the opt-in one-read octav_fast_kernel (not bit-exact). numpy_sum.h states the order NumPy adds in; the workgroup
// kernels are in octav_rows.hip (rows, groups), the lane-per-unit kernel in octav_unit_lanes.hip.
//
// Two kernels sit here because the compiler's whole-module passes resist a finer split: octav_tail_kernel shares the
// __noinline__ pairwise_sum with octav_kernel and octav_seg_kernel, and alone in a module that function inherits the
// tail's launch bounds and is compiled differently (its register spills move); octav_fast_kernel is the only caller
// that hands octav_step constants, and alone in a module they are propagated into it before it is inlined.
//
//   ref: algorithms/uniform_quantize/octav.py:30-112  (_guess_clipping_with_octav)
#include <cstdlib>

#include "numpy_sum.h"
#include "octav_common.h"

namespace mi355q {
namespace {

template <bool USE_LDS>
__global__ void octav_kernel(OctavArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const long long unit = static_cast<long long>(blockIdx.x) * (blockDim.x / kWave) + wave;
  const bool live = unit < a.units;
  const float* u = nullptr;
  if (live)
    u = stage_unit<USE_LDS>(a.x + unit * a.len, a.len, smem + static_cast<size_t>(wave) * a.lds_stride, lane);
  if constexpr (USE_LDS) __syncthreads();
  if (!live) return;

  const int len = a.len;
  const float qnan = __builtin_nanf("");
  float guess = 1.0f;
  unsigned long long moved = 0;  // iterations in which this unit's guess still moved
  for (int it = 0; it < a.max_iter; ++it) {
    RunSum pos, neg;
    const float hi = guess, lo = -guess;
    for (int base = 0; base < len; base += kWave) {
      const int i = base + lane;
      const float v = i < len ? u[i] : qnan;
      const unsigned long long mp = __ballot(v >= hi), mn = __ballot(v <= lo);
      // nothing selected and no run waiting for its end: the batch changes nothing
      if ((mp | mn) == 0 && (pos.pend_len | neg.pend_len) == 0) continue;
      pos.feed(mp, base, v, u, lane);
      neg.feed(mn, base, v, u, lane);
    }
    pos.flush(u, lane);
    neg.flush(u, lane);
    const OctavStep st = octav_step(guess, pos.acc, neg.acc, pos.count, neg.count, len, a.s,
                                    a.count_is_f64);
    if (lane == 0) a.hist[static_cast<long long>(it) * a.units + unit] = st.next;
    if (!st.close) moved |= 1ull << it;
    if (reached_fixed_point(guess, st.next)) {
      if (lane == 0) repeat_iterate(a, it, unit, st.next);
      break;
    }
    guess = st.next;
  }
  if (lane == 0) publish_moving(a.moving, moved);
}

// acc = (..((acc + R0) + R1)..) over the lanes set in `ends`, in lane order (R = that lane's `partial`).
// Few ends: a scalar loop over the set bits. Otherwise the run totals are compacted to lanes 0..k-1
// (one ds_permute; the other lanes park theirs above k), then every lane repeats x = left
// neighbour's x + R (lane 0's neighbour is acc): lane j is final after j + 1 rounds and stays
// final, so k rounds (rounded up to the unroll) leave the total in lane k - 1.
__device__ __forceinline__ float chain_ends(float acc, float partial, unsigned long long ends, int lane) {
  const int k = __builtin_popcountll(ends);
  if (k <= 3) {
    while (ends != 0) {
      acc = acc + lane_bcast(partial, __builtin_ctzll(ends));
      ends &= ends - 1ull;
    }
    return acc;
  }
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
  return lane_bcast(x, k - 1);
}

// One mask of a sparsely selected row, by ONE wave. `cv` / `cp` list the n elements that passed an
// earlier, lower guess (values and positions in the row, ascending): while the guess keeps
// growing, what it selects is a subset of them, so an iteration costs what it selects instead of a
// pass over the row. A run is a stretch of selected candidates at consecutive positions inside
// one 8192-chunk; lane l holds candidate base + l and its successor, so the link "my successor
// continues my run" needs no neighbour exchange. Runs shorter than 8 are summed left to right
// from +0.0 (NumPy's n < 8 loop) by rounds of "left neighbour's partial sum + mine", the run
// totals join the running total in order (chain_ends). A run of 8 or more candidates needs the
// eight-accumulator scheme: the caller is told (false) and repeats the iteration the dense way.
template <bool NEG>
__device__ __forceinline__ bool sparse_mask_sum(float* cv, unsigned short* cp, int n, float thr, float keep, int lane,
                                                float* sum_out, int* count_out, int* kept_out) {
  float acc = 0.f;
  int count = 0;
  int kept = 0;                 // the list shrinks as the guess grows: candidates beyond `keep` move to the front
  bool carry_link = false;      // lane 0 continues the run the previous batch ended with
  float carry_partial = 0.f;
  int carry_len = 0;
  for (int base = 0; base < n; base += kWave) {
    const int i = base + lane;
    const bool in = i < n, in1 = i + 1 < n;
    const float v = in ? cv[i] : 0.f, vn = in1 ? cv[i + 1] : 0.f;
    const int p = in ? static_cast<int>(cp[i]) : -1, pn = in1 ? static_cast<int>(cp[i + 1]) : -3;
    const bool sel = in && (NEG ? v <= thr : v >= thr);
    const bool seln = in1 && (NEG ? vn <= thr : vn >= thr);
    const bool linkn = sel && seln && pn == p + 1 && (pn & (kChunk - 1)) != 0;
    const unsigned long long S = __ballot(sel), Ln = __ballot(linkn);
    count += __builtin_popcountll(S);
    {
      // (in place: everything this batch reads is in registers, and what is kept lands at or below
      // the batch's own start)
      const bool stay = in && (NEG ? v <= keep : v >= keep);
      const unsigned long long K = __ballot(stay);
      const int at = kept + __builtin_amdgcn_mbcnt_hi(static_cast<unsigned>(K >> 32),
                                                     __builtin_amdgcn_mbcnt_lo(static_cast<unsigned>(K), 0));
      if (stay) { cv[at] = v; cp[at] = static_cast<unsigned short>(p); }
      kept += __builtin_popcountll(K);
    }
    const unsigned long long L = (Ln << 1) | (carry_link ? 1ull : 0ull);   // bit l: lane l continues lane l - 1's run
    unsigned long long c7 = L & (L << 1);
    c7 &= c7 << 2;
    c7 &= c7 << 3;                                                         // seven links in a row: a run of 8
    const int lead = carry_link ? __builtin_ctzll(~L) : 0;                 // elements of the carried run in this batch
    if (c7 != 0 || carry_len + lead >= 8) return false;
    float partial = sel ? v : 0.f;
    if (lane == 0 && carry_link) partial = carry_partial + v;
    const bool cont = lane != 0 && ((L >> lane) & 1ull) != 0;
    for (unsigned long long c = L & ~1ull; c != 0; c &= c << 1) {
      const float left = wave_shr1(partial);
      if (cont) partial = left + v;
    }
    const unsigned long long ends = S & ~Ln;
    if (ends != 0) acc = chain_ends(acc, partial, ends, lane);
    carry_link = (Ln >> 63) != 0;
    if (carry_link) {     // the open run started in this batch (fewer than seven links end at lane 63)
      carry_partial = lane_bcast(partial, 63);
      carry_len = __builtin_clzll(~L) + 1;
    }
  }
  *sum_out = acc;
  *count_out = count;
  *kept_out = kept;
  return true;
}

// The rest of a row's iterations on ONE wave: the candidates the row's workgroup listed are staged in
// LDS (a few KB) and re-tested against every new guess (sparse_mask_sum; the lists shrink as the
// guess grows). Should an iterate step below what the candidates passed, or a run of 8+ candidates
// show up, the wave falls back to scanning the row itself from global memory (the generic one-wave
// scheme of octav_kernel) for the iterations that are left -- correct whatever the data does.
__global__ __launch_bounds__(kWave) void octav_tail_kernel(OctavArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const long long unit = blockIdx.x;
  const int lane = threadIdx.x;
  const TailState ts = a.tail[unit];
  if (ts.next_it <= 0 || ts.next_it >= a.max_iter) return;
  const int cap = a.tail_cap, len = a.len;
  float* cv[2] = {smem, smem + cap};
  unsigned short* cp[2] = {reinterpret_cast<unsigned short*>(smem + 2 * cap), reinterpret_cast<unsigned short*>(smem + 2 * cap) + cap};
  int n[2] = {ts.n[0], ts.n[1]};
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const float* gv = a.tail_values + (unit * 2 + m) * cap;
    const unsigned short* gp = a.tail_pos + (unit * 2 + m) * cap;
    for (int i = lane; i < n[m]; i += kWave) { cv[m][i] = gv[i]; cp[m][i] = gp[i]; }
  }
  const float* u = a.x + unit * len;
  const float qnan = __builtin_nanf("");
  float guess = ts.guess, cand_guess = ts.cand_guess;
  unsigned long long moved = static_cast<unsigned long long>(ts.moved_lo) | (static_cast<unsigned long long>(ts.moved_hi) << 32);
  bool lists_ok = true;
  for (int it = ts.next_it; it < a.max_iter; ++it) {
    const float hi = guess, lo = -guess;
    float pos_sum = 0.f, neg_sum = 0.f;
    int cpos = 0, cneg = 0;
    bool have = false;
    if (lists_ok && guess >= cand_guess) {
      // candidates a little below the guess stay listed: an iterate that settles may step back by an ulp
      const float keep = hi * 0.998046875f;     // 1 - 2^-9
      int l0 = 0, l1 = 0;
      have = sparse_mask_sum<false>(cv[0], cp[0], n[0], hi, keep, lane, &pos_sum, &cpos, &l0) &&
             sparse_mask_sum<true>(cv[1], cp[1], n[1], lo, -keep, lane, &neg_sum, &cneg, &l1);
      if (have) { n[0] = l0; n[1] = l1; cand_guess = keep; }
    }
    if (!have) {
      lists_ok = false;          // (a failed pass leaves its list half compacted)
      RunSum pos, neg;
      for (int base = 0; base < len; base += kWave) {
        const int i = base + lane;
        const float v = i < len ? u[i] : qnan;
        const unsigned long long mp = __ballot(v >= hi), mn = __ballot(v <= lo);
        if ((mp | mn) == 0 && (pos.pend_len | neg.pend_len) == 0) continue;
        pos.feed(mp, base, v, u, lane);
        neg.feed(mn, base, v, u, lane);
      }
      pos.flush(u, lane);
      neg.flush(u, lane);
      pos_sum = pos.acc; neg_sum = neg.acc;
      cpos = static_cast<int>(pos.count); cneg = static_cast<int>(neg.count);
    }
    const OctavStep st = octav_step(guess, pos_sum, neg_sum, cpos, cneg, len, a.s, a.count_is_f64);
    if (lane == 0) a.hist[static_cast<long long>(it) * a.units + unit] = st.next;
    if (!st.close) moved |= 1ull << it;
    if (reached_fixed_point(guess, st.next)) {
      if (lane == 0) repeat_iterate(a, it, unit, st.next);
      break;
    }
    guess = st.next;
  }
  if (lane == 0) publish_moving(a.moving, moved);
}

// ---- general [outer, channels, inner] view: unit c = the `outer` segments x[o, c, :] -----
// NumPy hands each contiguous segment to the inner loop separately and keeps one running
// total per channel: acc = acc + pairwise(run) for every run of every segment, in order
// (tests/test_numpy_sum_model.py::test_mixed_reductions). One wave per channel; segments are
// read from global memory (L2-resident after the first Newton iteration).
__global__ void octav_seg_kernel(OctavArgs a, long long channels, long long outer) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const long long c = static_cast<long long>(blockIdx.x) * (blockDim.x / kWave) + wave;
  if (c >= channels) return;
  const int inner = a.len;
  const float qnan = __builtin_nanf("");
  float guess = 1.0f;
  unsigned long long moved = 0;  // iterations in which this unit's guess still moved
  for (int it = 0; it < a.max_iter; ++it) {
    RunSum pos, neg;
    long long npos = 0, nneg = 0;
    const float hi = guess, lo = -guess;
    for (long long o = 0; o < outer; ++o) {
      const float* u = a.x + (o * channels + c) * inner;
      for (int base = 0; base < inner; base += kWave) {
        const int i = base + lane;
        const float v = i < inner ? u[i] : qnan;
        pos.feed(__ballot(v >= hi), base, v, u, lane);
        neg.feed(__ballot(v <= lo), base, v, u, lane);
      }
      pos.flush(u, lane);
      neg.flush(u, lane);
      npos += pos.count;
      nneg += neg.count;
      pos.count = neg.count = 0;
    }
    const OctavStep st = octav_step(guess, pos.acc, neg.acc, npos, nneg, outer * inner, a.s, 1);
    if (lane == 0) a.hist[static_cast<long long>(it) * a.units + c] = st.next;
    if (!st.close) moved |= 1ull << it;
    if (reached_fixed_point(guess, st.next)) {
      if (lane == 0) repeat_iterate(a, it, c, st.next);
      break;
    }
    guess = st.next;
  }
  if (lane == 0) publish_moving(a.moving, moved);
}

// ---- channel-last units: x viewed as [outer, channels], one unit per channel -------------
// NumPy reduces the leading axes of a C-contiguous array row by row (`out[c] += x[o, c]`,
// masked elements skipped), i.e. each channel is a plain left-to-right float32 sum over o
// (tests/numpy_sum_model.py states and checks this). One lane per channel keeps that order and
// makes every load a coalesced row segment.
constexpr int kColsUnroll = 8;

__global__ __launch_bounds__(256) void octav_cols_kernel(OctavArgs a, long long channels) {
  const long long c_raw = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  const bool live = c_raw < channels;           // dead lanes shadow the last channel, write nothing
  const long long c = live ? c_raw : channels - 1;
  const long long outer = a.len;
  float guess = 1.0f;
  bool settled = false;
  unsigned long long moved = 0;  // iterations in which this unit's guess still moved
  for (int it = 0; it < a.max_iter; ++it) {
    const float hi = guess, lo = -guess;
    float pos = 0.f, neg = 0.f;
    long long npos = 0, nneg = 0;
    const float* p = a.x + c;
    long long o = 0;
    for (; o + kColsUnroll <= outer; o += kColsUnroll) {
      float v[kColsUnroll];
#pragma unroll
      for (int k = 0; k < kColsUnroll; ++k) v[k] = p[static_cast<long long>(k) * channels];
#pragma unroll
      for (int k = 0; k < kColsUnroll; ++k) {
        if (v[k] >= hi) { pos = pos + v[k]; ++npos; }
        if (v[k] <= lo) { neg = neg + v[k]; ++nneg; }
      }
      p += kColsUnroll * channels;
    }
    for (; o < outer; ++o, p += channels) {
      const float v = *p;
      if (v >= hi) { pos = pos + v; ++npos; }
      if (v <= lo) { neg = neg + v; ++nneg; }
    }
    const OctavStep st = octav_step(guess, pos, neg, npos, nneg, outer, a.s, a.count_is_f64);
    if (live && !settled) a.hist[static_cast<long long>(it) * a.units + c] = st.next;
    if (live && !settled && !st.close) moved |= 1ull << it;
    if (!settled && reached_fixed_point(guess, st.next)) {
      settled = true;
      if (live) repeat_iterate(a, it, c, st.next);
    }
    guess = st.next;
    if (__all(settled)) break;
  }
  // one lane per 64 channels publishes the union of the wave
  for (int off = kWave / 2; off > 0; off >>= 1) moved |= __shfl_xor(moved, off, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0) publish_moving(a.moving, moved);
}

// The reference stops at the first iteration where *every* unit is close
// (octav.py:109); every unit ran all iterations, so just pick that iterate.
__global__ __launch_bounds__(256) void octav_pick_kernel(const float* __restrict__ hist,
                                                        const unsigned long long* __restrict__ moving,
                                                        long long units, int max_iter, int early_stop,
                                                        float* __restrict__ clip, int* iters_out) {
  int k = max_iter - 1;
  if (early_stop)
    for (int it = 0; it < max_iter; ++it)
      if (((*moving >> it) & 1ull) == 0) { k = it; break; }
  const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (i < units) clip[i] = hist[static_cast<long long>(k) * units + i];
  if (i == 0 && iters_out != nullptr) *iters_out = k + 1;
}

struct UnitPlan {
  bool use_lds;
  int waves;       // waves (units) per block
  int lds_stride;  // floats
  size_t smem;
};

UnitPlan plan_units(int len) {
  UnitPlan p{};
  const int stride = (len + 3) / 4 * 4;
  const size_t per_wave = static_cast<size_t>(stride) * sizeof(float);
  constexpr size_t kBudget = 64 * 1024;  // per block: keeps >= 2 blocks per CU
  int waves = static_cast<int>(kBudget / (per_wave ? per_wave : 1));
  if (waves > 4) waves = 4;
  // (one-wave blocks would fit ten 16 KB slices per CU instead of eight; measured 12 % slower:
  // the loops are bound by scalar-instruction issue, not by waves in flight)
  if (waves >= 1) {
    p.use_lds = true;
    p.waves = waves;
    p.lds_stride = stride;
    p.smem = per_wave * waves;
  } else {
    p.use_lds = false;
    p.waves = 4;
    p.lds_stride = 0;
    p.smem = 0;
  }
  return p;
}

// ---------------------------------------------------------------- OCTAV, one read (opt-in, tolerance class T2) ---
// ref: algorithms/uniform_quantize/octav.py:30-112. The kernels above reproduce NumPy's float32 summation ORDER (pairwise
// over runs of selected elements) so that the clipping constants are the reference's bit for bit; the price is 0.045 of
// one read of the tensor. The reference pins neither NumPy nor its summation order (SURVEY 7 classes OCTAV as T2), so this
// kernel offers the other trade: a unit (row / block) stays in REGISTERS as |x| for all iterations -- one pass over HBM --
// and a masked sum is per-lane float32 partials (<= 64 elements each), a float32 tree over a wave's lanes and a float64
// sum over a unit's waves: within 1e-6 of the reference's scale, not bit-identical to it.
//   c <- sum_{|x| >= c} |x| / (f32(n_sel) (1 - s) + f64(s) N):  for c > 0 the reference's two masks (x >= c, x <= -c) are
// disjoint and their sums' difference is the sum of |x| over their union; for c == 0 (every weight tensor's second iterate:
// a first guess of 1 selects nothing) each zero sits in both masks, counted twice in n_sel as the reference counts it
// (octav.py:87-100). NaNs fail both tests there and `|x| >= c` here.
// The reference's early stop is global (octav.py:109): every unit runs all iterations, records its iterates and the
// iterations in which it still moved, and octav_pick_kernel takes the first iterate at which no unit moved.
struct OctavFastArgs {
  const float* x;
  long long units;
  int len;          // elements per unit, a multiple of 4
  int max_iter;
  float s;
  float* hist;      // [max_iter][units]
  unsigned long long* moving;
};

// Sum over the LANES (<= 64) lanes that own a unit, result on every one of them, without LDS traffic: butterflies inside a
// row of 16 lanes are DPP operands of the add itself (quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror); rows
// are combined through four v_readlane (the wave's four row totals in scalar registers). A ds_bpermute per step (what
// __shfl_xor compiles to) made the twelve dependent exchanges of one iteration cost more than its 64 compare-select-adds.
template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
template <int CTRL>
__device__ __forceinline__ int dpp_i32(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true); }

template <int LANES>
__device__ __forceinline__ float unit_sum_f32(float v) {
  if constexpr (LANES >= 2) v += dpp_f32<0xB1>(v);
  if constexpr (LANES >= 4) v += dpp_f32<0x4E>(v);
  if constexpr (LANES >= 8) v += dpp_f32<0x141>(v);
  if constexpr (LANES >= 16) v += dpp_f32<0x140>(v);
  if constexpr (LANES >= 32) {
    const int b = __builtin_bit_cast(int, v);
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0)), r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16));
    const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32)), r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48));
    if constexpr (LANES >= 64) v = (r0 + r1) + (r2 + r3);
    else v = (threadIdx.x & 32) ? r2 + r3 : r0 + r1;
  }
  return v;
}
template <int LANES>
__device__ __forceinline__ int unit_sum_i32(int v) {
  if constexpr (LANES >= 2) v += dpp_i32<0xB1>(v);
  if constexpr (LANES >= 4) v += dpp_i32<0x4E>(v);
  if constexpr (LANES >= 8) v += dpp_i32<0x141>(v);
  if constexpr (LANES >= 16) v += dpp_i32<0x140>(v);
  if constexpr (LANES >= 32) {
    const int r0 = __builtin_amdgcn_readlane(v, 0), r1 = __builtin_amdgcn_readlane(v, 16);
    const int r2 = __builtin_amdgcn_readlane(v, 32), r3 = __builtin_amdgcn_readlane(v, 48);
    if constexpr (LANES >= 64) v = (r0 + r1) + (r2 + r3);
    else v = (threadIdx.x & 32) ? r2 + r3 : r0 + r1;
  }
  return v;
}

// LANES lanes own a unit (1 .. 64: part of a wave or a wave; 256 / 1024: the workgroup), V float4 per lane.
template <int LANES, int V>
__global__ __launch_bounds__(LANES > 256 ? LANES : 256) void octav_fast_kernel(OctavFastArgs a) {
  constexpr int THREADS = LANES > 256 ? LANES : 256;
  constexpr int UPB = THREADS / LANES;                     // units per workgroup
  constexpr int WAVES = LANES / kWave;                    // waves per unit (0: several units per wave)
  const int l = threadIdx.x % LANES;
  const long long u = static_cast<long long>(blockIdx.x) * UPB + threadIdx.x / LANES;
  const bool live = u < a.units;
  const int len4 = a.len / 4;
  const float4* __restrict__ x4 = reinterpret_cast<const float4*>(a.x) + (live ? u : 0) * len4;
  const float qnan = __builtin_nanf("");
  // every load is issued before the first value is looked at (V 16-byte loads in flight per lane): slots past the
  // unit's end re-read its last piece and are blanked afterwards instead of branching around the load
  typedef float v4f __attribute__((ext_vector_type(4)));
  v4f raw[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const int c = j * LANES + l;
    raw[j] = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(&x4[c < len4 ? c : len4 - 1]));     // read once
  }
  float v[V][4];
  int zeros = 0;                                          // per lane, or -- units that own whole waves -- per wave
  float top = 0.f;                                        // this lane's largest |x| (fmaxf passes NaNs and blanks by)
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const bool mine = live && j * LANES + l < len4;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[j][e] = mine ? fabsf(raw[j][e]) : qnan;           // a blank slot, like a NaN, is never selected and never a zero
      top = fmaxf(top, v[j][e]);
      if constexpr (LANES >= kWave) zeros += __builtin_popcountll(__builtin_amdgcn_ballot_w64(v[j][e] == 0.f));
      else zeros += v[j][e] == 0.f;
    }
  }
  __shared__ double red_sum[2][WAVES > 0 ? WAVES : 1];
  __shared__ int red_cnt[2][WAVES > 0 ? WAVES : 1];
  float unit_top = 0.f;                                  // the unit's largest |x| (units that own whole waves)
  if constexpr (LANES >= kWave) {
    unit_top = top;
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) unit_top = fmaxf(unit_top, __shfl_xor(unit_top, off, kWave));
    if constexpr (WAVES > 1) {
      __shared__ float red_top[WAVES > 0 ? WAVES : 1];
      if ((threadIdx.x & (kWave - 1)) == 0) red_top[threadIdx.x / kWave] = unit_top;
      __syncthreads();
#pragma unroll
      for (int k = 0; k < WAVES; ++k) unit_top = fmaxf(unit_top, red_top[k]);
    }
  }
  float guess = 1.0f;
  unsigned long long moved = 0;
  int it = 0;
  for (; it < a.max_iter; ++it) {
    float part = 0.f;
    int cnt = 0;
    if constexpr (LANES >= kWave) {
      // The guess is the same on every lane of the wave: a guess above the unit's largest |x| (the first guess, 1, of
      // weights below 1) selects nothing, and the iteration costs nothing.
      if (!(guess > unit_top)) {
        float p0 = 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f;
#pragma unroll
        for (int j = 0; j < V; ++j) {
          // compare -> select -> lane count, element by element on VCC: left to the scheduler, the 64 compares are issued
          // first and their lane masks (128 scalar registers) spill through v_writelane / v_readlane
          // four elements per step, the four compares first: each lane mask (an SGPR pair of its own) is three
          // instructions old when its select and its s_bcnt1 read it, so neither waits for the compare to retire
          float t0, t1, t2, t3;
          int n0, n1, n2, n3;
          unsigned long long m0, m1, m2, m3;
          asm volatile(
              "v_cmp_ge_f32_e64 %[m0], %[x0], %[g]\n\tv_cmp_ge_f32_e64 %[m1], %[x1], %[g]\n\t"
              "v_cmp_ge_f32_e64 %[m2], %[x2], %[g]\n\tv_cmp_ge_f32_e64 %[m3], %[x3], %[g]\n\t"
              "v_cndmask_b32_e64 %[t0], 0, %[x0], %[m0]\n\tv_cndmask_b32_e64 %[t1], 0, %[x1], %[m1]\n\t"
              "v_cndmask_b32_e64 %[t2], 0, %[x2], %[m2]\n\tv_cndmask_b32_e64 %[t3], 0, %[x3], %[m3]\n\t"
              "s_bcnt1_i32_b64 %[n0], %[m0]\n\ts_bcnt1_i32_b64 %[n1], %[m1]\n\t"
              "s_bcnt1_i32_b64 %[n2], %[m2]\n\ts_bcnt1_i32_b64 %[n3], %[m3]\n\t"
              "v_add_f32 %[p0], %[p0], %[t0]\n\tv_add_f32 %[p1], %[p1], %[t1]\n\t"
              "v_add_f32 %[p2], %[p2], %[t2]\n\tv_add_f32 %[p3], %[p3], %[t3]\n\t"
              "s_add_i32 %[n0], %[n0], %[n1]\n\ts_add_i32 %[n2], %[n2], %[n3]\n\t"
              "s_add_i32 %[c], %[c], %[n0]\n\ts_add_i32 %[c], %[c], %[n2]"
              : [p0] "+v"(p0), [p1] "+v"(p1), [p2] "+v"(p2), [p3] "+v"(p3), [c] "+s"(cnt),
                [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2), [t3] "=&v"(t3),
                [n0] "=&s"(n0), [n1] "=&s"(n1), [n2] "=&s"(n2), [n3] "=&s"(n3),
                [m0] "=&s"(m0), [m1] "=&s"(m1), [m2] "=&s"(m2), [m3] "=&s"(m3)
              : [x0] "v"(v[j][0]), [x1] "v"(v[j][1]), [x2] "v"(v[j][2]), [x3] "v"(v[j][3]), [g] "v"(guess)
              : "scc");
        }
        part = (p0 + p1) + (p2 + p3);
        if (guess == 0.f) cnt += zeros;                  // every zero sits in both of the reference's masks
      }
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool sel = v[j][e] >= guess;
          part += sel ? v[j][e] : 0.f;
          cnt += sel;
        }
      cnt = unit_sum_i32<LANES>(cnt + (guess == 0.f ? zeros : 0));
    }
    // per-lane float32 partials (<= 64 elements), float32 tree over the wave's lanes, float64 across the unit's waves
    double sum = static_cast<double>(unit_sum_f32<(LANES < kWave ? LANES : kWave)>(part));
    if constexpr (WAVES > 1) {
      const int w = threadIdx.x / kWave, b = it & 1;
      if ((threadIdx.x & (kWave - 1)) == 0) { red_sum[b][w] = sum; red_cnt[b][w] = cnt; }
      __syncthreads();
      sum = 0.0; cnt = 0;
#pragma unroll
      for (int k = 0; k < WAVES; ++k) { sum += red_sum[b][k]; cnt += red_cnt[b][k]; }
    }
    const OctavStep st = octav_step(guess, static_cast<float>(sum), 0.f, cnt, 0, a.len, a.s, 1);
    if (live && l == 0) a.hist[static_cast<long long>(it) * a.units + u] = st.next;
    if (!st.close) moved |= 1ull << it;
    const bool fixed = reached_fixed_point(guess, st.next);
    guess = st.next;
    // every lane of a unit holds the same iterate: the unit leaves together; lanes of other units in the wave go on
    if constexpr (LANES >= kWave) {
      if (fixed) { ++it; break; }
    }
  }
  if constexpr (LANES >= kWave) {
    if (live && l == 0)
      for (int k = it; k < a.max_iter; ++k) a.hist[static_cast<long long>(k) * a.units + u] = guess;
  }
  if (!live) moved = 0;
  // one flag update per wave at most
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const unsigned lo = __shfl_xor(static_cast<unsigned>(moved), off, kWave);
    const unsigned hi = __shfl_xor(static_cast<unsigned>(moved >> 32), off, kWave);
    moved |= (static_cast<unsigned long long>(hi) << 32) | lo;
  }
  if ((threadIdx.x & (kWave - 1)) == 0) publish_moving(a.moving, moved);
}

template <int LANES, int V>
void launch_octav_fast(const OctavFastArgs& a, hipStream_t st) {
  constexpr int THREADS = LANES > 256 ? LANES : 256;
  constexpr int UPB = THREADS / LANES;
  hipLaunchKernelGGL((octav_fast_kernel<LANES, V>), dim3(static_cast<unsigned>((a.units + UPB - 1) / UPB)), dim3(THREADS), 0, st, a);
}

// the route every length can take: one wave per unit (octav_kernel)
int32_t launch_octav_wave(OctavArgs a, hipStream_t st) {
  const UnitPlan p = plan_units(a.len);
  a.lds_stride = p.lds_stride;
  const dim3 blk(p.waves * kWave);
  const dim3 grid(static_cast<unsigned>((a.units + p.waves - 1) / p.waves));
  if (p.use_lds)
    hipLaunchKernelGGL(octav_kernel<true>, grid, blk, p.smem, st, a);
  else
    hipLaunchKernelGGL(octav_kernel<false>, grid, blk, 0, st, a);
  MI355Q_CHECK_LAUNCH("octav launch");
  return MI355Q_OK;
}

// ---------------------------------------------------------------- what every entry point does first and last
enum class OctavEntry { kUnits, kOneRead, kNd };     // mi355q_octav_clip_f32, _fast_f32, _nd_f32

struct OctavCall {
  int32_t status;               // what the call returns when octav_begin says false
  float* hist;                  // [max_iter][units], the front of the workspace
  unsigned long long* moving;   // the 8-byte-aligned word behind it, cleared
  float s;                      // float32(4^-bits / divisor)
  hipStream_t st;
};

// Checks the arguments in the entry point's order (its own range checks where they always stood), carves the
// workspace, clears `moving` and computes s. The view is [outer, units, len]; outer is 1 for the two contiguous forms.
// false: return c->status -- a refusal, or MI355Q_OK when there are no units.
bool octav_begin(OctavEntry entry, const float* x, int64_t outer, int64_t units, int64_t len, int32_t bits,
                 int32_t max_iter, float exponent_divisor, const float* clip_out, void* workspace,
                 size_t workspace_bytes, void* stream, OctavCall* c) {
  const auto refuse = [c](int32_t status) { c->status = status; return false; };
  clear_error();
  if (outer < 0 || units < 0 || len < 0) return refuse(fail(MI355Q_BAD_ARG, "negative shape"));
  if (max_iter < 1 || max_iter > 64) return refuse(fail(MI355Q_BAD_ARG, "max_iter must be in [1, 64]"));
  if (bits < 1 || bits > 16) return refuse(fail(MI355Q_BAD_ARG, "bits must be in [1, 16]"));
  if (units == 0) return refuse(MI355Q_OK);
  if (outer == 0 || len == 0) return refuse(fail(MI355Q_BAD_SHAPE, "empty reduction unit"));
  if (entry == OctavEntry::kUnits && len > 0x7FFFFFFFLL - 64) return refuse(fail(MI355Q_UNSUPPORTED, "unit_len too large"));
  if (entry == OctavEntry::kOneRead && (len % 4 != 0 || len > 65536))
    return refuse(fail(MI355Q_UNSUPPORTED, "the one-read OCTAV kernel takes units of 4 .. 65536 elements, a multiple of 4 (got %lld):"
                                           " use mi355q_octav_clip_f32", static_cast<long long>(len)));
  if (entry == OctavEntry::kOneRead && units > 0x7FFFFFFFLL) return refuse(fail(MI355Q_UNSUPPORTED, "too many units"));
  if (entry == OctavEntry::kNd && (outer > 0x7FFFFFFFLL || len > 0x7FFFFFFFLL - 64 || outer * len > 0x7FFFFFFFLL))
    return refuse(fail(MI355Q_UNSUPPORTED, "reduction unit too large"));
  if (!x || !clip_out) return refuse(fail(MI355Q_BAD_ARG, "null pointer"));
  if (entry == OctavEntry::kOneRead && (reinterpret_cast<uintptr_t>(x) & 15u))
    return refuse(fail(MI355Q_BAD_ARG, "x must be 16-byte aligned"));
  const size_t need = mi355q_octav_workspace_bytes(units, max_iter);
  if (!workspace || workspace_bytes < need)
    return refuse(fail(MI355Q_BAD_ARG, "workspace too small: need %zu bytes", need));
  c->st = as_stream(stream);
  c->hist = static_cast<float*>(workspace);
  c->moving = reinterpret_cast<unsigned long long*>(c->hist + (units * max_iter + 1) / 2 * 2);
  if (hipMemsetAsync(c->moving, 0, sizeof(unsigned long long), c->st) != hipSuccess)
    return refuse(fail(MI355Q_HIP_ERROR, "hipMemsetAsync failed"));
  // scale = np.asarray(4.0 ** (-bits) / exponent_divisor, dtype=np.float32)  (octav.py:64)
  double p4 = 1.0;
  for (int i = 0; i < bits; ++i) p4 *= 0.25;
  c->s = static_cast<float>(p4 / static_cast<double>(exponent_divisor));
  c->status = MI355Q_OK;
  return true;
}

// octav_pick_kernel: the iterate of the first iteration in which no unit moved (or the last one).
int32_t octav_finish(const OctavCall& c, long long units, int32_t max_iter, int32_t early_stop, float* clip_out,
                     int32_t* iters_out) {
  hipLaunchKernelGGL(octav_pick_kernel, dim3(static_cast<unsigned>((units + 255) / 256)), dim3(256), 0, c.st,
                     c.hist, c.moving, units, max_iter, early_stop, clip_out, iters_out);
  MI355Q_CHECK_LAUNCH("octav pick launch");
  return MI355Q_OK;
}

}  // namespace

int32_t launch_octav_tail(const OctavArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(octav_tail_kernel, dim3(static_cast<unsigned>(a.units)), dim3(kWave), static_cast<size_t>(a.tail_cap) * 12, st, a);
  MI355Q_CHECK_LAUNCH("octav tail launch");
  return MI355Q_OK;
}

}  // namespace mi355q

using namespace mi355q;

extern "C" size_t mi355q_octav_workspace_bytes(int64_t units, int32_t max_iter) {
  if (units <= 0 || max_iter <= 0) return 0;
  return static_cast<size_t>(units) * max_iter * sizeof(float) + 64 * sizeof(int);
}

extern "C" size_t mi355q_octav_rows_workspace_bytes(int64_t units, int64_t unit_len, int32_t max_iter) {
  const size_t base = mi355q_octav_workspace_bytes(units, max_iter);
  if (base == 0 || unit_len < kRowsMinLen || unit_len > kRowsMaxLen) return base;
  const size_t cap = static_cast<size_t>(octav_tail_cap(static_cast<int>(unit_len)));
  return ((base + 63) & ~static_cast<size_t>(63)) + static_cast<size_t>(units) * (sizeof(TailState) + 2 * cap * (sizeof(float) + sizeof(unsigned short)));
}

extern "C" int32_t mi355q_octav_clip_f32(const float* x, int64_t units, int64_t unit_len,
                                         int32_t bits, int32_t max_iter, float exponent_divisor,
                                         int32_t early_stop, int32_t count_is_f64, float* clip_out,
                                         int32_t* iters_out, void* workspace,
                                         size_t workspace_bytes, void* stream) {
  OctavCall c;
  if (!octav_begin(OctavEntry::kUnits, x, 1, units, unit_len, bits, max_iter, exponent_divisor, clip_out, workspace,
                   workspace_bytes, stream, &c))
    return c.status;
  const OctavArgs a{x, units, static_cast<int>(unit_len), 0, max_iter, count_is_f64, c.s, c.hist, c.moving};
  // The routes, in the order they are tried; MI355Q_OCTAV_WAVE_KERNEL sends every length to the last one.
  int32_t status;
  if ((unit_len == 32 || unit_len == 64 || unit_len == 128 || unit_len == 256) && (reinterpret_cast<uintptr_t>(x) & 15) == 0 &&
      (units + kWave - 1) / kWave <= 0x7FFFFFFFLL && octav_unit_lanes_on() && !getenv("MI355Q_OCTAV_WAVE_KERNEL")) {
    // blockwise units: a lane per unit, the unit in registers (octav_unit_lanes_kernel)
    status = launch_octav_unit_lanes(a, c.st);
  } else if (unit_len >= kRowsMinLen && unit_len <= kRowsMaxLen && !getenv("MI355Q_OCTAV_WAVE_KERNEL")) {
    // rows of a weight matrix: a workgroup per row, the row in LDS (octav_rows_kernel, octav_tail_kernel)
    status = launch_octav_rows(a, workspace, workspace_bytes, c.st);
  } else if (unit_len >= 2 * kPiece && unit_len <= 512 && (unit_len & (unit_len - 1)) == 0 &&
             (units * unit_len) % kGroupLen == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 &&
             units * unit_len / kGroupLen <= 0x7FFFFFFFLL && !getenv("MI355Q_OCTAV_WAVE_KERNEL")) {
    // blockwise units: 4096 contiguous elements (8 .. 128 whole units) per workgroup (octav_groups_kernel)
    status = launch_octav_groups(a, c.st);
  } else {
    status = launch_octav_wave(a, c.st);
  }
  if (status != MI355Q_OK) return status;
  return octav_finish(c, units, max_iter, early_stop, clip_out, iters_out);
}

extern "C" int32_t mi355q_octav_clip_fast_f32(const float* x, int64_t units, int64_t unit_len, int32_t bits,
                                              int32_t max_iter, float exponent_divisor, int32_t early_stop,
                                              float* clip_out, int32_t* iters_out, void* workspace,
                                              size_t workspace_bytes, void* stream) {
  OctavCall c;
  if (!octav_begin(OctavEntry::kOneRead, x, 1, units, unit_len, bits, max_iter, exponent_divisor, clip_out, workspace,
                   workspace_bytes, stream, &c))
    return c.status;
  const OctavFastArgs a{x, units, static_cast<int>(unit_len), max_iter, c.s, c.hist, c.moving};
  const int len4 = static_cast<int>(unit_len / 4);
  if (len4 <= 4) launch_octav_fast<1, 4>(a, c.st);
  else if (len4 <= 8) launch_octav_fast<2, 4>(a, c.st);
  else if (len4 <= 16) launch_octav_fast<4, 4>(a, c.st);
  else if (len4 <= 32) launch_octav_fast<8, 4>(a, c.st);
  else if (len4 <= 64) launch_octav_fast<16, 4>(a, c.st);
  else if (len4 <= 128) launch_octav_fast<32, 4>(a, c.st);
  else if (len4 <= 256) launch_octav_fast<64, 4>(a, c.st);
  else if (len4 <= 512) launch_octav_fast<64, 8>(a, c.st);
  else if (len4 <= 1024) launch_octav_fast<64, 16>(a, c.st);
  else if (len4 <= 2048) launch_octav_fast<256, 8>(a, c.st);
  else if (len4 <= 4096) launch_octav_fast<256, 16>(a, c.st);
  else if (len4 <= 8192) launch_octav_fast<1024, 8>(a, c.st);
  else launch_octav_fast<1024, 16>(a, c.st);
  MI355Q_CHECK_LAUNCH("octav one-read launch");
  return octav_finish(c, units, max_iter, early_stop, clip_out, iters_out);
}

extern "C" int32_t mi355q_octav_clip_nd_f32(const float* x, int64_t outer, int64_t channels,
                                            int64_t inner, int32_t bits, int32_t max_iter,
                                            float exponent_divisor, int32_t early_stop, float* clip_out,
                                            int32_t* iters_out, void* workspace,
                                            size_t workspace_bytes, void* stream) {
  if (outer == 1)  // contiguous units: the LDS-staged kernel
    return mi355q_octav_clip_f32(x, channels, inner, bits, max_iter, exponent_divisor, early_stop, 1,
                                 clip_out, iters_out, workspace, workspace_bytes, stream);
  OctavCall c;
  if (!octav_begin(OctavEntry::kNd, x, outer, channels, inner, bits, max_iter, exponent_divisor, clip_out, workspace,
                   workspace_bytes, stream, &c))
    return c.status;
  // an axis is always given in this form, so s * N is evaluated in float64
  const OctavArgs a{x, channels, static_cast<int>(inner == 1 ? outer : inner), 0, max_iter, 1, c.s, c.hist, c.moving};
  if (inner == 1)
    hipLaunchKernelGGL(octav_cols_kernel, dim3(static_cast<unsigned>((channels + 255) / 256)), dim3(256), 0,
                       c.st, a, static_cast<long long>(channels));
  else
    hipLaunchKernelGGL(octav_seg_kernel, dim3(static_cast<unsigned>((channels + 3) / 4)), dim3(4 * kWave), 0,
                       c.st, a, static_cast<long long>(channels), static_cast<long long>(outer));
  MI355Q_CHECK_LAUNCH("octav nd launch");
  return octav_finish(c, channels, max_iter, early_stop, clip_out, iters_out);
}
