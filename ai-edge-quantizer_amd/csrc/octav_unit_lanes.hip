// OCTAV clipping search, order-exact, blockwise units of 32 / 64 / 128 / 256 elements: a lane per unit, the unit in
// registers (octav_unit_lanes_kernel). numpy_sum.h states the order NumPy adds in; octav.hip chooses the route.
#include <cstdlib>

#include "octav_common.h"

namespace mi355q {
namespace {

// ---- short units on LANES (the four blockwise granularities: 32 / 64 / 128 / 256 elements per unit) ----
//
// octav_groups_kernel (octav_rows.hip) treats a stretch of 4096 elements like a row: pieces of 16 on threads, run sums listed in
// LDS through a workgroup prefix sum, chains on a few lanes, two barriers per iteration (~15 vector instructions per
// element and mask, 0.039 of one read at 4096 x 4096 in blocks of 128). A unit this short needs none of that: LANE l of
// a wave owns unit 64 b + l, keeps its elements in REGISTERS for all iterations (16-register tuples read with a
// wave-uniform index, so the walks are loops) and walks them left to right as NumPy's masked reduction does -- nothing is
// exchanged between lanes, no run sum is listed, there is no barrier. An iteration is one of
//   the fast step (lane_step_pair), valid while every run is shorter than 8: seq = 0 + a0 + a1 + ... is NumPy's n < 8
//       loop, and acc = acc + seq where the run ends. Branch-free: every step adds (selected ? +0.0 : seq) to acc --
//       adding +0.0 is exact, a total that started at +0.0 is never -0.0 -- and sets seq = selected ? seq + x : +0.0, both
//       masks side by side, selections as sign bits of x - g and (-x) - g (no compare, no scalar register);
//   the long-aware step (lane_step_pair_long) wherever a run of 8+ is met -- the tuple in which a run reaches 8 is walked
//       again from the state it began with (walk_unit) -- and throughout at guess 0, the second iterate of a weight
//       tensor, where half of every mask is selected: the same step, and where a run of 8+ ENDS, NumPy's eight-accumulator
//       leaf over that run (from memory; only the lanes concerned) takes the place of seq;
//   the step by compares (lane_step_exact) for units that hold a NaN or an infinity and for iterates that are not finite;
//   and, once every live unit of the wave selects a handful of elements with growing iterates, a walk over per-lane
//       candidate lists in LDS (walk_candidates) instead of the unit.
// A lane that reached its fixed point is masked off; the wave leaves when all have. Bit-identical to octav_kernel /
// octav_groups_kernel (tests/test_gpu_octav_unit_lanes.py); how it got here, measured: profiles/r06_octav_unit_lanes.txt.
__device__ __forceinline__ float unit_leaf(const float* a, int n) {   // NumPy's leaf, 8 <= n <= 128
  float r[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) r[k] = a[k];
  const int full = n & ~7;
  if (full == 8) {
    // runs of 8 .. 15 (nearly all there are): the up to seven elements behind the accumulators are asked for together with
    // them -- one round trip to memory, not one per element of the tail
    float t[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) t[k] = 8 + k < n ? a[8 + k] : 0.f;
    float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
#pragma unroll
    for (int k = 0; k < 7; ++k) res = 8 + k < n ? res + t[k] : res;
    return res;
  }
  for (int i = 8; i < full; i += 8) {
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = r[k] + a[i + k];
  }
  float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (int i = full; i < n; ++i) res = res + a[i];
  return res;
}

// NumPy's pairwise sum of a run of 8 .. 256 elements: a leaf up to 128, beyond that the two halves (the first rounded
// down to a multiple of 8), each a leaf -- a unit of 256 needs one level of the recursion, no more.
template <bool WIDE>      // WIDE: units of 256 (shorter units never see the second case: one branch less at every site)
__device__ __forceinline__ float unit_long_run(const float* a, int n) {
  if (!WIDE || n <= 128) return unit_leaf(a, n);
  int n2 = n / 2;
  n2 -= n2 % 8;
  const float left = unit_leaf(a, n2);
  return left + unit_leaf(a + n2, n - n2);
}

struct LaneMask {
  float acc, seq;
  int cnt;
};

// One element, one mask, any run: compares, the run length kept, NumPy's leaf where a run of 8+ ends (the exact walk;
// `here` = the element's address).
template <bool NEG, bool WIDE>
__device__ __forceinline__ void lane_step_exact(LaneMask& m, int& len, float v, float thr, const float* here) {
  const bool sel = NEG ? v <= thr : v >= thr;
  float add = sel ? 0.f : m.seq;
  if (!sel && len >= 8) add = unit_long_run<WIDE>(here - len, len);
  m.acc = m.acc + add;
  m.seq = sel ? m.seq + v : 0.f;
  len = sel ? len + 1 : 0;
  m.cnt += sel ? 1 : 0;
}

// The fast walk's state: both masks, no compare and no scalar register anywhere (a v_cmp result crosses to the scalar
// file and back before a v_cndmask can use it: with the running totals depending on every select, that round trip was
// most of a step's time). For a guess g > 0 and a finite x:   x >= g  <=>  x - g is not negative,   x <= -g  <=>
// (-x) - g is not negative, and neither difference can be -0.0 (x - x = +0.0), so "not selected" is the difference's
// sign bit smeared over the word (one subtraction, one shift) and the selects are bit operations.
// The run lengths of both masks share a register (16 bits each) and so do the counts of unselected elements.
struct LanePair {
  float acc_p, seq_p, acc_n, seq_n;
  unsigned len2, unsel2, long2;     // [15:0] positive mask, [31:16] negative mask; long2 = OR of every len2 seen
};

// (as an instruction the compiler cannot look into: it rewrites (d >> 31) & y as d < 0 ? y : 0 -- the compare and select
// through the scalar file this walk exists to avoid)
__device__ __forceinline__ unsigned sign_smear(float d) {
  unsigned m;
  asm("v_ashrrev_i32 %0, 31, %1" : "=v"(m) : "v"(d));
  return m;
}

// (the additions as single instructions too: seen as C++, the two masks' additions are paired into v_pk_add_f32, whose
// second operand must be a register PAIR holding x twice -- a copy of the whole unit, spilled)
__device__ __forceinline__ float add_f32(float a_, float b_) {
  float r;
  asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a_), "v"(b_));
  return r;
}

__device__ __forceinline__ void lane_step_pair(LanePair& s, float v, float g) {
  const unsigned np_ = sign_smear(v - g);       // all ones: NOT selected
  const unsigned nn_ = sign_smear((-v) - g);
  s.acc_p = add_f32(s.acc_p, __uint_as_float(__float_as_uint(s.seq_p) & np_));   // + (selected ? +0.0 : seq)
  s.acc_n = add_f32(s.acc_n, __uint_as_float(__float_as_uint(s.seq_n) & nn_));
  s.seq_p = __uint_as_float(__float_as_uint(add_f32(s.seq_p, v)) & ~np_);        // selected ? seq + x : +0.0
  s.seq_n = __uint_as_float(__float_as_uint(add_f32(s.seq_n, v)) & ~nn_);
  const unsigned both = (np_ & 0xFFFFu) | (nn_ & 0xFFFF0000u);
  s.len2 = (s.len2 + 0x00010001u) & ~both;
  asm("v_or_b32 %0, %1, %2" : "=v"(s.long2) : "v"(s.long2), "v"(s.len2));   // (s.long2 |= s.len2 as C++ is turned into a
  s.unsel2 += both & 0x00010001u;                                           //  tree over all the unit's run lengths, kept live and spilled)
}

// (the second bound is waves per SIMD: 1 / 2 / 3 / 4 = 512 / 256 / 168 / 128 registers)
//
// The unit lives in 32-float register TUPLES read with a wave-uniform index (s_set_gpr_idx_on): the walks are loops of
// four steps, not LEN unrolled steps. Unrolled, the fast walk was 18 KB of straight-line code that every wave of the
// chip entered at the same moment: its first execution cost 20-25 us of instruction-cache misses, more than the walk.
typedef float v16f __attribute__((ext_vector_type(16)));

// (eight named 16-register tuples, not an array of them and not four of 32: the array went through scratch on its way
// into registers, and 32-register tuples were spilled whole when a second one had to be placed)
struct UnitRegs {
  v16f t0, t1, t2, t3, t4, t5, t6, t7, t8, t9, t10, t11, t12, t13, t14, t15;      // (units of 256: all sixteen)
};

// (tuples are handed around BY VALUE: a reference to a member plus a run-time element index is an address computation, and the
// struct then lives in scratch)
template <int T>
__device__ __forceinline__ v16f unit_tuple(const UnitRegs& r) {
  if constexpr (T == 0) return r.t0;
  else if constexpr (T == 1) return r.t1;
  else if constexpr (T == 2) return r.t2;
  else if constexpr (T == 3) return r.t3;
  else if constexpr (T == 4) return r.t4;
  else if constexpr (T == 5) return r.t5;
  else if constexpr (T == 6) return r.t6;
  else if constexpr (T == 7) return r.t7;
  else if constexpr (T == 8) return r.t8;
  else if constexpr (T == 9) return r.t9;
  else if constexpr (T == 10) return r.t10;
  else if constexpr (T == 11) return r.t11;
  else if constexpr (T == 12) return r.t12;
  else if constexpr (T == 13) return r.t13;
  else if constexpr (T == 14) return r.t14;
  else return r.t15;
}

template <int T>
__device__ __forceinline__ void set_unit_tuple(UnitRegs& r, v16f t) {
  if constexpr (T == 0) r.t0 = t;
  else if constexpr (T == 1) r.t1 = t;
  else if constexpr (T == 2) r.t2 = t;
  else if constexpr (T == 3) r.t3 = t;
  else if constexpr (T == 4) r.t4 = t;
  else if constexpr (T == 5) r.t5 = t;
  else if constexpr (T == 6) r.t6 = t;
  else if constexpr (T == 7) r.t7 = t;
  else if constexpr (T == 8) r.t8 = t;
  else if constexpr (T == 9) r.t9 = t;
  else if constexpr (T == 10) r.t10 = t;
  else if constexpr (T == 11) r.t11 = t;
  else if constexpr (T == 12) r.t12 = t;
  else if constexpr (T == 13) r.t13 = t;
  else if constexpr (T == 14) r.t14 = t;
  else r.t15 = t;
}

__device__ __forceinline__ float tuple_element(v16f t, int jj) { return t[jj]; }

template <int J0, int N, typename F>
__device__ __forceinline__ void each_slot(const UnitRegs& r, F&& f) {   // f(value) for positions J0 .. J0 + N - 1
  if constexpr (N > 0) {
    f(tuple_element(unit_tuple<J0 / 16>(r), J0 % 16));
    each_slot<J0 + 1, N - 1>(r, f);
  }
}

__device__ __forceinline__ void walk16(LanePair& s, v16f t, float guess) {
#pragma unroll 1
  for (int j = 0; j < 16; j += 4) {
    lane_step_pair(s, t[j], guess);
    lane_step_pair(s, t[j + 1], guess);
    lane_step_pair(s, t[j + 2], guess);
    lane_step_pair(s, t[j + 3], guess);
  }
}

// The same step for ANY run length and for guess 0 as well (finite data, finite guess >= 0): the differences get + 0.0 --
// nothing for a guess above zero, and at guess +0.0 it turns the one wrong sign, (-0.0) - (+0.0) = -0.0, into +0.0 (x >= +0.0
// holds for -0.0) -- and where a run of 8 or more ends, NumPy's leaf over that run (from memory, only the lanes concerned)
// takes the place of the left-to-right sum. Costs a compare and a branch per step more than lane_step_pair: this walk runs
// where the fast one reported a long run, and at guess 0, where nearly every unit has one.
template <bool WIDE>
__device__ __forceinline__ void lane_step_pair_long(LanePair& s, float v, float g, const float* at) {
  const unsigned np_ = sign_smear((v - g) + 0.f);
  const unsigned nn_ = sign_smear(((-v) - g) + 0.f);
  const unsigned both = (np_ & 0xFFFFu) | (nn_ & 0xFFFF0000u);
  float add_p = __uint_as_float(__float_as_uint(s.seq_p) & np_);
  float add_n = __uint_as_float(__float_as_uint(s.seq_n) & nn_);
  const unsigned ends_long = s.len2 & 0xFFF8FFF8u & both;       // a half that holds a length >= 8 and is not selected here
  if (ends_long != 0) {
    // (at most one of the two masks ends a long run at a given element: both would need the element before it in both
    // masks, which only a zero at guess 0 is -- and then this element, being finite, is in one of them. One site of the leaf.)
    const bool pos = (ends_long & 0xFFFFu) != 0;
    const int len = static_cast<int>(pos ? s.len2 & 0xFFFFu : s.len2 >> 16);
    const float sum = unit_long_run<WIDE>(at - len, len);
    add_p = pos ? sum : add_p;
    add_n = pos ? add_n : sum;
  }
  s.acc_p = add_f32(s.acc_p, add_p);
  s.acc_n = add_f32(s.acc_n, add_n);
  s.seq_p = __uint_as_float(__float_as_uint(add_f32(s.seq_p, v)) & ~np_);
  s.seq_n = __uint_as_float(__float_as_uint(add_f32(s.seq_n, v)) & ~nn_);
  s.len2 = (s.len2 + 0x00010001u) & ~both;
  s.unsel2 += both & 0x00010001u;
}

template <bool WIDE>
__device__ __forceinline__ void walk16_long(LanePair& s, v16f t, float guess, const float* at) {
#pragma unroll 1
  for (int j = 0; j < 16; ++j) lane_step_pair_long<WIDE>(s, t[j], guess, at + j);
}

// The full walk of the ordinary iterations, a tuple at a time: the fast steps, unless a run of 8+ is open where the tuple
// begins (then the long-aware steps at once) or reaches 8 inside it (then the tuple is walked AGAIN, from the state it
// began with, by the long-aware steps). A rare long run costs its wave sixteen slower steps -- walking the whole unit
// again cost that wave another iteration, and the kernel ends with its slowest wave.
template <int TUPLES, int T = 0>
__device__ __forceinline__ void walk_unit(LanePair& s, const UnitRegs& r, float guess, const float* u) {
  if constexpr (T < TUPLES) {
    bool long_steps = __ballot((s.len2 & 0xFFF8FFF8u) != 0) != 0;      // (wave-uniform)
    if (!long_steps) {
      const LanePair began = s;
      s.long2 = 0;
      walk16(s, unit_tuple<T>(r), guess);
      if (__ballot((s.long2 & 0x00F800F8u) != 0) != 0) {
        s = began;
        long_steps = true;
      }
    }
    if (long_steps) walk16_long<(TUPLES > 8)>(s, unit_tuple<T>(r), guess, u + 16 * T);
    walk_unit<TUPLES, T + 1>(s, r, guess, u);
  }
}

template <int TUPLES, int T = 0>
__device__ __forceinline__ void walk_unit_long(LanePair& s, const UnitRegs& r, float guess, const float* u) {
  if constexpr (T < TUPLES) {
    walk16_long<(TUPLES > 8)>(s, unit_tuple<T>(r), guess, u + 16 * T);
    walk_unit_long<TUPLES, T + 1>(s, r, guess, u);
  }
}

// ---- late iterations on a few candidates. Once an iterate grows, what it selects is a subset of what the previous one
// selected; the last iterations of a unit select a handful of elements and would still walk all of it. So when every live
// unit of the wave selected at most cand_capacity<LEN>() elements and its iterate grew, the next fast walk also LISTS what it selects
// (value and position per lane, in LDS: slot k of lane l at k * 64 + l), and the iterations after that walk the lists:
// the same step with one addition -- a gap between two candidates' positions ends the runs in front of it, exactly what
// walking over the unselected elements in between does (acc + seq, then seq = +0.0). An iterate below the one the list was
// made for (never seen on weights; the iteration does not forbid it) sends the wave back to full walks.
// capacity: 16 / 24 / 32 / 32 entries per lane for units of 32 / 64 / 128 / 256 (+ one slot that takes the unconditional store of a
// step that lists nothing). Measured at 4096 x 4096 (us per call): units of 128: 16 -> 107.7, 24 -> 93.4, 32 -> 91.1; of 64: 99.6 / 97.2 / 98.2;
// of 32: 81.5 / 95.2 / 111.5 (longer lists are walked in full by every later iteration).
template <int LEN>
constexpr int cand_capacity() { return LEN <= 32 ? 16 : (LEN <= 64 ? 24 : 32); }
constexpr int kCandNoPos = -4;     // position of an empty slot: never adjacent to anything

struct CandList {
  float* v;      // [capacity + 1][64]
  int* pos;      // [capacity + 1][64]
};

__device__ __forceinline__ void lane_step_pair_collect(LanePair& s, float v, float g, const CandList& c, int lane,
                                                       int position, int& count) {
  const unsigned np_ = sign_smear(v - g);
  const unsigned nn_ = sign_smear((-v) - g);
  c.v[count * kWave + lane] = v;                       // (overwritten by the next step unless this one is selected)
  c.pos[count * kWave + lane] = position;
  count += static_cast<int>(~(np_ & nn_) & 1u);        // selected by either mask
  s.acc_p = add_f32(s.acc_p, __uint_as_float(__float_as_uint(s.seq_p) & np_));
  s.acc_n = add_f32(s.acc_n, __uint_as_float(__float_as_uint(s.seq_n) & nn_));
  s.seq_p = __uint_as_float(__float_as_uint(add_f32(s.seq_p, v)) & ~np_);
  s.seq_n = __uint_as_float(__float_as_uint(add_f32(s.seq_n, v)) & ~nn_);
  const unsigned both = (np_ & 0xFFFFu) | (nn_ & 0xFFFF0000u);
  s.len2 = (s.len2 + 0x00010001u) & ~both;
  asm("v_or_b32 %0, %1, %2" : "=v"(s.long2) : "v"(s.long2), "v"(s.len2));
  s.unsel2 += both & 0x00010001u;
}

__device__ __forceinline__ void walk16_collect(LanePair& s, v16f t, float guess, const CandList& c, int lane, int base,
                                               int& count) {
#pragma unroll 1
  for (int j = 0; j < 16; j += 2) {
    lane_step_pair_collect(s, t[j], guess, c, lane, base + j, count);
    lane_step_pair_collect(s, t[j + 1], guess, c, lane, base + j + 1, count);
  }
}

template <int TUPLES, int T = 0>
__device__ __forceinline__ void walk_unit_collect(LanePair& s, const UnitRegs& r, float guess, const CandList& c, int lane,
                                                  int& count) {
  if constexpr (T < TUPLES) {
    walk16_collect(s, unit_tuple<T>(r), guess, c, lane, 16 * T, count);
    walk_unit_collect<TUPLES, T + 1>(s, r, guess, c, lane, count);
  }
}

// One pass over the first `slots` candidates (wave-uniform; a lane with fewer has empty slots: value 0, never selected
// by a guess above 0, position never adjacent). s.unsel2 counts the candidates NOT selected.
__device__ __forceinline__ void walk_candidates(LanePair& s, const CandList& c, int lane, int slots, float g) {
  int prev = kCandNoPos;
#pragma unroll 1
  for (int k = 0; k < slots; ++k) {
    const float v = c.v[k * kWave + lane];
    const int position = c.pos[k * kWave + lane];
    const unsigned gap = static_cast<unsigned>((prev + 1 - position) >> 31);     // positions ascend: all ones unless adjacent
    prev = position;
    const unsigned np_ = sign_smear(v - g);
    const unsigned nn_ = sign_smear((-v) - g);
    const unsigned ep = gap | np_, en = gap | nn_;      // the run in front of this element ends (or there is none)
    s.acc_p = add_f32(s.acc_p, __uint_as_float(__float_as_uint(s.seq_p) & ep));
    s.acc_n = add_f32(s.acc_n, __uint_as_float(__float_as_uint(s.seq_n) & en));
    s.seq_p = __uint_as_float(__float_as_uint(add_f32(__uint_as_float(__float_as_uint(s.seq_p) & ~ep), v)) & ~np_);
    s.seq_n = __uint_as_float(__float_as_uint(add_f32(__uint_as_float(__float_as_uint(s.seq_n) & ~en), v)) & ~nn_);
    const unsigned both = (np_ & 0xFFFFu) | (nn_ & 0xFFFF0000u);
    s.len2 = ((s.len2 & ~gap) + 0x00010001u) & ~both;
    asm("v_or_b32 %0, %1, %2" : "=v"(s.long2) : "v"(s.long2), "v"(s.len2));
    s.unsel2 += both & 0x00010001u;
  }
}

// the exact walk, tuple by tuple like the fast one (ONE loop over the unit with the tuple chosen by the position made
// the compiler keep a second copy of the unit in scratch and read it from there, a dependent load per step)
struct ExactWalk {
  LaneMask p, n;
  int lp, ln;
};

template <bool WIDE>
__device__ __forceinline__ void exact16(ExactWalk& w, v16f t, float hi, float lo, const float* at) {
#pragma unroll 1
  for (int j = 0; j < 16; ++j) {
    const float v = t[j];
    lane_step_exact<false, WIDE>(w.p, w.lp, v, hi, at + j);
    lane_step_exact<true, WIDE>(w.n, w.ln, v, lo, at + j);
  }
}

template <int TUPLES, int T = 0>
__device__ __forceinline__ void exact_unit(ExactWalk& w, const UnitRegs& r, float hi, float lo, const float* u) {
  if constexpr (T < TUPLES) {
    exact16<(TUPLES > 8)>(w, unit_tuple<T>(r), hi, lo, u + 16 * T);
    exact_unit<TUPLES, T + 1>(w, r, hi, lo, u);
  }
}

// tuples T0 .. T0 + N - 1 from this lane's LDS row (16 floats each)
template <int T0, int N>
__device__ __forceinline__ void tuples_from_lds(UnitRegs& r, const float* row) {
  if constexpr (N > 0) {
    v16f t;
#pragma unroll
    for (int p_ = 0; p_ < 16; ++p_) t[p_] = row[p_];
    set_unit_tuple<T0>(r, t);
    tuples_from_lds<T0 + 1, N - 1>(r, row + 16);
  }
}

// The load: positions H * STAGE .. (H + 1) * STAGE - 1 of the wave's 64 units per stage, whole lines from HBM (16 lanes per
// 256-byte stretch of a unit) turned through LDS so that lane l ends up with unit l. A stage's lines are asked for BEFORE the stage
// in front of it is turned (its trip through LDS then hides under their round trip to memory).
template <int LEN, int STAGE>
struct StageLines {
  float4 v[STAGE / 4];
};

template <int LEN, int STAGE, int H>
__device__ __forceinline__ StageLines<LEN, STAGE> ask_unit_stage(const float* base, long long wave_floats, int lane) {
  constexpr int kPer = STAGE / 4;              // float4 per unit and stage
  StageLines<LEN, STAGE> out;
#pragma unroll
  for (int q = 0; q < STAGE / 4; ++q) {        // 64 units x kPer float4 = kPer instructions of 64 lanes
    const int f = q * kWave + lane;
    const int uu = f / kPer, p4 = f % kPer;
    const long long e = static_cast<long long>(uu) * LEN + H * STAGE + p4 * 4;
    out.v[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (e < wave_floats) out.v[q] = *reinterpret_cast<const float4*>(base + e);
  }
  return out;
}

template <int LEN, int STAGE, int STRIDE, int H>
__device__ __forceinline__ void load_unit_stages(UnitRegs& xr, const float* base, long long wave_floats, float* lds, int lane,
                                                 const StageLines<LEN, STAGE>& mine) {
  constexpr int kPer = STAGE / 4;
  StageLines<LEN, STAGE> next;
  if constexpr (H + 1 < LEN / STAGE) next = ask_unit_stage<LEN, STAGE, H + 1>(base, wave_floats, lane);
#pragma unroll
  for (int q = 0; q < STAGE / 4; ++q) {
    const int f = q * kWave + lane;
    const int uu = f / kPer, p4 = f % kPer;
    float* d = lds + uu * STRIDE + p4 * 4;
    d[0] = mine.v[q].x; d[1] = mine.v[q].y; d[2] = mine.v[q].z; d[3] = mine.v[q].w;
  }
  __syncthreads();
  tuples_from_lds<H * STAGE / 16, STAGE / 16>(xr, lds + lane * STRIDE);
  __syncthreads();
  if constexpr (H + 1 < LEN / STAGE) load_unit_stages<LEN, STAGE, STRIDE, H + 1>(xr, base, wave_floats, lds, lane, next);
}

template <int LEN>
__global__ __launch_bounds__(kWave, LEN >= 256 ? 1 : (LEN >= 128 ? 2 : (LEN >= 64 ? 3 : 4))) void octav_unit_lanes_kernel(OctavArgs a) {
  constexpr int kStage = LEN < 64 ? LEN : 64;       // positions per trip through LDS
  constexpr int kStride = kStage + 1;               // floats per unit in LDS: lane l reads bank (l + p) % 32
  constexpr int kTuples = LEN / 16;
  constexpr int kCand = cand_capacity<LEN>();
  constexpr int kLdsFloats = kWave * kStride > 2 * (kCand + 1) * kWave ? kWave * kStride : 2 * (kCand + 1) * kWave;
  __shared__ float lds[kLdsFloats];    // the transposition's staging area, then the candidate lists
  const int lane = threadIdx.x;
  const long long unit0 = static_cast<long long>(blockIdx.x) * kWave;
  const long long unit = unit0 + lane;
  const bool live = unit < a.units;
  const float* u = a.x + (live ? unit : 0) * LEN;
  UnitRegs xr;
  // (a lane reading its own 16-byte pieces instead cost 25 us at 4096 x 4096: 64 lines per load instruction)
  {
    const float* base = a.x + unit0 * LEN;
    const long long wave_floats = (a.units - unit0 < kWave ? a.units - unit0 : kWave) * LEN;
    load_unit_stages<LEN, kStage, kStride, 0>(xr, base, wave_floats, lds, lane, ask_unit_stage<LEN, kStage, 0>(base, wave_floats, lane));
  }
  float amax = 0.f;     // NaN is never selected and never the maximum
  float poison = 0.f;   // x * 0 summed: NaN as soon as the unit holds a NaN or an infinity (those units: the exact walk only)
  each_slot<0, LEN>(xr, [&](float v) {
    amax = fmaxf(amax, fabsf(v));
    poison = __builtin_fmaf(v, 0.f, poison);
  });
  const bool special = poison != poison;
  float guess = 1.0f;
  bool done = !live;
  unsigned long long moved = 0;     // wave-uniform: iterations in which some unit of this wave still moved
  const CandList cand{lds, reinterpret_cast<int*>(lds + (kCand + 1) * kWave)};
  int mode = 0;                     // wave-uniform: 0 full walks, 1 the next walk lists what it selects, 2 the lists are walked
  int cand_slots = 0;               // wave-uniform: the longest list
  int cand_count = 0;               // this lane's list
  float cand_guess = 0.f;           // the iterate this lane's list was made for
  for (int it = 0; it < a.max_iter; ++it) {
    bool still_moving = false;
    bool may_list = false;          // after this iteration: few elements selected and the iterate grew
    if (mode == 2 && __ballot(!done && !(guess >= cand_guess)) != 0) mode = 0;      // (an iterate fell below its list)
    if (mode == 1) {                // (also for a unit this iterate selects nothing of: it walks nothing)
      cand_count = 0;
      cand_guess = guess;
    }
    if (!done) {
      LaneMask p{0.f, 0.f, 0}, n{0.f, 0.f, 0};
      if (guess <= amax) {      // (a guess above the unit's largest |x| selects nothing: the reference's first guess 1.0)
        // three walks. Units with special values and guesses that are not finite: compares (exact_unit). Guess 0 (a weight
        // tensor's second iterate: x >= 0 / x <= -0, a run of 8+ in nearly every unit) and the units whose fast walk met a
        // run of 8+: the sign-bit walk with the leaf where such a run ends (walk_unit_long). Everything else: the fast walk.
        const bool by_compares = special || !(guess >= 0.f) || !(guess < __builtin_inff());
        bool long_runs = !by_compares && !(guess > 0.f);
        if (__ballot(!by_compares && !long_runs) != 0) {
          LanePair s{0.f, 0.f, 0.f, 0.f, 0u, 0u, 0u};
          int walked = LEN;
          if (mode == 2) {
            walk_candidates(s, cand, lane, cand_slots, guess);
            walked = cand_slots;
          } else if (mode == 1) {
            walk_unit_collect<kTuples>(s, xr, guess, cand, lane, cand_count);
          } else {
            walk_unit<kTuples>(s, xr, guess, u);
            s.long2 = 0;         // (long runs were dealt with where they ended; one that touches the unit's end: below)
          }
          // a run that touches the unit's end ends there
          const int lp = static_cast<int>(s.len2 & 0xFFFFu), ln = static_cast<int>(s.len2 >> 16);
          p.acc = s.acc_p + (mode == 0 && lp >= 8 ? unit_long_run<(LEN > 128)>(u + LEN - lp, lp) : s.seq_p);
          n.acc = s.acc_n + (mode == 0 && ln >= 8 ? unit_long_run<(LEN > 128)>(u + LEN - ln, ln) : s.seq_n);
          p.cnt = walked - static_cast<int>(s.unsel2 & 0xFFFFu);
          n.cnt = walked - static_cast<int>(s.unsel2 >> 16);
          long_runs |= !by_compares && (s.long2 & 0x00F800F8u) != 0;      // (listing / list walks: some run reached 8)
        }
        if (long_runs) {
          LanePair s{0.f, 0.f, 0.f, 0.f, 0u, 0u, 0u};
          walk_unit_long<kTuples>(s, xr, guess, u);
          const int lp = static_cast<int>(s.len2 & 0xFFFFu), ln = static_cast<int>(s.len2 >> 16);
          p.acc = s.acc_p + (lp >= 8 ? unit_long_run<(LEN > 128)>(u + LEN - lp, lp) : s.seq_p);
          n.acc = s.acc_n + (ln >= 8 ? unit_long_run<(LEN > 128)>(u + LEN - ln, ln) : s.seq_n);
          p.cnt = LEN - static_cast<int>(s.unsel2 & 0xFFFFu);
          n.cnt = LEN - static_cast<int>(s.unsel2 >> 16);
        }
        if (by_compares) {
          const float hi = guess, lo = -guess;
          ExactWalk w{LaneMask{0.f, 0.f, 0}, LaneMask{0.f, 0.f, 0}, 0, 0};
          exact_unit<kTuples>(w, xr, hi, lo, u);
          p = w.p;
          n = w.n;
          p.acc = p.acc + (w.lp >= 8 ? unit_long_run<(LEN > 128)>(u + LEN - w.lp, w.lp) : p.seq);
          n.acc = n.acc + (w.ln >= 8 ? unit_long_run<(LEN > 128)>(u + LEN - w.ln, w.ln) : n.seq);
        }
      }
      const OctavStep st = octav_step(guess, p.acc, n.acc, p.cnt, n.cnt, LEN, a.s, a.count_is_f64);
      a.hist[static_cast<long long>(it) * a.units + unit] = st.next;
      still_moving = !st.close;
      may_list = !special && guess > 0.f && st.next >= guess && st.next < __builtin_inff() && p.cnt + n.cnt <= kCand;
      if (reached_fixed_point(guess, st.next)) {
        repeat_iterate(a, it, unit, st.next);
        done = true;
      }
      guess = st.next;
    }
    if (__ballot(still_moving) != 0) moved |= 1ull << it;      // (outside the divergent part: every lane keeps the wave's mask)
    if (__ballot(!done) == 0) break;
    if (mode == 1) {
      // the lists are complete: empty slots behind every lane's own, the longest list bounds the walks
      int longest = cand_count;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) longest = max(longest, __shfl_xor(longest, off));
      cand_slots = __builtin_amdgcn_readfirstlane(longest);
      for (int k = cand_count; k < cand_slots; ++k) {
        cand.v[k * kWave + lane] = 0.f;
        cand.pos[k * kWave + lane] = kCandNoPos;
      }
      mode = 2;
    } else if (mode == 0 && __ballot(!done && !may_list) == 0) {
      mode = 1;
    }
  }
  if (lane == 0) publish_moving(a.moving, moved);
}

}  // namespace

// MI355Q_OCTAV_UNIT_LANES=0: blockwise units take octav_groups_kernel again (A / B, tests compare the two)
bool octav_unit_lanes_on() {
  const char* e = getenv("MI355Q_OCTAV_UNIT_LANES");
  return e == nullptr || atoi(e) != 0;
}

int32_t launch_octav_unit_lanes(const OctavArgs& a, hipStream_t st) {
  const dim3 grid(static_cast<unsigned>((a.units + kWave - 1) / kWave));
  if (a.len == 32) hipLaunchKernelGGL(octav_unit_lanes_kernel<32>, grid, dim3(kWave), 0, st, a);
  else if (a.len == 64) hipLaunchKernelGGL(octav_unit_lanes_kernel<64>, grid, dim3(kWave), 0, st, a);
  else if (a.len == 128) hipLaunchKernelGGL(octav_unit_lanes_kernel<128>, grid, dim3(kWave), 0, st, a);
  else hipLaunchKernelGGL(octav_unit_lanes_kernel<256>, grid, dim3(kWave), 0, st, a);
  MI355Q_CHECK_LAUNCH("octav unit lanes launch");
  return MI355Q_OK;
}

}  // namespace mi355q
