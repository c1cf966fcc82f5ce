// What the OCTAV kernel families share: the argument block, one Newton update, the early-stop flags, and the
// families' launch functions (octav.hip has the entry points and the route choice).
//   ref: algorithms/uniform_quantize/octav.py:30-112  (_guess_clipping_with_octav)
#pragma once

#include "common.h"

namespace mi355q {

struct OctavArgs {
  const float* x;
  long long units;
  int len;          // elements per unit
  int lds_stride;   // floats per wave slice (multiple of 4)
  int max_iter;
  int count_is_f64; // axis given: s * N is evaluated in float64 (N is np.int64)
  float s;          // float32(4^-bits / divisor)
  float* hist;      // [max_iter][units] guesses
  unsigned long long* moving;  // bit `it` set: some unit's guess still moved in iteration `it`
  // octav_rows_kernel -> octav_tail_kernel hand-over (null: the rows kernel runs every iteration itself)
  struct TailState* tail;      // [units]
  float* tail_values;          // [units][2][tail_cap]: the candidates' values, positive mask first
  unsigned short* tail_pos;    // [units][2][tail_cap]: their positions in the row
  int tail_cap;
};

// What a row's workgroup leaves for the wave that finishes the row (octav_tail_kernel).
struct TailState {
  int next_it;          // first iteration the tail runs; 0: the rows kernel finished the row itself
  int n[2];             // candidates per mask
  float guess;          // the iterate to continue from
  float cand_guess;     // every listed candidate satisfies |x| >= cand_guess
  unsigned moved_lo, moved_hi;   // iterations (bit mask) in which the guess still moved so far
  int pad;
};

struct OctavStep {
  float next;
  bool close;
};

// One Newton update from the two masked sums and their element counts
// (ref octav.py:76-110), with NumPy's promotions spelled out.
__device__ __forceinline__ OctavStep octav_step(float guess, float pos_sum, float neg_sum,
                                                long long pos_count, long long neg_count,
                                                long long len, float s, int count_is_f64) {
  const float num = pos_sum - neg_sum;
  float den = static_cast<float>(pos_count);
  den = static_cast<float>(static_cast<double>(den) + static_cast<double>(neg_count));
  den = den * (1.0f - s);
  if (count_is_f64)
    den = static_cast<float>(static_cast<double>(den) +
                             static_cast<double>(s) * static_cast<double>(len));
  else
    den = den + s * static_cast<float>(len);
  const float next = num / den;
  // np.allclose(old, new): |old - new| <= atol + rtol * |new|, all float32
  const float tol = 1e-8f + 1e-5f * fabsf(next);
  const bool close = (fabsf(guess - next) <= tol && __builtin_isfinite(next)) || guess == next;
  return {next, close};
}

// The reference's early stop only asks whether *any* unit still moved in an iteration, so the
// units publish a bit mask instead of counting: one atomic per wave at most, and none when the
// bits are already there (a stale read only costs a redundant atomic). With 131 072 block units
// the per-iteration counters were ~1.3 M same-address atomics = 6.5 of the 7.3 ms.
__device__ __forceinline__ void publish_moving(unsigned long long* flags, unsigned long long moved) {
  if (moved == 0) return;
  const unsigned long long seen = __atomic_load_n(flags, __ATOMIC_RELAXED);
  if ((seen & moved) != moved) atomicOr(flags, moved);
}

// A Newton update that returns its own input (same value, hence the same two masks, the same
// sums and the same update again) has reached an exact fixed point: every later iteration of
// this unit would recompute the identical number and find it "close". The masks stop changing
// after a handful of iterations on real weights, so the remaining passes over the unit are
// skipped and their history entries filled in.
__device__ __forceinline__ bool reached_fixed_point(float guess, float next) { return next == guess; }

__device__ __forceinline__ void repeat_iterate(const OctavArgs& a, int it, long long unit, float value) {
  for (int r = it + 1; r < a.max_iter; ++r) a.hist[static_cast<long long>(r) * a.units + unit] = value;
}

// ---------------------------------------------------------------- routes of mi355q_octav_clip_f32 (octav.hip)
// Rows of kRowsMinLen .. kRowsMaxLen elements take octav_rows_kernel (octav_rows.hip tells how the lower bound was
// measured), pieces of kPiece elements on threads; power-of-two units up to 512 in stretches of kGroupLen elements take
// octav_groups_kernel.
#ifndef MI355Q_ROWS_MIN_LEN
#define MI355Q_ROWS_MIN_LEN 129
#endif
constexpr int kRowsMinLen = MI355Q_ROWS_MIN_LEN, kRowsMaxLen = 2 * 8192;   // (two of NumPy's chunks) up to 4 pieces per thread
constexpr int kPiece = 16;
constexpr int kGroupLen = 4096;

// Each family's launch: the kernel(s) of one route on `st`, MI355Q_OK or the failed launch's status. `a` is complete
// but for what only the family knows (LDS stride, the tail hand-over).
int32_t launch_octav_unit_lanes(const OctavArgs& a, hipStream_t st);                                      // octav_unit_lanes.hip
int32_t launch_octav_rows(OctavArgs a, void* workspace, size_t workspace_bytes, hipStream_t st);          // octav_rows.hip
int32_t launch_octav_groups(const OctavArgs& a, hipStream_t st);                                          // octav_rows.hip
int32_t launch_octav_tail(const OctavArgs& a, hipStream_t st);      // octav.hip: a one-wave kernel; launch_octav_rows calls it
bool octav_unit_lanes_on();     // MI355Q_OCTAV_UNIT_LANES
int octav_tail_cap(int len);    // candidates per mask a row may hand to its tail

}  // namespace mi355q
