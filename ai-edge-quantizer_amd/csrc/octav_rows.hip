// OCTAV clipping search, order-exact, pieces of 16 elements on threads: a workgroup per row (octav_rows_kernel; the
// one-wave octav_tail_kernel that finishes a row is in octav.hip) and a workgroup per 4096 elements of short units
// (octav_groups_kernel). numpy_sum.h states the order NumPy adds in; octav.hip chooses the route.
#include <cstdlib>

#include "numpy_sum.h"
#include "octav_common.h"

namespace mi355q {
namespace {

// ---- long contiguous units (1024 <= len <= 8192): one workgroup per unit, lanes own 16 elements ----
//
// Where the time went in octav_kernel on rows of 4096 weights (profiles/r01_octav_iterations...):
// with the guess at 0 each of the two masks selects every other element at random, a row has
// ~1000 runs per mask, and the running total `acc = acc + pairwise(run)` is a chain of ~2000
// dependent additions per row that ONE wave walked 64 elements at a time, with a scalar bit scan,
// DPP rounds and a ds_permute per batch (328 us for one iteration over 4096 rows), at one or two
// waves per SIMD because a 16 KB row sits behind every wave.
//
// Here a 256-thread workgroup owns a row (staged once in LDS for all iterations) and the work is
// split by what can be parallel:
//   masks   every wave compares its 64-element batches; thread t keeps the 16 mask bits of "its"
//           piece, elements [16 t, 16 t + 16). When the guess did not decrease (it never does after
//           the first update on real weights) the new selection is a subset of the old one, so
//           every thread just re-tests the set bits of its own old word: the cost follows the
//           number of selected elements;
//   runs    every thread walks the runs that START in its piece (bit scans on its own word; a run
//           that reaches the end of the piece continues through the following words, read from
//           LDS, up to NumPy's 8192-element chunk boundary) and sums each with NumPy's pairwise
//           scheme from LDS: left to right below 8 elements, eight strided accumulators up to 128,
//           runs longer than that (dense rows) by a whole wave. The sums land, in run order, in a
//           list in LDS (a workgroup prefix sum over the per-thread run counts gives the slots);
//   chain   acc = acc + R_j over the list: the only serial part. The positive and the negative
//           mask's chains run on two different waves at the same time (one wave issues one
//           addition per four cycles however the operands arrive); the lists are read with
//           broadcast 16-byte LDS loads, 32 entries ahead of the additions.
// The row is stored with one float of padding per 16 (thread-owned pieces start on distinct banks).
// (round 6: from 129 elements on -- 1024 until then. Units of 384 / 640 / 768 / 896 elements, the rows of small transformers'
// projections, took the one-wave-per-unit kernel: 0.63 ms per 2^24 elements against 0.37 / 0.26 / 0.23 / 0.21 ms here; 512
// took the groups kernel: 0.32 against 0.29 ms; 144 / 200 / 250: 0.78 / 0.72 / 0.66 against 0.75 / 0.58 / 0.48 ms. Below 128
// the one-wave kernel is the faster of the two; 32 / 64 / 128 / 256 elements are a lane's: octav_unit_lanes_kernel.)

__device__ __forceinline__ int pidx(int e) { return e + (e >> 4); }


// Wave-wide integer prefix sum on the DPP network (no LDS round trips): Hillis-Steele inside each
// row of 16 lanes (row_shr 1, 2, 4, 8; lanes without a source add 0), then lane 15 of rows 0 / 2
// into rows 1 / 3 (row_bcast:15) and lane 31 into rows 2 and 3 (row_bcast:31).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_add(int x) {
  return x + __builtin_amdgcn_update_dpp(0, x, CTRL, ROW_MASK, 0xF, true);
}

__device__ __forceinline__ int wave_incl_scan(int x) {
  x = dpp_add<0x111, 0xF>(x);
  x = dpp_add<0x112, 0xF>(x);
  x = dpp_add<0x114, 0xF>(x);
  x = dpp_add<0x118, 0xF>(x);
  x = x + __builtin_amdgcn_update_dpp(0, x, 0x142, 0xA, 0xF, false);   // row_bcast:15 -> rows 1, 3
  x = x + __builtin_amdgcn_update_dpp(0, x, 0x143, 0xC, 0xF, false);   // row_bcast:31 -> rows 2, 3
  return x;
}

// NumPy's pairwise sum of row[e0 .. e0 + n) (padded addressing), computed by ONE lane.
// n <= 128 (longer runs go to pairwise_wave below).
__device__ __forceinline__ float pairwise_lane(const float* row, int e0, int n) {
  if (n < 8) {
    float res = 0.f;
    for (int i = 0; i < n; ++i) res = res + row[pidx(e0 + i)];
    return res;
  }
  float r[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) r[k] = row[pidx(e0 + k)];
  const int full = n & ~7;
  for (int i = 8; i < full; i += 8) {
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = r[k] + row[pidx(e0 + i + k)];
  }
  float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (int i = full; i < n; ++i) res = res + row[pidx(e0 + i)];
  return res;
}

// The same for n > 128, by a whole wave (wave-uniform arguments): lanes 0..7 are the eight
// accumulators of a leaf, the recursion splits as NumPy does.
__device__ __forceinline__ float leaf_wave(const float* row, int e0, int m, int lane) {
  const int full = m & ~7;
  float r = 0.f;
  if (lane < 8) {
    r = row[pidx(e0 + lane)];
    for (int i = 8; i < full; i += 8) r = r + row[pidx(e0 + i + lane)];
  }
  const float r0 = lane_bcast(r, 0), r1 = lane_bcast(r, 1), r2 = lane_bcast(r, 2),
              r3 = lane_bcast(r, 3), r4 = lane_bcast(r, 4), r5 = lane_bcast(r, 5),
              r6 = lane_bcast(r, 6), r7 = lane_bcast(r, 7);
  float res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
  for (int i = full; i < m; ++i) res = res + row[pidx(e0 + i)];
  return res;
}

template <int DEPTH>
__device__ __noinline__ float pairwise_wave(const float* row, int e0, int n, int lane) {
  if (n <= 128) return leaf_wave(row, e0, n, lane);   // (n >= 8 here: halves of n > 128 are >= 64)
  if constexpr (DEPTH > 0) {
    int n2 = n / 2;
    n2 -= n2 % 8;
    const float left = pairwise_wave<DEPTH - 1>(row, e0, n2, lane);
    const float right = pairwise_wave<DEPTH - 1>(row, e0 + n2, n - n2, lane);
    return left + right;
  } else {
    return leaf_wave(row, e0, n, lane);  // unreachable for n <= 8192
  }
}

template <int W>
struct RowsShared {      // small per-workgroup exchange area (in front of the row in LDS)
  int wave_runs[2][4][W];   // [mask][slot][wave]: runs starting in that wave's pieces
  int wave_count[2][W];     // selected elements per wave
  int wave_changed[W];      // some word of the wave differs from the previous iteration's
  float sum[2];             // the two chain totals
  float wave_amax[W];       // largest |x| of the wave's pieces (written once, area 0)
};
// floats per exchange area (there are two, by iteration parity)
constexpr int rows_xchg_floats(int threads) { return threads <= 256 ? 64 : 256; }

// One mask of one piece: `word` = the 16 selection bits of elements x[0..16) (element e0 = 16 pc),
// `carry` = the element before the piece is selected too (same chunk). Writes the sums of the runs
// that START in this piece to list[j0 ...] in order.
//   * runs shorter than 8 that end inside the piece: a fixed 16-step pass over the registers --
//     cur = cur + (selected ? x : +0.0), flushed to the list where a run ends (no data-dependent
//     control flow; a step that ends no run stores to a per-thread dummy slot);
//   * a run that reaches the piece's end continues through the following words (LDS); shorter
//     than 8 in total: the left-to-right chain simply goes on over the row in LDS;
//   * runs of 8 .. 128 elements: eight strided accumulators (pairwise_lane, from LDS);
//   * longer runs (dense rows): reported back, summed by the whole wave afterwards.
__device__ __forceinline__ void piece_runs(const float (&x)[kPiece], unsigned word, unsigned carry, int pc,
                                           int npieces, const unsigned short* words, const float* row,
                                           float* list, float* dummy, int j0, int* long_e0, int* long_n,
                                           int* long_j, int qmask = kChunk / kPiece - 1) {
  // leading elements that continue a run started in an earlier piece are not this thread's business
  const unsigned lead = carry ? ((word + 1u) & ~word) - 1u : 0u;   // the low run of ones (if bit 0 is set)
  const unsigned w = word & ~lead & 0xFFFFu;
  const unsigned ends = w & ~(w >> 1) & 0x7FFFu;   // runs ending inside the piece (bit 15 = open end)
  float cur = 0.f;
  int j = j0;
#pragma unroll
  for (int i = 0; i < kPiece; ++i) {
    const int sel = static_cast<int>(w << (31 - i)) >> 31;      // 0 / -1
    cur = cur + __int_as_float(__float_as_int(x[i]) & sel);
    if (i < kPiece - 1) {
      const int fin = static_cast<int>(ends << (31 - i)) >> 31;
      float* dst = fin ? list + j : dummy;
      *dst = cur;
      j -= fin;
      cur = __int_as_float(__float_as_int(cur) & ~fin);
    }
  }
  // runs of 8+ elements that lie inside the piece (rare): redo them with the eight accumulators
  unsigned m8 = w & (w >> 1); m8 &= m8 >> 2; m8 &= m8 >> 4;      // bit i: ones at i .. i+7
  m8 &= ~(m8 << 1);                                              // ... and i is where they start
  const unsigned starts = w & ~(w << 1);
  while (m8 != 0) {
    const int i = __builtin_ctz(m8);
    m8 &= m8 - 1u;
    const int n = __builtin_ctz(~(w >> i));
    if (i + n < kPiece)    // (a run that reaches the end is handled below)
      list[j0 + __builtin_popcount(starts & ((1u << i) - 1u))] = pairwise_lane(row, kPiece * pc + i, n);
  }
  if (w >> (kPiece - 1)) {   // the last run is open: follow it
    const unsigned zeros = ~w & 0xFFFFu;
    const int i = zeros ? 32 - __builtin_clz(zeros) : 0;     // its first bit (0 when w is all ones)
    int n = kPiece - i;
    int q = pc + 1;
    while (q < npieces && (q & qmask) != 0) {   // (a run ends where NumPy's chunk -- or the unit -- does)
      const unsigned nx = words[q];
      if (nx == 0xFFFFu) { n += kPiece; ++q; continue; }
      n += __builtin_ctz(~nx);
      break;
    }
    const int e0 = kPiece * pc + i;
    float res = cur;
    if (n < 8) {
      for (int k = kPiece - i; k < n; ++k) res = res + row[pidx(e0 + k)];
    } else if (n <= 128) {
      res = pairwise_lane(row, e0, n);
    } else {
      *long_e0 = e0; *long_n = n; *long_j = j;
    }
    list[j] = res;
  }
}

// The same for a sparsely selected piece (late iterations select ~1 % of a row): a loop over
// the runs that start here instead of the fixed pass over all 16 elements -- the cost follows the
// number of runs (the caller takes this form when no lane of the wave has more than a few).
__device__ __forceinline__ void piece_runs_sparse(unsigned word, unsigned carry, int pc, int npieces,
                                                  const unsigned short* words, const float* row, float* list,
                                                  int j0, int* long_e0, int* long_n, int* long_j,
                                                  int qmask = kChunk / kPiece - 1) {
  const unsigned lead = carry ? ((word + 1u) & ~word) - 1u : 0u;
  const unsigned w = word & ~lead & 0xFFFFu;
  unsigned st = w & ~(w << 1);
  int j = j0;
  while (st != 0) {
    const int i = __builtin_ctz(st);
    st &= st - 1u;
    int n = __builtin_ctz(~(w >> i));            // bits above 15 - i read as "run ended"
    if (i + n == kPiece) {                       // reaches the end of the piece: follow it
      int q = pc + 1;
      while (q < npieces && (q & qmask) != 0) {
        const unsigned nx = words[q];
        if (nx == 0xFFFFu) { n += kPiece; ++q; continue; }
        n += __builtin_ctz(~nx);
        break;
      }
    }
    const int e0 = kPiece * pc + i;
    float res = 0.f;
    if (n == 1) {
      res = 0.f + row[pidx(e0)];
    } else if (n <= 128) {
      res = pairwise_lane(row, e0, n);
    } else {
      *long_e0 = e0; *long_n = n; *long_j = j;
    }
    list[j] = res;
    ++j;
  }
}

// THREADS = 64 / 128 / 256: rows of up to 1024 / 2048 elements leave half or three quarters of a
// 256-thread workgroup without a piece, so they get smaller workgroups (more rows per CU).
// THREADS = 512 / 1024 (one piece per thread) for rows of up to 8192 / 16384 elements: with 256
// threads and two to four pieces each, such a row (70 - 140 KB of LDS) left its CU with one wave
// per SIMD walking four pieces one after the other.
// 16-byte list loads the chain wave keeps in flight per half step: 8 (32 entries ahead) cost the whole workgroup 64
// VGPRs and left 26 - 29 spilled at the 128 the occupancy allows; 4 leave 4 - 8 spilled and are 2 - 4 % faster; 2 are slower
#ifndef MI355Q_OCTAV_CHAIN_Q
#define MI355Q_OCTAV_CHAIN_Q 4
#endif
template <int SLOTS, int THREADS>
__global__ __launch_bounds__(THREADS, THREADS >= 512 ? 4 : (SLOTS == 1 ? 4 : (SLOTS == 2 ? 2 : 1))) void octav_rows_kernel(OctavArgs a) {
  constexpr int kRowsThreads = THREADS, kWaves = THREADS / kWave;
  constexpr int kWavesAlloc = kWaves < 4 ? 4 : kWaves;      // (entries of absent waves stay 0)
  constexpr int kX = rows_xchg_floats(THREADS);
  using Shared = RowsShared<kWavesAlloc>;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const long long unit = blockIdx.x;
  const int len = a.len;
  const int npieces = (len + kPiece - 1) / kPiece;
  static_assert(sizeof(Shared) <= kX * sizeof(float), "exchange area");
  float* dummy = smem + 2 * kX + tid;                      // (two exchange areas in front)
  float* row = smem + 2 * kX + kRowsThreads;
  const int row_floats = (pidx(len) + 4) & ~3;
  float* list_pos = row + row_floats;                       // run sums of the two masks, in run order
  const int cap = ((len / 2 + 2 + 63) & ~63) + 64;         // (+ one per 8192-chunk) + the chain's read-ahead
  float* list_neg = list_pos + cap;
  unsigned short* words_pos = reinterpret_cast<unsigned short*>(list_neg + cap);
  unsigned short* words_neg = words_pos + ((npieces + 1) & ~1);

  for (int i = tid; i < 2 * kX; i += THREADS) smem[i] = 0.f;   // both exchange areas: waves this workgroup does not have count as 0
  __syncthreads();
  // ---- stage the unit: every thread keeps its pieces in registers for all iterations (one HBM
  // read), the row also goes to LDS for the runs that leave a piece
  const float qnan = __builtin_nanf("");
  float x[SLOTS][kPiece];
  float before[SLOTS];      // the element in front of each piece (same chunk), else NaN
  {
    const float* g = a.x + unit * len;
    const bool al = (reinterpret_cast<uintptr_t>(g) & 15) == 0;
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
      const int e0 = kPiece * (tid + kRowsThreads * s);
      if (al && e0 + kPiece <= len) {
        const float4* g4 = reinterpret_cast<const float4*>(g + e0);
        const float4 v0 = g4[0], v1 = g4[1], v2 = g4[2], v3 = g4[3];
        x[s][0] = v0.x; x[s][1] = v0.y; x[s][2] = v0.z; x[s][3] = v0.w;
        x[s][4] = v1.x; x[s][5] = v1.y; x[s][6] = v1.z; x[s][7] = v1.w;
        x[s][8] = v2.x; x[s][9] = v2.y; x[s][10] = v2.z; x[s][11] = v2.w;
        x[s][12] = v3.x; x[s][13] = v3.y; x[s][14] = v3.z; x[s][15] = v3.w;
      } else {
#pragma unroll
        for (int i = 0; i < kPiece; ++i) x[s][i] = e0 + i < len ? g[e0 + i] : qnan;
      }
    }
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
      const int e0 = kPiece * (tid + kRowsThreads * s);
      const int p = pidx(e0);
#pragma unroll
      for (int i = 0; i < kPiece; ++i)
        if (e0 + i < len) row[p + i] = x[s][i];
    }
  }
  {
    // largest |x| of the row (NaN ignored: a NaN is never selected): a guess above it selects nothing
    float am = 0.f;
#pragma unroll
    for (int s = 0; s < SLOTS; ++s)
#pragma unroll
      for (int i = 0; i < kPiece; ++i) am = fmaxf(am, fabsf(x[s][i]));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) am = fmaxf(am, __shfl_xor(am, off));
    if (lane == 0) reinterpret_cast<Shared*>(smem)->wave_amax[wave] = am;
  }
  __syncthreads();
  float row_amax = 0.f;
#pragma unroll
  for (int k = 0; k < kWavesAlloc; ++k) row_amax = fmaxf(row_amax, reinterpret_cast<Shared*>(smem)->wave_amax[k]);
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) {
    const int pc = tid + kRowsThreads * s;
    before[s] = (pc > 0 && pc < npieces && (pc & (kChunk / kPiece - 1)) != 0) ? row[pidx(kPiece * pc - 1)] : qnan;
  }

  unsigned wp[SLOTS], wn[SLOTS];
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) wp[s] = wn[s] = 0u;
  float guess = 1.0f;
  float pos_sum = 0.f, neg_sum = 0.f;
  int cp = 0, cn = 0;
  unsigned long long moved = 0;
  // the serial chain runs on one wave per workgroup: spread it over the SIMDs of the CU
  // (workgroups u, u + 256, u + 512, ... tend to be co-resident)
  const int chain_wave = static_cast<int>((unit + (unit >> 8)) % kWaves);
  // late iterations select a few per cent of a row: the candidates are listed once and a single wave
  // per row (octav_tail_kernel: no row in LDS, no barriers, dozens of rows per CU) finishes the row
  constexpr bool kCanHandOver = SLOTS == 1;
  const int cand_cap = a.tail_cap;
  bool force = true, handed_over = false;
  int nit = 0;      // iterations that exchanged something (the exchange areas alternate with it)
  int scan_p = 0, scan_n = 0;   // the last dense iteration's inclusive scans of selected elements inside the wave
  for (int it = 0; it < a.max_iter; ++it) {
#if !defined(MI355Q_OCTAV_HOISTED)
    // The per-lane LDS addresses of an iteration (this thread's mask words, its dummy slot, its wave's exchange slots)
    // are functions of the thread index alone: hoisted out of the loop they are eight VGPRs that live across every
    // iteration -- and at the 128 VGPRs four rows per CU allow, eight scratch dwords per lane (33 MB of dirty lines
    // per 4096 x 4096 call, profiles/r05_octav_exact_writes.txt). Laundering the index makes them this iteration's
    // values: a dozen integer instructions per iteration instead, no scratch in any instantiation, and 4096 x 4096
    // went from 187 to 175 us (profiles/r06_octav_remat.txt; -DMI355Q_OCTAV_HOISTED restores the hoisted form).
    int tid_now = threadIdx.x;
    asm volatile("" : "+v"(tid_now));
    const int tid = tid_now, lane = tid_now & (kWave - 1), wave = tid_now >> 6;
    float* dummy = smem + 2 * kX + tid;
#endif
    const float hi = guess, lo = -guess;
    bool have_sums = false;
    if (guess > row_amax) {
      // nothing reaches the guess (the reference's first guess 1.0 on ordinary weights): empty masks
#pragma unroll
      for (int s = 0; s < SLOTS; ++s) wp[s] = wn[s] = 0u;
      pos_sum = neg_sum = 0.f;
      cp = cn = 0;
      force = true;
      have_sums = true;
    }
    if (!have_sums) {
    // (two exchange areas, alternating: an iteration whose masks did not change has only
    // one barrier, so a fast wave may already publish the next iteration's counts while a slow one
    // still reads this one's)
    Shared* sh = reinterpret_cast<Shared*>(smem + kX * (nit & 1));
    ++nit;
    // ---- masks of the thread's own pieces, from registers
    unsigned changed = 0;
    unsigned sp[SLOTS], sn[SLOTS];   // run starts
    int pre_p[SLOTS], pre_n[SLOTS];
    int tp = 0, tn = 0;
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
      unsigned np_ = 0, nn_ = 0;
#pragma unroll
      for (int i = 0; i < kPiece; ++i) {
        np_ |= x[s][i] >= hi ? 1u << i : 0u;
        nn_ |= x[s][i] <= lo ? 1u << i : 0u;
      }
      changed |= (np_ ^ wp[s]) | (nn_ ^ wn[s]);
      wp[s] = np_; wn[s] = nn_;
      const int pc = tid + kRowsThreads * s;
      if (pc < npieces) {
        words_pos[pc] = static_cast<unsigned short>(np_);
        words_neg[pc] = static_cast<unsigned short>(nn_);
      }
      tp += __builtin_popcount(np_);
      tn += __builtin_popcount(nn_);
      const unsigned cpos = before[s] >= hi ? 1u : 0u, cneg = before[s] <= lo ? 1u : 0u;
      sp[s] = np_ & ~((np_ << 1) | cpos) & 0xFFFFu;
      sn[s] = nn_ & ~((nn_ << 1) | cneg) & 0xFFFFu;
      const int ip = wave_incl_scan(__builtin_popcount(sp[s])), in = wave_incl_scan(__builtin_popcount(sn[s]));
      pre_p[s] = ip - __builtin_popcount(sp[s]);
      pre_n[s] = in - __builtin_popcount(sn[s]);
      if (lane == kWave - 1) { sh->wave_runs[0][s][wave] = ip; sh->wave_runs[1][s][wave] = in; }
    }
    tp = wave_incl_scan(tp);
    tn = wave_incl_scan(tn);
    scan_p = tp; scan_n = tn;
    const bool wave_changed = __ballot(changed != 0) != 0;
    if (lane == kWave - 1) {
      sh->wave_count[0][wave] = tp; sh->wave_count[1][wave] = tn;
      sh->wave_changed[wave] = wave_changed ? 1 : 0;
    }
    __syncthreads();
    bool any_changed;
    if constexpr (kWavesAlloc > 4) {
      any_changed = __ballot(lane < kWavesAlloc && sh->wave_changed[lane] != 0) != 0;
    } else {
      any_changed = (sh->wave_changed[0] | sh->wave_changed[1] | sh->wave_changed[2] | sh->wave_changed[3]) != 0;
    }
    if (any_changed || force) {
      force = false;
      // (the same masks give the same sums and counts: late iterations mostly skip all of this)
      int npos = 0, nneg = 0;
      if constexpr (kWavesAlloc > 4) {
        // many waves, one slot: lane k holds wave k's figures, one scan per figure on the DPP network
        static_assert(SLOTS == 1, "wide workgroups own one piece per thread");
        const int uw = __builtin_amdgcn_readfirstlane(wave);
        const bool in = lane < kWavesAlloc;
        const int ip = wave_incl_scan(in ? sh->wave_runs[0][0][lane] : 0);
        const int inn = wave_incl_scan(in ? sh->wave_runs[1][0][lane] : 0);
        const int icp = wave_incl_scan(in ? sh->wave_count[0][lane] : 0);
        const int icn = wave_incl_scan(in ? sh->wave_count[1][lane] : 0);
        npos = __builtin_amdgcn_readlane(ip, kWavesAlloc - 1);
        nneg = __builtin_amdgcn_readlane(inn, kWavesAlloc - 1);
        cp = __builtin_amdgcn_readlane(icp, kWavesAlloc - 1);
        cn = __builtin_amdgcn_readlane(icn, kWavesAlloc - 1);
        if (uw > 0) {
          pre_p[0] += __builtin_amdgcn_readlane(ip, uw - 1);
          pre_n[0] += __builtin_amdgcn_readlane(inn, uw - 1);
        }
      } else {
        cp = cn = 0;
#pragma unroll
        for (int k = 0; k < kWavesAlloc; ++k) { cp += sh->wave_count[0][k]; cn += sh->wave_count[1][k]; }
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
          int bp = npos, bn = nneg;   // runs of earlier slots, then of earlier waves of this slot
#pragma unroll
          for (int k = 0; k < kWavesAlloc; ++k) {
            const int c0 = sh->wave_runs[0][s][k], c1 = sh->wave_runs[1][s][k];
            if (k < wave) { bp += c0; bn += c1; }
            npos += c0; nneg += c1;
          }
          pre_p[s] += bp; pre_n[s] += bn;
        }
      }
      // ---- run sums, in run order
      int long_e0[2 * SLOTS], long_n[2 * SLOTS], long_j[2 * SLOTS];
#pragma unroll
      for (int s = 0; s < SLOTS; ++s) {
        const int pc = tid + kRowsThreads * s;
        long_n[2 * s] = long_n[2 * s + 1] = 0;
        long_e0[2 * s] = long_e0[2 * s + 1] = long_j[2 * s] = long_j[2 * s + 1] = 0;
        // (wave-uniform choice per mask: the fixed 16-step pass costs ~240 instructions whatever
        // is selected, the run loop ~30 per run of the busiest lane)
        const bool sparse_p = __ballot(__builtin_popcount(sp[s]) > 3) == 0;
        const bool sparse_n = __ballot(__builtin_popcount(sn[s]) > 3) == 0;
        if (pc < npieces) {
          if (sparse_p)
            piece_runs_sparse(wp[s], before[s] >= hi ? 1u : 0u, pc, npieces, words_pos, row, list_pos,
                              pre_p[s], &long_e0[2 * s], &long_n[2 * s], &long_j[2 * s]);
          else
            piece_runs(x[s], wp[s], before[s] >= hi ? 1u : 0u, pc, npieces, words_pos, row, list_pos, dummy,
                       pre_p[s], &long_e0[2 * s], &long_n[2 * s], &long_j[2 * s]);
          if (sparse_n)
            piece_runs_sparse(wn[s], before[s] <= lo ? 1u : 0u, pc, npieces, words_neg, row, list_neg,
                              pre_n[s], &long_e0[2 * s + 1], &long_n[2 * s + 1], &long_j[2 * s + 1]);
          else
            piece_runs(x[s], wn[s], before[s] <= lo ? 1u : 0u, pc, npieces, words_neg, row, list_neg, dummy,
                       pre_n[s], &long_e0[2 * s + 1], &long_n[2 * s + 1], &long_j[2 * s + 1]);
        }
      }
      // dense rows: runs longer than 128 elements, one at a time by the wave that found them
#pragma unroll
      for (int k = 0; k < 2 * SLOTS; ++k) {
        unsigned long long pending = __ballot(long_n[k] > 0);
        while (pending != 0) {
          const int src = __builtin_ctzll(pending);
          pending &= pending - 1ull;
          const int e0 = __builtin_amdgcn_readlane(long_e0[k], src);
          const int n = __builtin_amdgcn_readlane(long_n[k], src);
          const int j = __builtin_amdgcn_readlane(long_j[k], src);
          const float res = pairwise_wave<8>(row, e0, n, lane);
          if (lane == 0) ((k & 1) ? list_neg : list_pos)[j] = res;
        }
      }
      // whole blocks of 64 entries, both lists padded to the longer one: no tail code in the chain
      // (adding +0.0 padding is exact: a running total that started at +0.0 is never -0.0)
      const int kp = (npos + 63) & ~63, kn = (nneg + 63) & ~63;
      const int kmax = kp > kn ? kp : kn;
      for (int j = npos + tid; j < kmax; j += kRowsThreads) list_pos[j] = 0.f;
      for (int j = nneg + tid; j < kmax; j += kRowsThreads) list_neg[j] = 0.f;
      __syncthreads();
      // ---- the chains: acc = acc + R_j in run order. A wave issues one dependent addition per four
      // cycles however many lanes take part, so ONE wave walks both lists at once: even lanes the
      // positive mask's, odd lanes the negative's (per-lane LDS addresses, two distinct ones per
      // load). Software pipelined by hand: the eight 16-byte loads of the NEXT 32 entries are issued,
      // then the 32 dependent additions of the current ones run while those loads are in flight
      // (the scheduling barriers keep the compiler from sinking the loads back behind the additions;
      // it still places the s_waitcnt itself). The lists are over-allocated by one block: what the
      // last read-ahead fetches is never added.
      if (wave == chain_wave) {
        const float4* l4 = reinterpret_cast<const float4*>((lane & 1) ? list_neg : list_pos);
        constexpr int Q = MI355Q_OCTAV_CHAIN_Q;      // 16-byte loads in flight per half step
        const int npair = kmax / (8 * Q);
        float acc = 0.f;
        float4 qa[Q], qb[Q];
#pragma unroll
        for (int k = 0; k < Q; ++k) qa[k] = l4[k];
        for (int pr = 0; pr < npair; ++pr) {
#pragma unroll
          for (int k = 0; k < Q; ++k) qb[k] = l4[(2 * pr + 1) * Q + k];
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int k = 0; k < Q; ++k) { acc = acc + qa[k].x; acc = acc + qa[k].y; acc = acc + qa[k].z; acc = acc + qa[k].w; }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int k = 0; k < Q; ++k) qa[k] = l4[(2 * pr + 2) * Q + k];
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int k = 0; k < Q; ++k) { acc = acc + qb[k].x; acc = acc + qb[k].y; acc = acc + qb[k].z; acc = acc + qb[k].w; }
          __builtin_amdgcn_sched_barrier(0);
        }
        if (lane < 2) sh->sum[lane] = acc;
      }
      __syncthreads();   // totals visible; the list may be rewritten by the next iteration
      pos_sum = sh->sum[0];
      neg_sum = sh->sum[1];
    }
    }  // dense body
    const OctavStep st = octav_step(guess, pos_sum, neg_sum, cp, cn, len, a.s, a.count_is_f64);
    if (tid == 0) a.hist[static_cast<long long>(it) * a.units + unit] = st.next;
    if (!st.close) moved |= 1ull << it;
    if (reached_fixed_point(guess, st.next)) {
      if (tid == 0) repeat_iterate(a, it, unit, st.next);
      break;
    }
    if constexpr (kCanHandOver) {
      if (a.tail != nullptr && !have_sums && it + 2 < a.max_iter && guess > 0.f && st.next >= guess && cp <= cand_cap && cn <= cand_cap) {
        // few elements selected and the guess growing: every later selection is a subset of this one.
        // List it (value, position; row order) for the tail. scan_p / scan_n are this iteration's
        // inclusive scans of the per-thread counts inside the wave, the exchange area has the waves' totals.
        const Shared* shc = reinterpret_cast<const Shared*>(smem + kX * ((nit - 1) & 1));
        int bp = scan_p - __builtin_popcount(wp[0]), bn = scan_n - __builtin_popcount(wn[0]);
        for (int k = 0; k < wave; ++k) { bp += shc->wave_count[0][k]; bn += shc->wave_count[1][k]; }
        // (each thread stores the few candidates of its own piece straight to global memory. Staging them
        // in LDS and copying whole lines out was measured: the partial-line stores here cost 4 x the row in
        // HBM traffic (profiles/r03_pmc_traffic.txt) but the kernel is bound by instruction issue, and the
        // two extra barriers + copy loops made it 10 % slower: 200 against 182 us at 4096 x 4096)
        float* vp = a.tail_values + (static_cast<long long>(unit) * 2) * cand_cap;
        float* vn = vp + cand_cap;
        unsigned short* pp = a.tail_pos + (static_cast<long long>(unit) * 2) * cand_cap;
        unsigned short* pn = pp + cand_cap;
        const int e0 = kPiece * tid;
#pragma unroll
        for (int i = 0; i < kPiece; ++i) {
          if ((wp[0] >> i) & 1u) { vp[bp] = x[0][i]; pp[bp] = static_cast<unsigned short>(e0 + i); ++bp; }
          if ((wn[0] >> i) & 1u) { vn[bn] = x[0][i]; pn[bn] = static_cast<unsigned short>(e0 + i); ++bn; }
        }
        if (tid == 0) {
          TailState ts;
          ts.next_it = it + 1; ts.n[0] = cp; ts.n[1] = cn; ts.guess = st.next; ts.cand_guess = guess;
          ts.moved_lo = static_cast<unsigned>(moved); ts.moved_hi = static_cast<unsigned>(moved >> 32); ts.pad = 0;
          a.tail[unit] = ts;
        }
        handed_over = true;
        break;
      }
    }
    guess = st.next;
  }
  if (tid == 0 && !handed_over) {
    publish_moving(a.moving, moved);
    if (a.tail != nullptr) a.tail[unit].next_it = 0;
  }
}

// ---- short units (blockwise recipes: 32 .. 512 elements): a workgroup takes kGroupLen contiguous
// elements = 8 .. 128 whole units through the same machinery ----------------------------------
// One wave per 128-element unit (octav_kernel) spends ~400 cycles per unit, mask and iteration on
// ballots, scalar bit scans and lane broadcasts with most lanes idle: 0.43 ms for 4096 x 4096 in
// blocks of 128. Here thread t owns piece t (16 elements in registers) of the group, a unit is
// ppu = unit_len / 16 consecutive pieces, and everything that is per row in octav_rows_kernel is
// per unit: the guess (LDS, one float per unit), where a run may continue (not past the unit's last
// piece), the slice of the run-sum list a chain walks, the selected-element counts (differences of
// the wave's inclusive scan at the unit's ends: units never straddle waves). Thread u < units runs
// unit u's two short chains and its Newton update; the group leaves the loop when every unit has
// reached a fixed point.
constexpr int kGroupThreads = kGroupLen / kPiece;

struct GroupsShared {          // per iteration parity, like RowsShared
  int wave_runs[2][4];         // [mask][wave]: runs starting in that wave's pieces
  int wave_changed[4];
};

__global__ __launch_bounds__(kGroupThreads, 2) void octav_groups_kernel(OctavArgs a, int ulen) {
  constexpr int kWaves = kGroupThreads / kWave;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int ppu = ulen / kPiece, qmask = ppu - 1, upg = kGroupLen / ulen;   // pieces per unit (a power of two), units per group
  const long long unit0 = static_cast<long long>(blockIdx.x) * upg;
  constexpr int npieces = kGroupThreads;
  float* dummy = smem + 128 + tid;
  float* row = smem + 128 + kGroupThreads;
  constexpr int row_floats = (kGroupLen + (kGroupLen >> 4) + 4) & ~3;
  float* list_pos = row + row_floats;
  constexpr int cap = ((kGroupLen / 2 + 2 + 63) & ~63) + 64;
  float* list_neg = list_pos + cap;
  unsigned short* words_pos = reinterpret_cast<unsigned short*>(list_neg + cap);
  unsigned short* words_neg = words_pos + npieces;
  int* run_pre = reinterpret_cast<int*>(words_neg + npieces);   // [2][threads]: index of the thread's first run in the list
  int* cnt_incl = run_pre + 2 * kGroupThreads;                   // [2][threads]: selected elements up to and including the thread's piece (per wave)
  float* ug = reinterpret_cast<float*>(cnt_incl + 2 * kGroupThreads);   // [upg]: the units' current guesses
  int* totals = reinterpret_cast<int*>(ug + kGroupThreads);      // [2]: runs in the whole group

  for (int i = tid; i < 128; i += kGroupThreads) smem[i] = 0.f;
  if (tid < upg) ug[tid] = 1.0f;
  const float qnan = __builtin_nanf("");
  float x[kPiece];
  {
    const float4* g4 = reinterpret_cast<const float4*>(a.x + unit0 * ulen + kPiece * tid);   // (16-byte aligned: see the dispatch)
    const float4 v0 = g4[0], v1 = g4[1], v2 = g4[2], v3 = g4[3];
    x[0] = v0.x; x[1] = v0.y; x[2] = v0.z; x[3] = v0.w;
    x[4] = v1.x; x[5] = v1.y; x[6] = v1.z; x[7] = v1.w;
    x[8] = v2.x; x[9] = v2.y; x[10] = v2.z; x[11] = v2.w;
    x[12] = v3.x; x[13] = v3.y; x[14] = v3.z; x[15] = v3.w;
    const int p = pidx(kPiece * tid);
#pragma unroll
    for (int i = 0; i < kPiece; ++i) row[p + i] = x[i];
  }
  __syncthreads();
  const float before = (tid & qmask) != 0 ? row[pidx(kPiece * tid - 1)] : qnan;   // the element in front of the piece, same unit
  const int my_unit = tid / ppu;

  unsigned wp = 0u, wn = 0u;
  // thread u < upg carries unit u's state
  float pos_sum = 0.f, neg_sum = 0.f;
  int cp = 0, cn = 0;
  unsigned long long moved = 0;
  bool done = tid >= upg;
  for (int it = 0; it < a.max_iter; ++it) {
    const float hi = ug[my_unit], lo = -hi;
    GroupsShared* sh = reinterpret_cast<GroupsShared*>(smem + 64 * (it & 1));
    unsigned np_ = 0, nn_ = 0;
#pragma unroll
    for (int i = 0; i < kPiece; ++i) {
      np_ |= x[i] >= hi ? 1u << i : 0u;
      nn_ |= x[i] <= lo ? 1u << i : 0u;
    }
    const unsigned changed = (np_ ^ wp) | (nn_ ^ wn);
    wp = np_; wn = nn_;
    words_pos[tid] = static_cast<unsigned short>(np_);
    words_neg[tid] = static_cast<unsigned short>(nn_);
    const unsigned cpos = before >= hi ? 1u : 0u, cneg = before <= lo ? 1u : 0u;
    const unsigned sp = np_ & ~((np_ << 1) | cpos) & 0xFFFFu, sn = nn_ & ~((nn_ << 1) | cneg) & 0xFFFFu;   // run starts
    const int ip = wave_incl_scan(__builtin_popcount(sp)), in = wave_incl_scan(__builtin_popcount(sn));
    int pre_p = ip - __builtin_popcount(sp), pre_n = in - __builtin_popcount(sn);
    cnt_incl[tid] = wave_incl_scan(__builtin_popcount(np_));
    cnt_incl[kGroupThreads + tid] = wave_incl_scan(__builtin_popcount(nn_));
    const bool wave_changed = __ballot(changed != 0) != 0;
    if (lane == kWave - 1) {
      sh->wave_runs[0][wave] = ip; sh->wave_runs[1][wave] = in;
      sh->wave_changed[wave] = wave_changed ? 1 : 0;
    }
    __syncthreads();
    const bool any_changed = (sh->wave_changed[0] | sh->wave_changed[1] | sh->wave_changed[2] | sh->wave_changed[3]) != 0;
    if (any_changed || it == 0) {
      int npos = 0, nneg = 0;
#pragma unroll
      for (int k = 0; k < kWaves; ++k) {
        const int c0 = sh->wave_runs[0][k], c1 = sh->wave_runs[1][k];
        if (k < wave) { pre_p += c0; pre_n += c1; }
        npos += c0; nneg += c1;
      }
      run_pre[tid] = pre_p;
      run_pre[kGroupThreads + tid] = pre_n;
      if (tid == 0) { totals[0] = npos; totals[1] = nneg; }
      int long_e0[2] = {0, 0}, long_n[2] = {0, 0}, long_j[2] = {0, 0};
      const bool sparse_p = __ballot(__builtin_popcount(sp) > 3) == 0;
      const bool sparse_n = __ballot(__builtin_popcount(sn) > 3) == 0;
      if (sparse_p)
        piece_runs_sparse(wp, cpos, tid, npieces, words_pos, row, list_pos, pre_p, &long_e0[0], &long_n[0], &long_j[0], qmask);
      else
        piece_runs(x, wp, cpos, tid, npieces, words_pos, row, list_pos, dummy, pre_p, &long_e0[0], &long_n[0], &long_j[0], qmask);
      if (sparse_n)
        piece_runs_sparse(wn, cneg, tid, npieces, words_neg, row, list_neg, pre_n, &long_e0[1], &long_n[1], &long_j[1], qmask);
      else
        piece_runs(x, wn, cneg, tid, npieces, words_neg, row, list_neg, dummy, pre_n, &long_e0[1], &long_n[1], &long_j[1], qmask);
      // units of more than 128 elements only: runs longer than 128, one at a time by the wave that found them
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        unsigned long long pending = __ballot(long_n[k] > 0);
        while (pending != 0) {
          const int src = __builtin_ctzll(pending);
          pending &= pending - 1ull;
          const int e0 = __builtin_amdgcn_readlane(long_e0[k], src);
          const int n = __builtin_amdgcn_readlane(long_n[k], src);
          const int j = __builtin_amdgcn_readlane(long_j[k], src);
          const float res = pairwise_wave<8>(row, e0, n, lane);
          if (lane == 0) (k ? list_neg : list_pos)[j] = res;
        }
      }
      __syncthreads();
      if (!done) {
        // ---- unit tid: acc = acc + R_j over its slice of each list, its counts
        const int first = tid * ppu, last = first + ppu - 1;
        const bool at_wave_start = (first & (kWave - 1)) == 0;
        {
          const int j0 = run_pre[first], j1 = tid + 1 < upg ? run_pre[first + ppu] : totals[0];
          float acc = 0.f;
          for (int j = j0; j < j1; ++j) acc = acc + list_pos[j];
          pos_sum = acc;
          cp = cnt_incl[last] - (at_wave_start ? 0 : cnt_incl[first - 1]);
        }
        {
          const int j0 = run_pre[kGroupThreads + first], j1 = tid + 1 < upg ? run_pre[kGroupThreads + first + ppu] : totals[1];
          float acc = 0.f;
          for (int j = j0; j < j1; ++j) acc = acc + list_neg[j];
          neg_sum = acc;
          cn = cnt_incl[kGroupThreads + last] - (at_wave_start ? 0 : cnt_incl[kGroupThreads + first - 1]);
        }
      }
    }
    if (!done) {
      const float guess = ug[tid];
      const OctavStep st = octav_step(guess, pos_sum, neg_sum, cp, cn, ulen, a.s, a.count_is_f64);
      a.hist[static_cast<long long>(it) * a.units + unit0 + tid] = st.next;
      if (!st.close) moved |= 1ull << it;
      if (reached_fixed_point(guess, st.next)) {
        repeat_iterate(a, it, unit0 + tid, st.next);
        done = true;
      }
      ug[tid] = st.next;
    }
    if (__syncthreads_and(done ? 1 : 0)) break;   // (also: guesses visible, lists free for the next iteration)
  }
  if (tid < upg) publish_moving(a.moving, moved);
}

size_t octav_groups_smem() {
  const size_t row_floats = static_cast<size_t>((kGroupLen + (kGroupLen >> 4) + 4) & ~3);
  const size_t cap = static_cast<size_t>(((kGroupLen / 2 + 2 + 63) & ~63) + 64);
  return 512 + kGroupThreads * sizeof(float) + row_floats * sizeof(float) + cap * 2 * sizeof(float) +
         2 * kGroupThreads * sizeof(unsigned short) + 4 * kGroupThreads * sizeof(int) + kGroupThreads * sizeof(float) + 16;
}

int octav_rows_threads(int len) {
  const int npieces = (len + kPiece - 1) / kPiece;
  if (npieces > 256 && !getenv("MI355Q_OCTAV_NARROW_ROWS")) return npieces <= 512 ? 512 : 1024;
  return npieces <= 64 ? 64 : (npieces <= 128 ? 128 : 256);
}

size_t octav_rows_smem(int len) {
  const int kRowsThreads = octav_rows_threads(len);
  const int npieces = (len + kPiece - 1) / kPiece;
  const size_t row_floats = static_cast<size_t>((len + (len >> 4) + 4) & ~3);
  const size_t cap = static_cast<size_t>(((len / 2 + 2 + 63) & ~63) + 64);
  return 2 * rows_xchg_floats(kRowsThreads) * sizeof(float) + kRowsThreads * sizeof(float) + row_floats * sizeof(float) + cap * 2 * sizeof(float) +
         static_cast<size_t>((npieces + 1) & ~1) * 2 * sizeof(unsigned short);
}

}  // namespace

// candidates per mask a row may hand to its tail (an eighth of the row, a multiple of 64)
int octav_tail_cap(int len) {
  static const int div = [] { const char* e = getenv("MI355Q_OCTAV_TAIL_DIV"); const int v = e ? atoi(e) : 0; return v >= 2 && v <= 256 ? v : 8; }();
  const int c = ((len / div) + 63) & ~63;
  return c < 64 ? 64 : c;
}

int32_t launch_octav_rows(OctavArgs a, void* workspace, size_t workspace_bytes, hipStream_t st) {
  // late iterations on a one-wave tail kernel (octav_tail_kernel) when the caller's workspace has room for
  // the hand-over (mi355q_octav_rows_workspace_bytes); MI355Q_OCTAV_TAIL=0 keeps every iteration in the rows kernel
  static const bool tail_on = [] { const char* e = getenv("MI355Q_OCTAV_TAIL"); return e == nullptr || atoi(e) != 0; }();
  const int threads = octav_rows_threads(a.len);
  const int slots = ((a.len + kPiece - 1) / kPiece + threads - 1) / threads;   // 1 .. 4 (> 1 only with 256 threads: MI355Q_OCTAV_NARROW_ROWS)
  a.tail_cap = octav_tail_cap(a.len);
  if (tail_on && slots == 1 && workspace_bytes >= mi355q_octav_rows_workspace_bytes(a.units, a.len, a.max_iter)) {
    const size_t need = mi355q_octav_workspace_bytes(a.units, a.max_iter);
    unsigned char* tb = reinterpret_cast<unsigned char*>(workspace) + ((need + 63) & ~static_cast<size_t>(63));
    a.tail = reinterpret_cast<TailState*>(tb);
    a.tail_values = reinterpret_cast<float*>(tb + static_cast<size_t>(a.units) * sizeof(TailState));
    a.tail_pos = reinterpret_cast<unsigned short*>(a.tail_values + static_cast<size_t>(a.units) * 2 * a.tail_cap);
  }
  const size_t smem = octav_rows_smem(a.len);
  const void* fn = threads == 1024 ? reinterpret_cast<const void*>(octav_rows_kernel<1, 1024>)
                 : threads == 512 ? reinterpret_cast<const void*>(octav_rows_kernel<1, 512>)
                 : slots == 4 ? reinterpret_cast<const void*>(octav_rows_kernel<4, 256>)
                 : slots == 3 ? reinterpret_cast<const void*>(octav_rows_kernel<3, 256>)
                 : slots == 2 ? reinterpret_cast<const void*>(octav_rows_kernel<2, 256>)
                 : threads == 256 ? reinterpret_cast<const void*>(octav_rows_kernel<1, 256>)
                 : threads == 128 ? reinterpret_cast<const void*>(octav_rows_kernel<1, 128>)
                                  : reinterpret_cast<const void*>(octav_rows_kernel<1, 64>);
  if (smem > 64 * 1024) {   // > 64 KB of dynamic LDS has to be asked for (per device: set on every call)
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return fail(MI355Q_HIP_ERROR, "hipFuncSetAttribute: %s", hipGetErrorString(e));
  }
  if (a.units > 0x7FFFFFFFLL) return fail(MI355Q_UNSUPPORTED, "too many units");
  void* kargs[] = {&a};
  if (hipLaunchKernel(fn, dim3(static_cast<unsigned>(a.units)), dim3(threads), kargs, smem, st) != hipSuccess)
    return fail(MI355Q_HIP_ERROR, "octav rows launch failed");
  MI355Q_CHECK_LAUNCH("octav rows launch");
  return a.tail != nullptr ? launch_octav_tail(a, st) : MI355Q_OK;
}

int32_t launch_octav_groups(const OctavArgs& a, hipStream_t st) {
  const size_t smem = octav_groups_smem();
  hipLaunchKernelGGL(octav_groups_kernel, dim3(static_cast<unsigned>(a.units * a.len / kGroupLen)), dim3(kGroupThreads), smem,
                     st, a, a.len);
  MI355Q_CHECK_LAUNCH("octav groups launch");
  return MI355Q_OK;
}

}  // namespace mi355q
