// Activation histograms (DynamicHistogram): the two per-element passes of
//   ref: utils/histogram_utils.py:139-164 (_DynamicHistogram1D.add) and :396-416 (the isfinite filter of DynamicHistogram.add)
// over a table of float32 tensors, each seen as [outer, channels, inner] (channels = 1: per tensor).
//
//   hist_stats_kernel   finite min, finite max and the number of finite elements of every (entry, channel);
//   hist_bins_kernel    idx = clip(int32(floor((x - lower_bound) / bin_width)), 0, n - 1) of every finite element, counted
//                       into the (entry, channel)'s own row of int64.
//
// Everything between the two (initialisation, padding, doubling of the bin width) is scalar work on the host
// (mi355q/utils/histogram_utils.py); it reads the statistics and never a count.
//
// The results are integers and exact extrema, so atomics do not make them depend on arrival order: the statistics are
// combined with integer max on an order-preserving key of the float, the counts with integer adds.
//
// Traversal. An entry is walked in one of two ways, chosen per entry:
//   rows     channels == 1 or inner >= kColsInner: contiguous runs of `inner` elements (the whole tensor when channels
//            is 1) cut into chunks; a wave (statistics) or a workgroup (bins) owns a chunk, reads it with 16-byte loads
//            behind a scalar head up to the first aligned address and a scalar tail, and keeps accumulating while
//            consecutive chunks belong to the same (entry, channel);
//   columns  channels > 1 and inner < kColsInner (channels on the last axis, or a short inner run): the tensor is a
//            matrix of outer rows of channels * inner floats, a lane owns four adjacent columns (one when the row
//            length or the pointer rules 16-byte loads out) over a band of rows, so its channels are fixed. The
//            statistics of a column's lanes meet in LDS, where the columns also change hands so that one atomic
//            instruction covers 64 neighbouring slots.
//
// Counting, by the largest n of the launch:
//   n <= 8         registers (compare and add per bin), reduced across the wave in rows mode; no LDS;
//   n <= 16384     uint32 bins in LDS (ds_add_u32), in rows mode as many replicas (a power of two, at most 32) as fit
//                  the 64 KiB, chosen by lane, because activations pile up in a few centre bins; in columns mode one
//                  copy per channel of the workgroup's columns (a wave's lanes fall on different channels), global
//                  adds where those do not fit; non-zero bins are flushed with one 64-bit global atomic add each;
//   above          rows mode: one window of 16384 bins per workgroup and pass over the run (a tensor is read once per
//                  window); columns mode: one global atomic add per element.
#include "common.h"

namespace mi355q {
namespace {

constexpr int kStatThreads = 256;
constexpr int kStatChunk = 8192;     // elements a wave takes per step in rows mode
constexpr int kBinThreads = 1024;    // 16 waves share one set of LDS bins; two workgroups fill a CU
constexpr int kRegThreads = 256;     // the register routes share nothing: smaller workgroups, 256 VGPRs to count in
constexpr int kBinChunk = 65536;     // elements a workgroup takes per step in rows mode
constexpr int kLdsWords = 16384;     // 64 KiB of uint32 bins
constexpr int kMaxReplicas = 32;
constexpr int kColsInner = 64;       // inner runs shorter than this are walked by columns
constexpr int kColRows = 64;         // fewest rows per step in columns mode. Fewer workgroups per tensor with longer walks
                                     // per lane measured slower (256 rows: 2.7 x on [256, 4096]; 2048 rows: 2.5 x on the
                                     // bins of [8192, 128]), and so did a zero / flush of the LDS bins every 64 rows (3.2 x)

typedef float v4f __attribute__((ext_vector_type(4)));

struct Entry {
  const float* x;
  int64_t outer, channels, inner, slot0;
  bool cols;
};

__device__ __forceinline__ Entry load_entry(const float* const* xs, const int64_t* outer, const int64_t* channels,
                                            const int64_t* inner, const int64_t* slot0, int e) {
  Entry t{xs[e], outer[e], channels[e], inner[e], slot0[e], false};
  t.cols = t.channels > 1 && t.inner < kColsInner;
  return t;
}

__device__ __forceinline__ bool is_finite(float v) { return (f2u(v) & 0x7F800000u) != 0x7F800000u; }

// Unsigned key with the order of the floats (-0 below +0). No finite float has key 0 or ~key 0, so a zeroed word
// means "nothing seen" for both the maximum (max of key) and the minimum (max of ~key).
__device__ __forceinline__ uint32_t order_key(float v) {
  const uint32_t b = f2u(v);
  return (b >> 31) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k) { return u2f((k >> 31) ? (k ^ 0x80000000u) : ~k); }

// f(value) for every element of the contiguous run [p, p + n), shared by NT lanes.
template <int NT, class F>
__device__ __forceinline__ void for_span(const float* __restrict__ p, int64_t n, int lane, F&& f) {
  int64_t head = static_cast<int64_t>((0 - (reinterpret_cast<uintptr_t>(p) >> 2)) & 3);
  if (head > n) head = n;
  if (lane < head) f(p[lane]);
  const v4f* p4 = reinterpret_cast<const v4f*>(p + head);
  const int64_t n4 = (n - head) >> 2;
  int64_t i = lane;
  for (; i + 3 * NT < n4; i += 4 * NT) {   // four 16-byte loads in flight per lane; read once: non-temporal
    v4f v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = __builtin_nontemporal_load(&p4[i + u * NT]);
#pragma unroll
    for (int u = 0; u < 4; ++u) { f(v[u].x); f(v[u].y); f(v[u].z); f(v[u].w); }
  }
  for (; i < n4; i += NT) {
    const v4f v = __builtin_nontemporal_load(&p4[i]);
    f(v.x); f(v.y); f(v.z); f(v.w);
  }
  const int64_t t = head + n4 * 4 + lane;
  if (t < n) f(p[t]);
}

// The lane layout of columns mode: `tpr` lanes (a power of two) side by side on a row, the rest on further rows.
struct ColMap {
  int vec;            // 4: a lane owns four adjacent columns read with one 16-byte load; 1: one column
  int64_t width;      // floats per row
  int64_t units;      // column units (of vec columns) per row
  int tpr, rows_per_step, tx, ty;
  int64_t groups, band_rows, bands, items;
};

template <int NT>
__device__ __forceinline__ ColMap col_map(const Entry& t, int tid, int64_t blocks) {
  ColMap m;
  m.width = t.channels * t.inner;
  m.vec = ((m.width & 3) == 0 && (reinterpret_cast<uintptr_t>(t.x) & 15) == 0) ? 4 : 1;
  m.units = m.width / m.vec;
  int tpr = 1;
  while (tpr < NT && tpr < m.units) tpr <<= 1;
  m.tpr = tpr;
  m.rows_per_step = NT / tpr;
  m.tx = tid & (tpr - 1);
  m.ty = tid / tpr;
  m.groups = (m.units + tpr - 1) / tpr;
  // the rows are shared out among the workgroups a column group can have, in bands of at least kColRows
  const int64_t per_group = blocks / m.groups > 0 ? blocks / m.groups : 1;
  m.band_rows = (t.outer + per_group - 1) / per_group;
  if (m.band_rows < kColRows) m.band_rows = kColRows;
  m.bands = (t.outer + m.band_rows - 1) / m.band_rows;
  m.items = m.groups * m.bands;
  return m;
}

// ---------------------------------------------------------------------------------------- statistics ---
// The workspace: 16 zeroed bytes per slot, one array per quantity so that a wave's atomics on neighbouring slots
// are one contiguous piece each (64 lanes in 64 different 64-byte segments run an order of magnitude slower).
constexpr size_t kStatSlotBytes = 16;
struct StatTable {
  unsigned long long* count;
  uint32_t* max_key;
  uint32_t* min_key_inv;
  __device__ __host__ StatTable(void* ws, int64_t slots)
      : count(static_cast<unsigned long long*>(ws)), max_key(reinterpret_cast<uint32_t*>(count + slots)),
        min_key_inv(max_key + slots) {}
};

struct StatAcc {
  float mn, mx;
  unsigned long long cnt;
  __device__ __forceinline__ void reset() {
    mn = __builtin_huge_valf();
    mx = -__builtin_huge_valf();
    cnt = 0;
  }
  __device__ __forceinline__ void add(float v) {
    const bool f = is_finite(v);   // a test, not a clamp: NaN and +-inf take no part
    mn = fminf(mn, f ? v : __builtin_huge_valf());
    mx = fmaxf(mx, f ? v : -__builtin_huge_valf());
    cnt += f ? 1u : 0u;
  }
  __device__ __forceinline__ void emit(const StatTable& ws, int64_t slot, int64_t slots) const {
    if (cnt == 0 || slot < 0 || slot >= slots) return;
    atomicMax(&ws.max_key[slot], order_key(mx));
    atomicMax(&ws.min_key_inv[slot], ~order_key(mn));
    atomicAdd(&ws.count[slot], cnt);
  }
};

// grid (blocks, count). ws_raw: kStatSlotBytes zeroed bytes per (entry, channel).
__global__ __launch_bounds__(kStatThreads) void hist_stats_kernel(
    const float* const* __restrict__ xs, const int64_t* __restrict__ outer, const int64_t* __restrict__ channels,
    const int64_t* __restrict__ inner, const int64_t* __restrict__ slot0, void* __restrict__ ws_raw, int64_t slots) {
  const StatTable ws(ws_raw, slots);
  const Entry t = load_entry(xs, outer, channels, inner, slot0, blockIdx.y);
  if (t.outer <= 0 || t.channels <= 0 || t.inner <= 0) return;
  const int tid = threadIdx.x;
  if (!t.cols) {
    const int64_t len = t.channels == 1 ? t.outer * t.inner : t.inner;
    const int64_t rows = t.channels == 1 ? 1 : t.outer * t.channels;
    const int64_t per_row = (len + kStatChunk - 1) / kStatChunk;
    const int64_t items = rows * per_row;
    const int lane = tid & (kWave - 1);
    const int64_t nwaves = static_cast<int64_t>(gridDim.x) * (kStatThreads / kWave);
    StatAcc a;
    a.reset();
    int64_t cur = -1;
    auto flush = [&]() {
#pragma unroll
      for (int off = kWave / 2; off > 0; off >>= 1) {
        a.mn = fminf(a.mn, __shfl_xor(a.mn, off, kWave));
        a.mx = fmaxf(a.mx, __shfl_xor(a.mx, off, kWave));
        a.cnt += __shfl_xor(a.cnt, off, kWave);
      }
      if (lane == 0) a.emit(ws, cur, slots);
      a.reset();
    };
    for (int64_t item = static_cast<int64_t>(blockIdx.x) * (kStatThreads / kWave) + tid / kWave; item < items;
         item += nwaves) {
      const int64_t row = item / per_row, chunk = item - row * per_row;
      const int64_t slot = t.slot0 + row % t.channels;
      if (slot != cur) {   // (wave-uniform)
        if (cur >= 0) flush();
        cur = slot;
      }
      const int64_t start = chunk * kStatChunk;
      const int64_t n = len - start < kStatChunk ? len - start : kStatChunk;
      for_span<kWave>(t.x + row * len + start, n, lane, [&](float v) { a.add(v); });
    }
    if (cur >= 0) flush();
    return;
  }
  __shared__ float sh_mn[4][kStatThreads], sh_mx[4][kStatThreads];
  __shared__ unsigned long long sh_cnt[4][kStatThreads];
  const ColMap m = col_map<kStatThreads>(t, tid, gridDim.x);
  for (int64_t item = blockIdx.x; item < m.items; item += gridDim.x) {
    const int64_t group = item / m.bands, band = item - group * m.bands;
    const int64_t unit = group * m.tpr + m.tx;
    const bool active = unit < m.units;
    const int64_t r0 = band * m.band_rows, r1 = active ? (r0 + m.band_rows < t.outer ? r0 + m.band_rows : t.outer) : r0;
    StatAcc a[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k].reset();
    const float* __restrict__ base = t.x + unit * m.vec;
    if (m.vec == 4) {
      int64_t r = r0 + m.ty;
      for (; r + 3 * m.rows_per_step < r1; r += 4 * m.rows_per_step) {
        v4f v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
          v[u] = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(base + (r + u * m.rows_per_step) * m.width));
#pragma unroll
        for (int u = 0; u < 4; ++u) { a[0].add(v[u].x); a[1].add(v[u].y); a[2].add(v[u].z); a[3].add(v[u].w); }
      }
      for (; r < r1; r += m.rows_per_step) {
        const v4f v = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(base + r * m.width));
        a[0].add(v.x); a[1].add(v.y); a[2].add(v.z); a[3].add(v.w);
      }
    } else {
      for (int64_t r = r0 + m.ty; r < r1; r += m.rows_per_step) a[0].add(base[r * m.width]);
    }
    // The lanes that share a column meet in LDS, and the columns change hands there: lane i of the workgroup then
    // holds column i, i + 256, ... of the group, so that every atomic instruction covers 64 neighbouring slots.
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      sh_mn[k][tid] = a[k].mn;
      sh_mx[k][tid] = a[k].mx;
      sh_cnt[k][tid] = a[k].cnt;
    }
    __syncthreads();
    const int cols_here = m.tpr * m.vec;
    const int64_t first_col = group * cols_here;
    for (int c = tid; c < cols_here && first_col + c < m.width; c += kStatThreads) {
      const int k = c & (m.vec - 1), x = c / m.vec;   // (vec is 1 or 4)
      StatAcc b{sh_mn[k][x], sh_mx[k][x], sh_cnt[k][x]};
      for (int y = 1; y < m.rows_per_step; ++y) {
        b.mn = fminf(b.mn, sh_mn[k][y * m.tpr + x]);
        b.mx = fmaxf(b.mx, sh_mx[k][y * m.tpr + x]);
        b.cnt += sh_cnt[k][y * m.tpr + x];
      }
      b.emit(ws, t.slot0 + (first_col + c) / t.inner, slots);
    }
  }
}

__global__ __launch_bounds__(256) void hist_stats_finalize_kernel(void* __restrict__ ws_raw, int64_t slots,
                                                                  float* __restrict__ mn, float* __restrict__ mx,
                                                                  int64_t* __restrict__ cnt) {
  const int64_t s = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (s >= slots) return;
  const StatTable ws(ws_raw, slots);
  const unsigned long long n = ws.count[s];
  mn[s] = n ? key_value(~ws.min_key_inv[s]) : __builtin_huge_valf();
  mx[s] = n ? key_value(ws.max_key[s]) : -__builtin_huge_valf();
  cnt[s] = static_cast<int64_t>(n);
}

// ---------------------------------------------------------------------------------------------- bins ---
struct BinSlot {
  double lb, bw;
  long long off;
  int n, pad;
};

// The caller's four per-slot tables as one 32-byte record; a row that does not lie inside the output is switched off here.
__global__ __launch_bounds__(256) void hist_bins_pack_kernel(const double* __restrict__ lb, const double* __restrict__ bw,
                                                             const int64_t* __restrict__ n, const int64_t* __restrict__ off,
                                                             int64_t slots, int64_t n_max, int64_t out_len,
                                                             BinSlot* __restrict__ out) {
  const int64_t s = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (s >= slots) return;
  const int64_t ns = n[s], os = off[s];
  const bool ok = ns > 0 && ns <= n_max && os >= 0 && os <= out_len - ns;
  out[s] = BinSlot{lb[s], bw[s], static_cast<long long>(os), ok ? static_cast<int>(ns) : 0, 0};
}

// PREC 0: float32 subtraction and division (float32 state). 1: float32 subtraction, float64 division (float32 lower
// bound, float64 width). 2: both in float64. The quotient is the correctly rounded IEEE one: no reciprocal.
template <int PREC>
struct Binner {
  double lb, bw;
  float lbf, bwf;
  int last;
  __device__ __forceinline__ explicit Binner(const BinSlot& s)
      : lb(s.lb), bw(s.bw), lbf(static_cast<float>(s.lb)), bwf(static_cast<float>(s.bw)), last(s.n - 1) {}
  __device__ __forceinline__ int operator()(float x) const {
    if (PREC == 0) {
      const float f = floorf((x - lbf) / bwf);
      return f > 0.f ? (f < 16777216.f ? (static_cast<int>(f) < last ? static_cast<int>(f) : last) : last) : 0;
    }
    const double d = PREC == 1 ? static_cast<double>(x - lbf) : static_cast<double>(x) - lb;
    const double f = floor(d / bw);
    return f > 0.0 ? (f < 16777216.0 ? (static_cast<int>(f) < last ? static_cast<int>(f) : last) : last) : 0;
  }
};

__device__ __forceinline__ void add_row(int64_t* __restrict__ out, long long at, uint32_t v) {
  if (v) atomicAdd(reinterpret_cast<unsigned long long*>(out) + at, static_cast<unsigned long long>(v));
}

// ROUTE 0: n_max == 1 and 1: n_max <= 8, counted in NB registers; 2: LDS bins, or global adds where they do not fit.
template <int PREC, int ROUTE>
__global__ __launch_bounds__(ROUTE == 2 ? kBinThreads : kRegThreads) void hist_bins_kernel(
    const float* const* __restrict__ xs, const int64_t* __restrict__ outer, const int64_t* __restrict__ channels,
    const int64_t* __restrict__ inner, const int64_t* __restrict__ slot0, const BinSlot* __restrict__ bin_slots,
    int64_t slots, int n_max, int64_t* __restrict__ out) {
  constexpr int NB = ROUTE == 0 ? 1 : 8;
  constexpr int NT = ROUTE == 2 ? kBinThreads : kRegThreads;
  __shared__ uint32_t lds[ROUTE == 2 ? kLdsWords : 1];
  const Entry t = load_entry(xs, outer, channels, inner, slot0, blockIdx.y);
  if (t.outer <= 0 || t.channels <= 0 || t.inner <= 0) return;
  if (t.slot0 < 0 || t.slot0 > slots - t.channels) return;
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);

  if (!t.cols) {
    const int64_t len = t.channels == 1 ? t.outer * t.inner : t.inner;
    const int64_t rows = t.channels == 1 ? 1 : t.outer * t.channels;
    if (ROUTE == 2 && n_max > kLdsWords) {
      // Rows that do not fit LDS: a workgroup takes one window of kLdsWords bins and reads the whole run for it, so a
      // tensor is read once per window (from L2 / MALL after the first) and every bin still gets one global add per
      // workgroup. (One global add per element instead was measured at 63 times the min/max pass.)
      const int wins = (n_max + kLdsWords - 1) / kLdsWords;
      const int64_t items = rows * wins;
      for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t row = item / wins;
        const int w0 = static_cast<int>(item - row * wins) * kLdsWords;
        const BinSlot s = bin_slots[t.slot0 + row % t.channels];
        if (s.n <= w0) continue;   // (workgroup-uniform)
        const int wn = s.n - w0 < kLdsWords ? s.n - w0 : kLdsWords;
        for (int i = tid; i < wn; i += NT) lds[i] = 0;
        __syncthreads();
        const Binner<PREC> bin(s);
        for_span<NT>(t.x + row * len, len, tid, [&](float v) {
          if (is_finite(v)) {
            const unsigned d = static_cast<unsigned>(bin(v) - w0);
            if (d < static_cast<unsigned>(wn)) atomicAdd(&lds[d], 1u);
          }
        });
        __syncthreads();
        for (int b = tid; b < wn; b += NT) add_row(out, s.off + w0 + b, lds[b]);
        __syncthreads();
      }
      return;
    }
    const int64_t per_row = (len + kBinChunk - 1) / kBinChunk;
    const int64_t items = rows * per_row;
    int64_t cur = -1;
    BinSlot s{0.0, 1.0, 0, 0, 0};
    uint32_t c[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) c[k] = 0;
    int replicas = 1;
    bool in_lds = false;
    auto open = [&](int64_t slot) {   // (workgroup-uniform)
      cur = slot;
      s = bin_slots[slot];
      if (ROUTE == 2) {
        in_lds = s.n > 0 && s.n <= kLdsWords;
        if (in_lds) {
          replicas = 1;
          while (replicas < kMaxReplicas && 2 * replicas * s.n <= kLdsWords) replicas <<= 1;
          for (int i = tid; i < replicas * s.n; i += NT) lds[i] = 0;
          __syncthreads();
        }
      }
    };
    auto close = [&]() {
      if (cur < 0 || s.n <= 0) return;
      if (ROUTE == 2) {
        if (in_lds) {
          __syncthreads();
          for (int b = tid; b < s.n; b += NT) {
            uint32_t v = 0;
            for (int r = 0; r < replicas; ++r) v += lds[r * s.n + b];
            add_row(out, s.off + b, v);
          }
          __syncthreads();
        }
      } else {
#pragma unroll
        for (int k = 0; k < NB; ++k) {
          uint32_t v = c[k];
#pragma unroll
          for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
          if (lane == 0 && k < s.n) add_row(out, s.off + k, v);
          c[k] = 0;
        }
      }
    };
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
      const int64_t row = item / per_row, chunk = item - row * per_row;
      const int64_t slot = t.slot0 + row % t.channels;
      if (slot != cur) {
        close();
        open(slot);
      }
      if (s.n <= 0) continue;   // no finite data in this (entry, channel)
      const Binner<PREC> bin(s);
      const int64_t start = chunk * kBinChunk;
      const int64_t n = len - start < kBinChunk ? len - start : kBinChunk;
      const float* p = t.x + row * len + start;
      if (ROUTE == 2) {
        if (in_lds) {
          uint32_t* mine = lds + (lane & (replicas - 1)) * s.n;
          for_span<NT>(p, n, tid, [&](float v) {
            if (is_finite(v)) atomicAdd(&mine[bin(v)], 1u);
          });
        } else {
          for_span<NT>(p, n, tid, [&](float v) {
            if (is_finite(v)) add_row(out, s.off + bin(v), 1u);
          });
        }
      } else {
        for_span<NT>(p, n, tid, [&](float v) {
          const bool f = is_finite(v);
          const int idx = bin(v);
#pragma unroll
          for (int k = 0; k < NB; ++k) c[k] += (f && idx == k) ? 1u : 0u;
        });
      }
    }
    close();
    return;
  }

  const ColMap m = col_map<NT>(t, tid, gridDim.x);
  for (int64_t item = blockIdx.x; item < m.items; item += gridDim.x) {
    const int64_t group = item / m.bands, band = item - group * m.bands;
    const int64_t unit = group * m.tpr + m.tx;
    const bool active = unit < m.units;
    const int64_t r0 = band * m.band_rows, r1 = r0 + m.band_rows < t.outer ? r0 + m.band_rows : t.outer;
    // the channels this workgroup's columns belong to: [c_lo, c_hi]
    const int64_t first_col = group * m.tpr * m.vec;
    int64_t last_col = first_col + static_cast<int64_t>(m.tpr) * m.vec - 1;
    if (last_col >= m.width) last_col = m.width - 1;
    const int64_t c_lo = first_col / t.inner, c_hi = last_col / t.inner;
    // a channel's bins start an odd number of words apart: with an even stride (16 bins) the lanes of a row, four
    // channels apart, would all fall into the same quarter of the 64 LDS banks
    const int stride = n_max | 1;
    const int64_t words = (c_hi - c_lo + 1) * stride;
    const bool in_lds = ROUTE == 2 && words <= kLdsWords;
    if (ROUTE == 2 && in_lds) {
      for (int i = tid; i < words; i += NT) lds[i] = 0;
      __syncthreads();
    }
    if (active) {
      BinSlot s[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int64_t ch = (unit * m.vec + (k < m.vec ? k : 0)) / t.inner;
        s[k] = bin_slots[t.slot0 + ch];
        if (k >= m.vec) s[k].n = 0;
      }
      const Binner<PREC> b0(s[0]), b1(s[1]), b2(s[2]), b3(s[3]);
      uint32_t c[4][NB];
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < NB; ++j) c[k][j] = 0;
      int lds_row[4];   // where each column's channel starts in the workgroup's LDS bins
#pragma unroll
      for (int k = 0; k < 4; ++k)
        lds_row[k] = static_cast<int>(((unit * m.vec + (k < m.vec ? k : 0)) / t.inner - c_lo) * stride);
      auto count = [&](int k, const Binner<PREC>& b, float v) {   // k is a constant after unrolling
        if (ROUTE == 2) {
          if (s[k].n > 0 && is_finite(v)) {
            const int idx = b(v);
            if (in_lds) {
              atomicAdd(&lds[lds_row[k] + idx], 1u);
            } else {
              add_row(out, s[k].off + idx, 1u);
            }
          }
        } else {
          const bool f = s[k].n > 0 && is_finite(v);
          const int idx = b(v);
#pragma unroll
          for (int j = 0; j < NB; ++j) c[k][j] += (f && idx == j) ? 1u : 0u;
        }
      };
      const float* __restrict__ base = t.x + unit * m.vec;
      if (m.vec == 4) {
        int64_t r = r0 + m.ty;
        for (; r + 3 * m.rows_per_step < r1; r += 4 * m.rows_per_step) {
          v4f v[4];
#pragma unroll
          for (int u = 0; u < 4; ++u)
            v[u] = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(base + (r + u * m.rows_per_step) * m.width));
#pragma unroll
          for (int u = 0; u < 4; ++u) { count(0, b0, v[u].x); count(1, b1, v[u].y); count(2, b2, v[u].z); count(3, b3, v[u].w); }
        }
        for (; r < r1; r += m.rows_per_step) {
          const v4f v = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(base + r * m.width));
          count(0, b0, v.x); count(1, b1, v.y); count(2, b2, v.z); count(3, b3, v.w);
        }
      } else {
        for (int64_t r = r0 + m.ty; r < r1; r += m.rows_per_step) count(0, b0, base[r * m.width]);
      }
      if (ROUTE != 2) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
          for (int j = 0; j < NB; ++j)
            if (j < s[k].n) add_row(out, s[k].off + j, c[k][j]);
      }
    }
    if (ROUTE == 2 && in_lds) {
      __syncthreads();
      for (int i = tid; i < words; i += NT) {
        const int64_t ch = i / stride;
        const int b = i - static_cast<int>(ch) * stride;
        const uint32_t v = lds[i];
        if (v) {
          const BinSlot s = bin_slots[t.slot0 + c_lo + ch];
          if (b < s.n) add_row(out, s.off + b, v);
        }
      }
      __syncthreads();
    }
  }
}

// Workgroups per entry: enough for the largest entry, fewer when the table itself fills the chip.
unsigned blocks_per_entry(int64_t max_numel, int64_t per_block, int32_t count, int64_t spread) {
  int64_t b = (max_numel + per_block - 1) / per_block;
  int64_t cap = spread / count;
  if (cap < 8) cap = 8;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return static_cast<unsigned>(b);
}

template <int PREC>
void launch_bins(int route, dim3 grid, hipStream_t st, const float* const* xs, const int64_t* outer,
                 const int64_t* channels, const int64_t* inner, const int64_t* slot0, const BinSlot* bs, int64_t slots,
                 int n_max, int64_t* out) {
  if (route == 0)
    hipLaunchKernelGGL((hist_bins_kernel<PREC, 0>), grid, dim3(kRegThreads), 0, st, xs, outer, channels, inner, slot0, bs,
                       slots, n_max, out);
  else if (route == 1)
    hipLaunchKernelGGL((hist_bins_kernel<PREC, 1>), grid, dim3(kRegThreads), 0, st, xs, outer, channels, inner, slot0, bs,
                       slots, n_max, out);
  else
    hipLaunchKernelGGL((hist_bins_kernel<PREC, 2>), grid, dim3(kBinThreads), 0, st, xs, outer, channels, inner, slot0, bs,
                       slots, n_max, out);
}

}  // namespace
}  // namespace mi355q

using namespace mi355q;

extern "C" size_t mi355q_hist_stats_workspace_bytes(int64_t slots) {
  return slots > 0 ? static_cast<size_t>(slots) * kStatSlotBytes : 0;
}

extern "C" int32_t mi355q_hist_stats_f32(const float* const* x_ptrs, const int64_t* outer, const int64_t* channels,
                                         const int64_t* inner, const int64_t* slot0, int32_t count, int64_t slots,
                                         int64_t max_numel, float* min_out, float* max_out, int64_t* count_out,
                                         void* workspace, size_t workspace_bytes, void* stream) {
  clear_error();
  if (count < 0 || count > 65535) return fail(MI355Q_BAD_ARG, "count must be in [0, 65535]");
  if (slots < 0 || max_numel < 0) return fail(MI355Q_BAD_ARG, "negative size");
  if (count == 0 || slots == 0) return MI355Q_OK;
  if (!x_ptrs || !outer || !channels || !inner || !slot0 || !min_out || !max_out || !count_out)
    return fail(MI355Q_BAD_ARG, "null pointer");
  const size_t need = mi355q_hist_stats_workspace_bytes(slots);
  if (!workspace || workspace_bytes < need) return fail(MI355Q_BAD_ARG, "workspace too small: need %zu bytes", need);
  hipStream_t st = as_stream(stream);
  if (hipMemsetAsync(workspace, 0, need, st) != hipSuccess) return fail(MI355Q_HIP_ERROR, "hist_stats: clearing the workspace");
  const unsigned blocks = blocks_per_entry(max_numel, static_cast<int64_t>(kStatChunk) * (kStatThreads / kWave), count, 65536);
  hipLaunchKernelGGL(hist_stats_kernel, dim3(blocks, static_cast<unsigned>(count)), dim3(kStatThreads), 0, st, x_ptrs,
                     outer, channels, inner, slot0, workspace, slots);
  MI355Q_CHECK_LAUNCH("hist_stats launch");
  hipLaunchKernelGGL(hist_stats_finalize_kernel, dim3(static_cast<unsigned>((slots + 255) / 256)), dim3(256), 0, st,
                     workspace, slots, min_out, max_out, count_out);
  MI355Q_CHECK_LAUNCH("hist_stats finalize launch");
  return MI355Q_OK;
}

extern "C" size_t mi355q_hist_bins_workspace_bytes(int64_t slots) {
  return slots > 0 ? static_cast<size_t>(slots) * sizeof(BinSlot) : 0;
}

extern "C" int32_t mi355q_hist_bins_f32(const float* const* x_ptrs, const int64_t* outer, const int64_t* channels,
                                        const int64_t* inner, const int64_t* slot0, int32_t count, int64_t slots,
                                        int64_t max_numel, const double* lower_bound, const double* bin_width,
                                        const int64_t* n_bins, const int64_t* row_offset, int64_t n_max,
                                        int32_t precision, int64_t* counts_out, int64_t out_len, void* workspace,
                                        size_t workspace_bytes, void* stream) {
  clear_error();
  if (count < 0 || count > 65535) return fail(MI355Q_BAD_ARG, "count must be in [0, 65535]");
  if (slots < 0 || max_numel < 0 || out_len < 0) return fail(MI355Q_BAD_ARG, "negative size");
  if (n_max < 0 || n_max > 0x7FFFFFFF) return fail(MI355Q_BAD_ARG, "n_max must be in [0, 2^31)");
  if (precision < 0 || precision > 2) return fail(MI355Q_BAD_ARG, "precision must be 0, 1 or 2");
  if (count == 0 || slots == 0 || n_max == 0) return MI355Q_OK;
  if (!x_ptrs || !outer || !channels || !inner || !slot0 || !lower_bound || !bin_width || !n_bins || !row_offset ||
      !counts_out)
    return fail(MI355Q_BAD_ARG, "null pointer");
  const size_t need = mi355q_hist_bins_workspace_bytes(slots);
  if (!workspace || workspace_bytes < need) return fail(MI355Q_BAD_ARG, "workspace too small: need %zu bytes", need);
  hipStream_t st = as_stream(stream);
  BinSlot* bs = static_cast<BinSlot*>(workspace);
  hipLaunchKernelGGL(hist_bins_pack_kernel, dim3(static_cast<unsigned>((slots + 255) / 256)), dim3(256), 0, st,
                     lower_bound, bin_width, n_bins, row_offset, slots, n_max, out_len, bs);
  MI355Q_CHECK_LAUNCH("hist_bins pack launch");
  const int route = n_max <= 1 ? 0 : n_max <= 8 ? 1 : 2;
  const dim3 grid(blocks_per_entry(max_numel, kBinChunk, count, 8192), static_cast<unsigned>(count));
  const int nm = static_cast<int>(n_max);
  if (precision == 0)
    launch_bins<0>(route, grid, st, x_ptrs, outer, channels, inner, slot0, bs, slots, nm, counts_out);
  else if (precision == 1)
    launch_bins<1>(route, grid, st, x_ptrs, outer, channels, inner, slot0, bs, slots, nm, counts_out);
  else
    launch_bins<2>(route, grid, st, x_ptrs, outer, channels, inner, slot0, bs, slots, nm, counts_out);
  MI355Q_CHECK_LAUNCH("hist_bins launch");
  return MI355Q_OK;
}
