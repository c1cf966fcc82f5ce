// Tensor comparison metrics for model validation: MSE, SNR, median diff ratio, cosine similarity and KL
// divergence of a float32 reference against a target read in its stored form.
//
//   ref: utils/validation_utils.py:63-255   (the five metrics, _preprocess_same_size_arrays)
//   ref: model_validator.py:357-361         (fn(target_data, reference_data))
//   ref: uniform_quantize_tensor.py:365-409 (how a quantized target becomes float)
//
// The target is dequantized in registers (no float32 copy of it in HBM). Both operands go through
// np.nan_to_num(nan=1e-9, neginf=-1e9, posinf=1e9) first.
//
// Order. np.square(x).mean() and np.sum(x) over a contiguous 1-D float32 array walk it in chunks of
// 8192 elements (the nditer buffer; tests/numpy_sum_model.py plain_sum, checked against NumPy at
// n = 1 .. 2^20 + 3 in tests/test_validation_host.py): every chunk is summed with NumPy's pairwise routine
// and the chunk sums are added left to right, acc = acc + pairwise(chunk). So
//   pass 1   one workgroup per chunk: the leaves (<= 128 elements, eight strided accumulators) in
//            parallel, then the pairwise tree over the leaves -- level by level when the chunk is
//            balanced (every full chunk: 8192 = 64 << 7), one lane per sum walking the tree otherwise;
//   combine  one wave per pair adds its chunk sums in order.
// Sum(t-r)^2, Sum r^2 and Sum p log((p+eps)/(q+eps)) are carried this way; the three dot products of the
// cosine (any order: NumPy takes them from BLAS sdot) are float32 products summed in float64.
//
// Median of |t - r| / (|r| + 1e-6) (float32, >= 0, so the bit pattern orders the values): a radix select
// over bits 30..20 (pass 1), 19..9 (pass 2) and 8..0 (pass 3), each pass followed by a select kernel that
// scans the pair's histogram. For even n the upper middle value is the next value of the same last-level
// bin set, or the smallest ratio above the whole final prefix (tracked in pass 3).
#include <cstdlib>

#include "common.h"
#include "compare_target.h"

namespace mi355q {
namespace {

constexpr int kChunk = 8192;          // NumPy nditer buffer size (elements)
constexpr int kThreads = 256;
constexpr int kMaxLeaves = 256;       // a chunk of <= 8192 elements has <= 65 pairwise leaves (tests/compare_route_cases.py)
constexpr int kBins1 = 2048;          // ratio bits 30..20
constexpr int kBins2 = 2048;          // ratio bits 19..9
constexpr int kBins3 = 512;           // ratio bits 8..0
constexpr int kHistBins = 2048;
constexpr int kCombineTile = 2048;    // chunk sums staged in LDS per step of the combine kernel

struct ChunkPartial {
  float sq, r2, kl, pad;
  double tr, tt, rr;
  double pad2;
};
static_assert(sizeof(ChunkPartial) == 48, "ChunkPartial layout");

struct SelectState {
  uint32_t prefix;      // ratio bits fixed so far (right-aligned)
  uint32_t min_above;   // smallest ratio pattern above the final prefix's span (pass 3)
  int64_t k;            // rank of the lower middle value among the elements that share `prefix`
};

struct Batch {
  const mi355q_compare_pair* table;   // device table, or nullptr: `one` is the only pair
  mi355q_compare_pair one;
  int32_t count;
  int32_t want_median;
  int32_t want_kl;                    // Sum p log((p+e)/(q+e)) is computed (logf per element)
  int64_t total_chunks;               // what the grids were sized for
  const int64_t* chunk0;              // [count + 1] first chunk of every pair (batched form)
  ChunkPartial* partials;             // [total chunks]
  unsigned long long* hist;           // [count][kHistBins]
  SelectState* state;                 // [count]
  mi355q_compare_result* results;     // [count]
};

__device__ __forceinline__ const mi355q_compare_pair& pair_of(const Batch& b, int32_t i) {
  return b.table ? b.table[i] : b.one;
}

// chunk -> pair (binary search over the chunk prefix table)
__device__ __forceinline__ int32_t pair_of_chunk(const Batch& b, int64_t chunk) {
  if (!b.table) return 0;
  int32_t lo = 0, hi = b.count - 1;
  while (lo < hi) {
    const int32_t mid = (lo + hi + 1) >> 1;
    if (b.chunk0[mid] <= chunk) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ int64_t first_chunk(const Batch& b, int32_t p) { return b.table ? b.chunk0[p] : 0; }

// A device table that failed compare_chunk_table_kernel's checks (an invalid entry, or element counts that do not
// add up to the chunks the grids were sized for) is marked with chunk0[count] = -1: no kernel then reads an
// operand or the partial sums, and every result is NaN.
__device__ __forceinline__ bool table_ok(const Batch& b) { return !b.table || b.chunk0[b.count] >= 0; }

__device__ __forceinline__ float nan_to_num(float v) {
  if (v != v) return 1e-9f;
  if (v == __builtin_inff()) return 1e9f;
  if (v == -__builtin_inff()) return -1e9f;
  return v;
}

struct Elem {
  float sq, r2, kl;
  float tr, tt, rr;
  uint32_t ratio;
};

__device__ __forceinline__ Elem element(const mi355q_compare_pair& p, int64_t e, bool kl, bool ratio) {
  const float t = nan_to_num(load_target(p, e));
  const float r = nan_to_num(p.reference[e]);
  Elem o;
  const float d = t - r;
  o.sq = d * d;
  o.r2 = r * r;
  o.kl = 0.f;
  if (kl) {
    const float pp = r > 0.f ? r : 0.f, qq = t > 0.f ? t : 0.f;
    o.kl = pp * logf((pp + 1e-9f) / (qq + 1e-9f));
  }
  o.tr = t * r;
  o.tt = t * t;
  o.rr = o.r2;
  o.ratio = ratio ? f2u(fabsf(d) / (fabsf(r) + 1e-6f)) : 0u;
  return o;
}

__device__ __forceinline__ uint32_t ratio_bits(const mi355q_compare_pair& p, int64_t e) {
  const float t = nan_to_num(load_target(p, e));
  const float r = nan_to_num(p.reference[e]);
  return f2u(fabsf(t - r) / (fabsf(r) + 1e-6f));
}

// ---------------------------------------------------------------- pass 1
__global__ __launch_bounds__(kThreads) void compare_sums_kernel(Batch b) {
  __shared__ uint32_t hist[kBins1];
  __shared__ int32_t leaf_start[kMaxLeaves], leaf_len[kMaxLeaves];
  __shared__ float leafv[3][kMaxLeaves];
  __shared__ int32_t stk_a[3][32], stk_b[3][32];
  __shared__ float stk_v[3][32];
  __shared__ int32_t n_leaves;
  __shared__ double red[3][kThreads / kWave];

  const int64_t chunk = blockIdx.x;
  if (!table_ok(b)) return;
  const int32_t pi = pair_of_chunk(b, chunk);
  const mi355q_compare_pair& p = pair_of(b, pi);
  const int64_t base = (chunk - first_chunk(b, pi)) * kChunk;
  if (base >= p.n) return;
  const int32_t m = static_cast<int32_t>(p.n - base < kChunk ? p.n - base : kChunk);
  const int tid = threadIdx.x;

  if (b.want_median)
    for (int i = tid; i < kBins1; i += kThreads) hist[i] = 0;
  if (tid == 0) {
    // NumPy's pairwise leaves of [0, m), in order (right child pushed first)
    int sp = 0, nl = 0;
    stk_a[0][0] = 0; stk_b[0][0] = m;
    while (sp >= 0) {
      const int s = stk_a[0][sp], len = stk_b[0][sp];
      --sp;
      if (len <= 128) {
        leaf_start[nl] = s; leaf_len[nl] = len; ++nl;
      } else {
        int n2 = len / 2;
        n2 -= n2 % 8;
        ++sp; stk_a[0][sp] = s + n2; stk_b[0][sp] = len - n2;
        ++sp; stk_a[0][sp] = s; stk_b[0][sp] = n2;
      }
    }
    n_leaves = nl;
  }
  __syncthreads();

  const int grp = tid >> 3, k = tid & 7;
  const int nl = n_leaves;
  const float* ref = p.reference + base;
  double a_tr = 0.0, a_tt = 0.0, a_rr = 0.0;
  for (int L = grp; L < nl; L += kThreads / 8) {
    const int s = leaf_start[L], len = leaf_len[L];
    float r_sq = 0.f, r_r2 = 0.f, r_kl = 0.f;
    const int full = len < 8 ? 0 : (len & ~7);
    if (full) {
      for (int j = k; j < full; j += 8) {
        const Elem v = element(p, base + s + j, b.want_kl, b.want_median);
        if (j == k) { r_sq = v.sq; r_r2 = v.r2; r_kl = v.kl; }
        else { r_sq = r_sq + v.sq; r_r2 = r_r2 + v.r2; r_kl = r_kl + v.kl; }
        a_tr += v.tr; a_tt += v.tt; a_rr += v.rr;
        if (b.want_median) atomicAdd(&hist[v.ratio >> 20], 1u);
      }
    }
    // ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)) on lane 0 of the group
#pragma unroll
    for (int off = 1; off < 8; off <<= 1) {
      const float o_sq = __shfl_xor(r_sq, off, kWave), o_r2 = __shfl_xor(r_r2, off, kWave),
                  o_kl = __shfl_xor(r_kl, off, kWave);
      r_sq = r_sq + o_sq; r_r2 = r_r2 + o_r2; r_kl = r_kl + o_kl;
    }
    if (k == 0) {
      if (!full) { r_sq = 0.f; r_r2 = 0.f; r_kl = 0.f; }   // n < 8: res = 0, then left to right
      for (int j = full; j < len; ++j) {
        const Elem v = element(p, base + s + j, b.want_kl, b.want_median);
        r_sq = r_sq + v.sq; r_r2 = r_r2 + v.r2; r_kl = r_kl + v.kl;
        a_tr += v.tr; a_tt += v.tt; a_rr += v.rr;
        if (b.want_median) atomicAdd(&hist[v.ratio >> 20], 1u);
      }
      leafv[0][L] = r_sq; leafv[1][L] = r_r2; leafv[2][L] = r_kl;
    }
  }
  (void)ref;
  __syncthreads();

  // balanced: m = leaf << depth with a leaf of 8 .. 128 elements, a multiple of 8 (every split exact)
  int depth = 0;
  while ((m >> depth) > 128) ++depth;
  const int leaf = m >> depth;
  if ((leaf << depth) == m && leaf >= 8 && leaf % 8 == 0) {
    for (int st = 1; st < nl; st <<= 1) {
      const int pairs = nl / (2 * st);
      for (int i = tid; i < 3 * pairs; i += kThreads) {
        const int qn = i / pairs, idx = (i - qn * pairs) * 2 * st;
        leafv[qn][idx] = leafv[qn][idx] + leafv[qn][idx + st];
      }
      __syncthreads();
    }
  } else if (tid < 3) {
    // one lane per sum walks the pairwise tree in post order (explicit stack in LDS, no recursion)
    const int qn = tid;
    int sp = 0, li = 0;
    bool have = false;
    float ret = 0.f;
    stk_a[qn][0] = m; stk_b[qn][0] = 0;   // (length, stage)
    while (true) {
      if (!have) {
        const int len = stk_a[qn][sp];
        if (len <= 128) {
          ret = leafv[qn][li++]; have = true; --sp;
        } else {
          int n2 = len / 2;
          n2 -= n2 % 8;
          stk_b[qn][sp] = 0;
          ++sp; stk_a[qn][sp] = n2;
        }
      } else {
        if (sp < 0) break;
        if (stk_b[qn][sp] == 0) {
          stk_v[qn][sp] = ret; stk_b[qn][sp] = 1;
          const int len = stk_a[qn][sp];
          int n2 = len / 2;
          n2 -= n2 % 8;
          ++sp; stk_a[qn][sp] = len - n2; have = false;
        } else {
          ret = stk_v[qn][sp] + ret; --sp;
        }
      }
    }
    leafv[qn][0] = ret;
  }

  // cosine sums: wave butterflies, then the four waves in order
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    a_tr += __shfl_xor(a_tr, off, kWave);
    a_tt += __shfl_xor(a_tt, off, kWave);
    a_rr += __shfl_xor(a_rr, off, kWave);
  }
  if ((tid & (kWave - 1)) == 0) {
    red[0][tid / kWave] = a_tr; red[1][tid / kWave] = a_tt; red[2][tid / kWave] = a_rr;
  }
  __syncthreads();

  if (b.want_median) {
    unsigned long long* g = b.hist + static_cast<int64_t>(pi) * kHistBins;
    for (int i = tid; i < kBins1; i += kThreads)
      if (hist[i]) atomicAdd(&g[i], static_cast<unsigned long long>(hist[i]));
  }
  if (tid == 0) {
    ChunkPartial o;
    o.sq = leafv[0][0]; o.r2 = leafv[1][0]; o.kl = leafv[2][0]; o.pad = 0.f;
    o.tr = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    o.tt = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    o.rr = ((red[2][0] + red[2][1]) + red[2][2]) + red[2][3];
    o.pad2 = 0.0;
    b.partials[chunk] = o;
  }
}

// chunk sums of every pair, left to right (one wave per pair)
__global__ __launch_bounds__(kWave) void compare_combine_kernel(Batch b) {
  const int32_t pi = blockIdx.x;
  if (!table_ok(b)) {
    if (threadIdx.x == 0) {
      mi355q_compare_result o{};
      o.sum_sq_diff = o.sum_ref_sq = o.sum_kl = o.median_lo = o.median_hi = __builtin_nanf("");
      o.dot_tr = o.dot_tt = o.dot_rr = __builtin_nan("");
      b.results[pi] = o;
    }
    return;
  }
  const mi355q_compare_pair& p = pair_of(b, pi);
  const int64_t c0 = first_chunk(b, pi);
  const int64_t nc = (p.n + kChunk - 1) / kChunk;
  const int lane = threadIdx.x;
  const ChunkPartial* part = b.partials + c0;
  double tr = 0.0, tt = 0.0, rr = 0.0;
  for (int64_t i = lane; i < nc; i += kWave) { tr += part[i].tr; tt += part[i].tt; rr += part[i].rr; }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    tr += __shfl_xor(tr, off, kWave);
    tt += __shfl_xor(tt, off, kWave);
    rr += __shfl_xor(rr, off, kWave);
  }
  // the chunk sums go through LDS a tile at a time (all lanes load, coalesced), so the three in-order chains
  // below wait on additions only, not on a global load per chunk
  __shared__ float tile[3][kCombineTile];
  float acc = 0.f;
  for (int64_t t0 = 0; t0 < nc; t0 += kCombineTile) {
    const int m = static_cast<int>(nc - t0 < kCombineTile ? nc - t0 : kCombineTile);
    for (int i = lane; i < m; i += kWave) {
      tile[0][i] = part[t0 + i].sq; tile[1][i] = part[t0 + i].r2; tile[2][i] = part[t0 + i].kl;
    }
    __syncthreads();
    if (lane < 3) {
      int i = 0;
      if (t0 == 0) { acc = tile[lane][0]; i = 1; }
#pragma unroll 16
      for (; i < m; ++i) acc = acc + tile[lane][i];
    }
    __syncthreads();
  }
  const float s_sq = __shfl(acc, 0, kWave), s_r2 = __shfl(acc, 1, kWave), s_kl = __shfl(acc, 2, kWave);
  if (lane == 0) {
    mi355q_compare_result o{};
    o.sum_sq_diff = s_sq; o.sum_ref_sq = s_r2; o.sum_kl = s_kl;
    o.median_lo = 0.f; o.median_hi = 0.f;
    o.dot_tr = tr; o.dot_tt = tt; o.dot_rr = rr;
    b.results[pi] = o;
  }
}

// ---------------------------------------------------------------- passes 2 and 3 of the median
template <int LEVEL>
__global__ __launch_bounds__(kThreads) void compare_hist_kernel(Batch b) {
  constexpr int kBins = LEVEL == 2 ? kBins2 : kBins3;
  __shared__ uint32_t hist[kBins];
  __shared__ uint32_t wmin[kThreads / kWave];
  const int64_t chunk = blockIdx.x;
  if (!table_ok(b)) return;
  const int32_t pi = pair_of_chunk(b, chunk);
  const mi355q_compare_pair& p = pair_of(b, pi);
  const int64_t base = (chunk - first_chunk(b, pi)) * kChunk;
  if (base >= p.n) return;
  const int64_t end = p.n - base < kChunk ? p.n : base + kChunk;
  const uint32_t prefix = b.state[pi].prefix;
  const int tid = threadIdx.x;
  for (int i = tid; i < kBins; i += kThreads) hist[i] = 0;
  __syncthreads();
  uint32_t mn = 0xFFFFFFFFu;
  for (int64_t e = base + tid; e < end; e += kThreads) {
    const uint32_t u = ratio_bits(p, e);
    if (LEVEL == 2) {
      if ((u >> 20) == prefix) atomicAdd(&hist[(u >> 9) & (kBins2 - 1)], 1u);
    } else {
      const uint32_t hi = u >> 9;
      if (hi == prefix) atomicAdd(&hist[u & (kBins3 - 1)], 1u);
      else if (hi > prefix && u < mn) mn = u;
    }
  }
  if (LEVEL == 3) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
      const uint32_t o = static_cast<uint32_t>(__shfl_xor(static_cast<int>(mn), off, kWave));
      mn = o < mn ? o : mn;
    }
    if ((tid & (kWave - 1)) == 0) wmin[tid / kWave] = mn;
  }
  __syncthreads();
  unsigned long long* g = b.hist + static_cast<int64_t>(pi) * kHistBins;
  for (int i = tid; i < kBins; i += kThreads)
    if (hist[i]) atomicAdd(&g[i], static_cast<unsigned long long>(hist[i]));
  if (LEVEL == 3 && tid == 0) {
    uint32_t w = wmin[0];
    for (int i = 1; i < kThreads / kWave; ++i) w = wmin[i] < w ? wmin[i] : w;
    if (w != 0xFFFFFFFFu) atomicMin(&b.state[pi].min_above, w);
  }
}

// Finds the bin that holds rank k of the pair's histogram, narrows the prefix and clears the histogram for
// the next pass. LEVEL 3 also places the upper middle value and writes the median pair.
template <int LEVEL>
__global__ __launch_bounds__(kThreads) void compare_select_kernel(Batch b) {
  constexpr int kBins = LEVEL == 1 ? kBins1 : (LEVEL == 2 ? kBins2 : kBins3);
  constexpr int kPer = kBins / kThreads;
  __shared__ unsigned long long bins[kBins];
  __shared__ unsigned long long part[kThreads];
  const int32_t pi = blockIdx.x;
  if (!table_ok(b)) return;
  const mi355q_compare_pair& p = pair_of(b, pi);
  if (p.n <= 0) return;
  const int tid = threadIdx.x;
  unsigned long long* g = b.hist + static_cast<int64_t>(pi) * kHistBins;
  unsigned long long s = 0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const unsigned long long v = g[tid * kPer + j];
    bins[tid * kPer + j] = v;
    s += v;
  }
  part[tid] = s;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kPer; ++j) g[tid * kPer + j] = 0ull;
  if (tid != 0) return;
  SelectState st = b.state[pi];
  if (LEVEL == 1) { st.k = (p.n - 1) / 2; st.prefix = 0; st.min_above = 0xFFFFFFFFu; }
  // the bin of rank k (k < the histogram's total by construction)
  int64_t below = 0;
  int t = 0;
  while (t < kThreads - 1 && below + static_cast<int64_t>(part[t]) <= st.k) below += static_cast<int64_t>(part[t++]);
  int bin = t * kPer;
  while (bin < kBins - 1 && below + static_cast<int64_t>(bins[bin]) <= st.k) below += static_cast<int64_t>(bins[bin++]);
  if (LEVEL < 3) {
    st.prefix = (st.prefix << (LEVEL == 1 ? 0 : 11)) | static_cast<uint32_t>(bin);
    st.k -= below;
    st.min_above = 0xFFFFFFFFu;
    b.state[pi] = st;
    return;
  }
  const uint32_t lo = (st.prefix << 9) | static_cast<uint32_t>(bin);
  // the upper middle value: rank k + 1 for even n, counted from the bins below `bin`
  uint32_t hi = lo;
  if ((p.n & 1) == 0) {
    const int64_t r2 = st.k + 1;
    int64_t cum = below + static_cast<int64_t>(bins[bin]);
    int b2 = bin;
    while (cum <= r2 && b2 < kBins - 1) cum += static_cast<int64_t>(bins[++b2]);
    hi = cum > r2 ? ((st.prefix << 9) | static_cast<uint32_t>(b2)) : st.min_above;
  }
  b.results[pi].median_lo = u2f(lo);
  b.results[pi].median_hi = u2f(hi);
}

__device__ bool pair_valid(const mi355q_compare_pair& p) {
  if (p.n < 0) return false;
  if (p.n == 0) return true;
  if (!p.reference || !p.target || p.target_kind < MI355Q_CMP_F32 || p.target_kind > MI355Q_CMP_I2) return false;
  if (p.target_kind >= MI355Q_CMP_I8)
    return p.scale && p.channels >= 1 && p.inner >= 1 && (p.diff_bits == 8 || p.diff_bits == 16 || p.diff_bits == 32);
  return true;
}

// chunk0[i] = first chunk of pair i; chunk0[count] = the total, or -1 when an entry is invalid or the total is not
// the `total_chunks` the grids were sized for (see table_ok)
__global__ __launch_bounds__(kWave) void compare_chunk_table_kernel(const mi355q_compare_pair* pairs, int32_t count,
                                                                    int64_t total_chunks, int64_t* chunk0) {
  if (threadIdx.x != 0) return;
  int64_t c = 0;
  bool ok = true;
  for (int32_t i = 0; i < count; ++i) {
    chunk0[i] = c;
    const int64_t n = pairs[i].n;
    ok = ok && pair_valid(pairs[i]);
    c += n > 0 ? (n + kChunk - 1) / kChunk : 0;
  }
  chunk0[count] = ok && c == total_chunks ? c : -1;
}

size_t align256(size_t v) { return (v + 255) & ~static_cast<size_t>(255); }

struct Layout {
  size_t chunk0, partials, hist, state, total;
};

Layout layout(int32_t count, int64_t total_chunks) {
  Layout l;
  l.chunk0 = 0;
  l.partials = align256(sizeof(int64_t) * (static_cast<size_t>(count) + 1));
  l.hist = l.partials + align256(sizeof(ChunkPartial) * static_cast<size_t>(total_chunks));
  l.state = l.hist + align256(sizeof(unsigned long long) * kHistBins * static_cast<size_t>(count));
  l.total = l.state + align256(sizeof(SelectState) * static_cast<size_t>(count));
  return l;
}

int32_t check_pair(const mi355q_compare_pair& p, int32_t i) {
  if (p.n < 0) return fail(MI355Q_BAD_ARG, "negative element count (pair %d)", i);
  if (p.n == 0) return MI355Q_OK;
  if (!p.reference || !p.target) return fail(MI355Q_BAD_ARG, "null operand (pair %d)", i);
  if (p.target_kind < MI355Q_CMP_F32 || p.target_kind > MI355Q_CMP_I2)
    return fail(MI355Q_BAD_ARG, "unknown target kind %d (pair %d)", p.target_kind, i);
  if (p.target_kind >= MI355Q_CMP_I8) {
    if (!p.scale) return fail(MI355Q_BAD_ARG, "integer target without scales (pair %d)", i);
    if (p.channels < 1 || p.inner < 1) return fail(MI355Q_BAD_ARG, "channels and inner must be >= 1 (pair %d)", i);
    if (p.diff_bits != 8 && p.diff_bits != 16 && p.diff_bits != 32)
      return fail(MI355Q_BAD_ARG, "diff_bits must be 8, 16 or 32 (pair %d)", i);
  }
  return MI355Q_OK;
}

int32_t run(Batch& b, int64_t total_chunks, void* workspace, size_t workspace_bytes, hipStream_t st) {
  const Layout l = layout(b.count, total_chunks);
  if (!workspace || workspace_bytes < l.total)
    return fail(MI355Q_BAD_ARG, "workspace of %zu bytes is smaller than the %zu needed", workspace_bytes, l.total);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  b.chunk0 = reinterpret_cast<int64_t*>(ws + l.chunk0);
  b.partials = reinterpret_cast<ChunkPartial*>(ws + l.partials);
  b.hist = reinterpret_cast<unsigned long long*>(ws + l.hist);
  b.state = reinterpret_cast<SelectState*>(ws + l.state);
  if (b.table) {
    hipLaunchKernelGGL(compare_chunk_table_kernel, dim3(1), dim3(kWave), 0, st, b.table, b.count, total_chunks,
                       const_cast<int64_t*>(b.chunk0));
    MI355Q_CHECK_LAUNCH("compare chunk table launch");
  }
  if (b.want_median && hipMemsetAsync(b.hist, 0, sizeof(unsigned long long) * kHistBins * b.count, st) != hipSuccess)
    return fail(MI355Q_HIP_ERROR, "hipMemsetAsync failed");
  if (total_chunks > 0) {
    hipLaunchKernelGGL(compare_sums_kernel, dim3(static_cast<unsigned>(total_chunks)), dim3(kThreads), 0, st, b);
    MI355Q_CHECK_LAUNCH("compare sums launch");
  }
  hipLaunchKernelGGL(compare_combine_kernel, dim3(b.count), dim3(kWave), 0, st, b);
  MI355Q_CHECK_LAUNCH("compare combine launch");
  if (b.want_median && total_chunks > 0) {
    hipLaunchKernelGGL(compare_select_kernel<1>, dim3(b.count), dim3(kThreads), 0, st, b);
    hipLaunchKernelGGL(compare_hist_kernel<2>, dim3(static_cast<unsigned>(total_chunks)), dim3(kThreads), 0, st, b);
    hipLaunchKernelGGL(compare_select_kernel<2>, dim3(b.count), dim3(kThreads), 0, st, b);
    hipLaunchKernelGGL(compare_hist_kernel<3>, dim3(static_cast<unsigned>(total_chunks)), dim3(kThreads), 0, st, b);
    hipLaunchKernelGGL(compare_select_kernel<3>, dim3(b.count), dim3(kThreads), 0, st, b);
    MI355Q_CHECK_LAUNCH("compare median launch");
  }
  return MI355Q_OK;
}

}  // namespace
}  // namespace mi355q

using namespace mi355q;

extern "C" int64_t mi355q_compare_chunks(int64_t n) { return n > 0 ? (n + kChunk - 1) / kChunk : 0; }

extern "C" size_t mi355q_compare_workspace_bytes(int32_t count, int64_t total_chunks) {
  if (count < 0 || total_chunks < 0) return 0;
  return layout(count, total_chunks).total;
}

extern "C" int32_t mi355q_compare_f32(const float* reference, const void* target, int64_t n, int32_t target_kind,
                                      int32_t diff_bits, int64_t channels, int64_t inner, const float* scale,
                                      const int32_t* zero_point, int32_t flags, mi355q_compare_result* result,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  clear_error();
  Batch b{};
  b.one.reference = reference; b.one.target = target; b.one.n = n; b.one.target_kind = target_kind;
  b.one.diff_bits = diff_bits; b.one.channels = channels; b.one.inner = inner; b.one.scale = scale;
  b.one.zero_point = zero_point;
  if (int32_t s = check_pair(b.one, 0)) return s;
  if (n == 0) return MI355Q_OK;
  if (!result) return fail(MI355Q_BAD_ARG, "null result pointer");
  b.table = nullptr;
  b.count = 1;
  b.want_median = (flags & MI355Q_COMPARE_MEDIAN) != 0;
  b.want_kl = (flags & MI355Q_COMPARE_NO_KL) == 0;
  b.results = result;
  return run(b, mi355q_compare_chunks(n), workspace, workspace_bytes, as_stream(stream));
}

extern "C" int32_t mi355q_compare_f32_batched(const mi355q_compare_pair* pairs, int32_t count, int64_t total_chunks,
                                              int32_t flags, mi355q_compare_result* results, void* workspace,
                                              size_t workspace_bytes, void* stream) {
  clear_error();
  if (count < 0 || total_chunks < 0) return fail(MI355Q_BAD_ARG, "negative count");
  if (count == 0) return MI355Q_OK;
  if (!pairs || !results) return fail(MI355Q_BAD_ARG, "null pointer");
  if (total_chunks > 0x7FFFFFFFLL) return fail(MI355Q_BAD_ARG, "too many chunks for one launch");
  Batch b{};
  b.table = pairs;
  b.count = count;
  b.want_median = (flags & MI355Q_COMPARE_MEDIAN) != 0;
  b.want_kl = (flags & MI355Q_COMPARE_NO_KL) == 0;
  b.results = results;
  return run(b, total_chunks, workspace, workspace_bytes, as_stream(stream));
}
