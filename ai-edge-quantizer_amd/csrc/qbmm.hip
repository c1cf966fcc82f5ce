// Integer execution of a quantized BATCH_MATMUL op (include/mi355q.h, "Integer batched matrix product").
//
//   acc[b,m,n] = Sum_k (A[b,m,k] - za) (B[b',k,n] - zb), b' = b or 0, exact in int32 for K <= 32768.
//
//   qbmm_mfma_kernel     Sum a b on v_mfma_i32_16x16x64_i8: the main loop and the tile of qfc_tile.h (a wave on 64 x 64
//                        outputs, a workgroup of 2 x 2 waves on 128 x 128) with the batch on blockIdx.z. Both operands
//                        are read contiguous along K, 16 consecutive k per lane.
//   transpose_kernel     An operand that is strided along K (a with adj_x, [K, M]; b without adj_y, [K, N], the default
//                        layout) is first transposed into the workspace, 64 x 64 byte tiles through LDS with 16-byte
//                        loads and stores. A route that staged such an operand through LDS inside the product (4 x 4
//                        byte transposes with v_perm_b32, one barrier per K step) was built, gave the same bits and
//                        was measured 5.3 - 6.6 x SLOWER than transposing first (profiles/qbmm_staged_bench.json),
//                        so it is not kept.
//   qbmm_generic_kernel  one thread per output, one element at a time: every other shape and alignment, same bits.
//   zero points          Sum_k a and Sum_k b (the weight sums of qfc_frag.h on the K-contiguous operands) give the terms
//                        of the MFMA route: acc = Sum a b - zb Sum_k a - za Sum_k b + K za zb. Each of the four terms is
//                        at most 2^29 in magnitude and exact in int32; a partial sum of them can pass 2^31, so they are
//                        combined in uint32, whose wrap-around is defined: the result is the total modulo 2^32, and the
//                        total lies within int32, so it is the total. No intermediate needs int64.
//   one matrix           batch = 1, (adj_x, adj_y) = (0, 1) and b_zero_point = 0 IS the FULLY_CONNECTED problem: the
//                        forward entry hands it to mi355q_qfc_forward_i8 (same statement, same bits, its kernel).
#include "common.h"
#include "compare_target.h"
#include "qfc_epilogue.h"
#include "qfc_tile.h"

namespace mi355q {
namespace {

constexpr int kThreads = kQfcThreads;
constexpr int kBmmMaxK = 32768;       // K * 255 * 255 < 2^31
constexpr int kStep = 64;             // elements of K per MFMA step
constexpr int kTile = 128;            // a workgroup's rows of M and of N
constexpr unsigned kMaxGridZ = 65535;

struct BmmArgs {
  const int8_t* a;         // [batch, M, K] or [batch, K, M]
  const int8_t* b;         // [b_batch, K, N] or [b_batch, N, K]
  const float* a_scale;    // 1 or batch * M
  const float* b_scale;    // 1 or N
  const int32_t* asum;     // [batch * M]   (read only when zb != 0, MFMA route)
  const int32_t* bsum;     // [b_batch * N] (read only when za != 0, MFMA route)
  float* y;                // [batch, M, N] or null (the output entry)
  int32_t* acc;            // [batch, M, N] or null
  OutArgs out;             // the output entry: q, mult, shift, per_channel, zp_y, act_min, act_max; bias null
  long long batch, M, N, K;
  int b_shared;            // b_batch == 1
  int a_per_row, b_per_chan;
  int za, zb;
  int adj_x, adj_y;
};

// What one output leaves as: the float rescale (and the accumulator), or the stored int8.
template <bool TOQ>
__device__ __forceinline__ void bmm_store(const BmmArgs& g, long long bz, long long m, long long n, int v, float sb,
                                          const Chan8& c8) {
  const long long o = (bz * g.M + m) * g.N + n;
  if constexpr (!TOQ) {
    const float sc = g.a_scale[g.a_per_row ? bz * g.M + m : 0] * sb;
    g.y[o] = static_cast<float>(v) * sc;
    if (g.acc) g.acc[o] = v;
  } else {
    static_cast<int8_t*>(g.out.q)[o] = output8(v, c8, g.out);
  }
}

// ---------------------------------------------------------------- the transposing pre-pass
// out [G, C, R] = in [G, R, C]^T for R % 64 == 0, C % 16 == 0, both 16-byte aligned: a workgroup takes a 64 x 64 tile,
// every thread one 16-byte load along C and one 16-byte store along R; the tile turns in LDS (rows of 64 + 4 bytes).
constexpr int kTr = 64, kTrRow = kTr + 4;

__global__ __launch_bounds__(kThreads) void transpose_kernel(const int8_t* __restrict__ in, long long R, long long C,
                                                             int8_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) int8_t tile[kTr * kTrRow];
  const long long grp = blockIdx.z, r0 = static_cast<long long>(blockIdx.y) * kTr, c0 = static_cast<long long>(blockIdx.x) * kTr;
  const int row = threadIdx.x >> 2, chunk = threadIdx.x & 3;
  const int8_t* src = in + grp * R * C;
  int8_t* dst = out + grp * R * C;
  if (c0 + 16 * chunk < C) {
    const I32x4 v = *reinterpret_cast<const I32x4*>(src + (r0 + row) * C + c0 + 16 * chunk);
#pragma unroll
    for (int w = 0; w < 4; ++w) *reinterpret_cast<int*>(tile + row * kTrRow + 16 * chunk + 4 * w) = v[w];
  }
  __syncthreads();
  if (c0 + row < C) {      // (this thread's output row is column `row` of the tile)
    I32x4 v;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      uint32_t word = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        word |= static_cast<uint32_t>(static_cast<uint8_t>(tile[(16 * chunk + 4 * w + e) * kTrRow + row])) << (8 * e);
      v[w] = static_cast<int>(word);
    }
    *reinterpret_cast<I32x4*>(dst + (c0 + row) * R + r0 + 16 * chunk) = v;
  }
}

// ---------------------------------------------------------------- the MFMA route
// K % 64 == 0; a [batch, M, K] and b [b_batch, N, K] 16-byte aligned, both contiguous along K (as given, or transposed
// by the pre-pass): the main loop of the FULLY_CONNECTED kernels with the batch on blockIdx.z.
template <bool TOQ>
__global__ __launch_bounds__(kThreads) void qbmm_mfma_kernel(BmmArgs g) {
  QfcWave wv;
  if (!qfc_wave<int8_t>(wv, g.M, g.N)) return;
  const long long bz = blockIdx.z;
  I32x4 acc[QfcTile<int8_t>::TM][TB];
  qfc_main_loop<int8_t, MI355Q_CMP_I8, kStep>(wv, g.a + bz * g.M * g.K,
                                              reinterpret_cast<const uint8_t*>(g.b + (g.b_shared ? 0 : bz) * g.N * g.K), g.M,
                                              g.N, g.K, acc);
  struct Chan {
    float sb;
    uint32_t corr;       // za Sum_k b - K za zb, modulo 2^32
    Chan8 c8;
  };
  qfc_walk_outputs<int8_t>(
      wv, g.M, g.N,
      [=](long long n) {
        Chan c;
        c.sb = TOQ ? 0.0f : g.b_scale[g.b_per_chan ? n : 0];
        c.corr = g.za != 0 ? static_cast<uint32_t>(g.za * g.bsum[(g.b_shared ? 0 : bz) * g.N + n]) -
                                 static_cast<uint32_t>(static_cast<int>(g.K) * g.za * g.zb)
                           : 0u;
        c.c8 = TOQ ? chan8(g.out, n) : Chan8{0, 0, 0, 0};
        return c;
      },
      [=, &acc](const Chan& c, int i, int j, int e, long long m, long long n) {
        uint32_t v = static_cast<uint32_t>(acc[i][j][e]) - c.corr;
        if (g.zb != 0) v -= static_cast<uint32_t>(g.zb * g.asum[bz * g.M + m]);
        bmm_store<TOQ>(g, bz, m, n, static_cast<int>(v), c.sb, c.c8);
      });
}

// ---------------------------------------------------------------- the generic route
__global__ __launch_bounds__(kThreads) void qbmm_generic_kernel(BmmArgs g) {
  const long long total = g.batch * g.M * g.N, step = static_cast<long long>(gridDim.x) * kThreads;
  for (long long o = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; o < total; o += step) {
    const long long n = o % g.N, m = (o / g.N) % g.M, bz = o / (g.N * g.M);
    const int8_t* ab = g.a + bz * g.M * g.K;
    const int8_t* bb = g.b + (g.b_shared ? 0 : bz) * g.N * g.K;
    const long long a0 = g.adj_x ? m : m * g.K, as = g.adj_x ? g.M : 1;
    const long long b0 = g.adj_y ? n * g.K : n, bs = g.adj_y ? 1 : g.N;
    int acc = 0;
    for (long long k = 0; k < g.K; ++k) acc += (static_cast<int>(ab[a0 + k * as]) - g.za) * (static_cast<int>(bb[b0 + k * bs]) - g.zb);
    if (g.y) bmm_store<false>(g, bz, m, n, acc, g.b_scale[g.b_per_chan ? n : 0], Chan8{0, 0, 0, 0});
    else bmm_store<true>(g, bz, m, n, acc, 0.0f, chan8(g.out, n));
  }
}

// ---------------------------------------------------------------- host side
inline size_t sums_bytes(int64_t count) {
  return (static_cast<size_t>(count) * sizeof(int32_t) + 255) & ~static_cast<size_t>(255);
}

inline size_t copy_bytes(int64_t count) { return (static_cast<size_t>(count) + 255) & ~static_cast<size_t>(255); }

inline bool mfma_shape(const void* a, int64_t M, int64_t K, int32_t adj_x, const void* b, int64_t N, int32_t adj_y) {
  return K > 0 && K % kStep == 0 && reinterpret_cast<uintptr_t>(a) % 16 == 0 && reinterpret_cast<uintptr_t>(b) % 16 == 0 &&
         (!adj_x || M % 16 == 0) && (adj_y || N % 16 == 0);
}

inline bool bmm_mfma_route(const BmmArgs& g) { return mfma_shape(g.a, g.M, g.K, g.adj_x, g.b, g.N, g.adj_y); }

// out [groups, C, K] of in [groups, K, C]
int32_t launch_transpose(const int8_t* in, long long groups, long long K, long long C, int8_t* out, hipStream_t st) {
  const dim3 grid(static_cast<unsigned>((C + kTr - 1) / kTr), static_cast<unsigned>(K / kTr), static_cast<unsigned>(groups));
  hipLaunchKernelGGL(transpose_kernel, grid, dim3(kThreads), 0, st, in, K, C, out);
  MI355Q_CHECK_LAUNCH("operand transpose launch");
  return MI355Q_OK;
}

// The launches that both entries share; g.y / g.acc / g.out say which entry it is. The workspace holds, each rounded up
// to 256 bytes: Sum_k a [batch M] and Sum_k b [b_batch N] (int32), then a^T and b^T where the layout needs them.
int32_t run_bmm(BmmArgs& g, int64_t b_batch, void* workspace, size_t workspace_bytes, hipStream_t st) {
  if (g.batch == 0 || g.M == 0 || g.N == 0) return MI355Q_OK;
  if (!bmm_mfma_route(g)) {
    hipLaunchKernelGGL(qbmm_generic_kernel, dim3(generic_blocks(g.batch * g.M * g.N)), dim3(kThreads), 0, st, g);
    MI355Q_CHECK_LAUNCH("integer batched matrix product launch");
    return MI355Q_OK;
  }
  const int64_t n_tiles = (g.N + kTile - 1) / kTile, m_tiles = (g.M + kTile - 1) / kTile;
  if (m_tiles > 65535 || n_tiles > 0x7FFFFFFFLL || g.batch > kMaxGridZ)
    return fail(MI355Q_UNSUPPORTED, "too many tiles or batches for one launch");
  const size_t at_bytes = g.adj_x ? copy_bytes(g.batch * g.M * g.K) : 0, bt_bytes = g.adj_y ? 0 : copy_bytes(b_batch * g.N * g.K);
  const size_t sums = sums_bytes(g.batch * g.M) + sums_bytes(b_batch * g.N);
  if (at_bytes + bt_bytes > 0) {
    if (const int32_t bad = check_workspace(workspace, workspace_bytes, sums + at_bytes + bt_bytes)) return bad;
    if (reinterpret_cast<uintptr_t>(workspace) % 16) return fail(MI355Q_BAD_ARG, "the workspace is not 16-byte aligned");
  }
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  if (g.adj_x) {
    int8_t* at = reinterpret_cast<int8_t*>(ws + sums);
    if (const int32_t bad = launch_transpose(g.a, g.batch, g.K, g.M, at, st)) return bad;
    g.a = at;
  }
  if (!g.adj_y) {
    int8_t* bt = reinterpret_cast<int8_t*>(ws + sums + at_bytes);
    if (const int32_t bad = launch_transpose(g.b, b_batch, g.K, g.N, bt, st)) return bad;
    g.b = bt;
  }
  if (g.zb != 0) {
    int32_t* asum = reinterpret_cast<int32_t*>(ws);
    if (const int32_t bad = launch_weight_sums(reinterpret_cast<const uint8_t*>(g.a), MI355Q_CMP_I8, g.batch * g.M, g.K, asum, st))
      return bad;
    g.asum = asum;
  }
  if (g.za != 0) {
    int32_t* bsum = reinterpret_cast<int32_t*>(ws + sums_bytes(g.batch * g.M));
    if (const int32_t bad = launch_weight_sums(reinterpret_cast<const uint8_t*>(g.b), MI355Q_CMP_I8, b_batch * g.N, g.K, bsum, st))
      return bad;
    g.bsum = bsum;
  }
  const dim3 grid(static_cast<unsigned>(n_tiles), static_cast<unsigned>(m_tiles), static_cast<unsigned>(g.batch));
  if (g.y) hipLaunchKernelGGL(qbmm_mfma_kernel<false>, grid, dim3(kThreads), 0, st, g);
  else hipLaunchKernelGGL(qbmm_mfma_kernel<true>, grid, dim3(kThreads), 0, st, g);
  MI355Q_CHECK_LAUNCH("integer batched matrix product launch");
  return MI355Q_OK;
}

// The checks of the operands that both entries make, in the order of the header.
int32_t check_operands(const void* a, int64_t batch, int64_t M, int64_t K, int32_t a_zero_point, const void* b,
                       int64_t b_batch, int64_t N, int32_t b_zero_point) {
  if (batch < 0 || M < 0 || K < 0 || N < 0 || b_batch < 0) return fail(MI355Q_BAD_ARG, "negative shape");
  if (!a || !b) return fail(MI355Q_BAD_ARG, "null pointer");
  if (a_zero_point < -128 || a_zero_point > 127)
    return fail(MI355Q_BAD_ARG, "zero point %d of a is outside int8", a_zero_point);
  if (b_zero_point < -128 || b_zero_point > 127)
    return fail(MI355Q_BAD_ARG, "zero point %d of b is outside int8", b_zero_point);
  if (b_batch != 1 && b_batch != batch)
    return fail(MI355Q_BAD_SHAPE, "b_batch must be 1 or batch = %lld (got %lld)", static_cast<long long>(batch),
                static_cast<long long>(b_batch));
  if (K > kBmmMaxK)
    return fail(MI355Q_UNSUPPORTED, "K = %lld exceeds %d (the int32 accumulator)", static_cast<long long>(K), kBmmMaxK);
  return MI355Q_OK;
}

int32_t check_bmm_workspace(int64_t batch, int64_t M, int64_t N, int64_t b_batch, int32_t za, int32_t zb,
                            const void* workspace, size_t workspace_bytes) {
  if (za == 0 && zb == 0) return MI355Q_OK;
  if (const int32_t bad = check_workspace(workspace, workspace_bytes, sums_bytes(batch * M) + sums_bytes(b_batch * N))) return bad;
  if (reinterpret_cast<uintptr_t>(workspace) % 4) return fail(MI355Q_BAD_ARG, "the workspace is not 4-byte aligned (int32 sums)");
  return MI355Q_OK;
}

void fill_operands(BmmArgs& g, const int8_t* a, int64_t batch, int64_t M, int64_t K, int32_t adj_x, int32_t za,
                   const int8_t* b, int64_t b_batch, int64_t N, int32_t adj_y, int32_t zb) {
  g.a = a; g.b = b; g.batch = batch; g.M = M; g.N = N; g.K = K;
  g.b_shared = (b_batch == 1 && batch != 1) ? 1 : 0;
  g.za = za; g.zb = zb; g.adj_x = adj_x ? 1 : 0; g.adj_y = adj_y ? 1 : 0;
}

}  // namespace
}  // namespace mi355q

using namespace mi355q;

extern "C" size_t mi355q_qbmm_workspace_bytes(int64_t batch, int64_t M, int64_t K, int32_t adj_x, int64_t b_batch, int64_t N,
                                              int32_t adj_y) {
  if (batch <= 0 || M <= 0 || K <= 0 || N <= 0 || b_batch <= 0) return 0;
  return sums_bytes(batch * M) + sums_bytes(b_batch * N) + (adj_x ? copy_bytes(batch * M * K) : 0) +
         (adj_y ? 0 : copy_bytes(b_batch * N * K));
}

// (a query, not a status: int64_t, as mi355q_compare_chunks is)
extern "C" int64_t mi355q_qbmm_mfma_route(const void* a, int64_t M, int64_t K, int32_t adj_x, const void* b, int64_t N,
                                          int32_t adj_y) {
  return mfma_shape(a, M, K, adj_x, b, N, adj_y) ? 1 : 0;
}

extern "C" int32_t mi355q_qbmm_forward_i8(const int8_t* a, int64_t batch, int64_t M, int64_t K, int32_t adj_x,
                                          const float* a_scale, int64_t a_scale_count, int32_t a_zero_point,
                                          const int8_t* b, int64_t b_batch, int64_t N, int32_t adj_y, const float* b_scale,
                                          int64_t b_scale_count, int32_t b_zero_point, float* y_out, int32_t* acc_out,
                                          void* workspace, size_t workspace_bytes, void* stream) {
  clear_error();
  if (const int32_t bad = check_operands(a, batch, M, K, a_zero_point, b, b_batch, N, b_zero_point)) return bad;
  if (!a_scale || !b_scale || !y_out) return fail(MI355Q_BAD_ARG, "null pointer");
  if (a_scale_count != 1 && a_scale_count != batch * M)
    return fail(MI355Q_BAD_ARG, "a_scale_count must be 1 or batch * M = %lld (got %lld)", static_cast<long long>(batch * M),
                static_cast<long long>(a_scale_count));
  if (b_scale_count != 1 && b_scale_count != N)
    return fail(MI355Q_BAD_ARG, "b_scale_count must be 1 or N = %lld (got %lld)", static_cast<long long>(N),
                static_cast<long long>(b_scale_count));
  if (const int32_t bad = check_bmm_workspace(batch, M, N, b_batch, a_zero_point, b_zero_point, workspace, workspace_bytes))
    return bad;
  // one matrix against K-contiguous rows without a zero point of their own is the FULLY_CONNECTED problem
  if (batch == 1 && !adj_x && adj_y && b_zero_point == 0 && M > 0 && N > 0 && K > 0)
    return mi355q_qfc_forward_i8(a, M, K, a_scale, a_scale_count, a_zero_point, b, MI355Q_CMP_I8, N, b_scale, b_scale_count, 0,
                                 y_out, acc_out, workspace, workspace_bytes, stream);
  BmmArgs g{};
  fill_operands(g, a, batch, M, K, adj_x, a_zero_point, b, b_batch, N, adj_y, b_zero_point);
  g.a_scale = a_scale; g.b_scale = b_scale; g.y = y_out; g.acc = acc_out;
  g.a_per_row = (a_scale_count != 1) ? 1 : 0;
  g.b_per_chan = (b_scale_count != 1) ? 1 : 0;
  return run_bmm(g, b_batch, workspace, workspace_bytes, as_stream(stream));
}

extern "C" int32_t mi355q_qbmm_output_i8(const int8_t* a, int64_t batch, int64_t M, int64_t K, int32_t adj_x,
                                         int32_t a_zero_point, const int8_t* b, int64_t b_batch, int64_t N, int32_t adj_y,
                                         int32_t b_zero_point, const int32_t* multiplier, const int32_t* shift,
                                         int64_t mcount, int32_t out_zero_point, int8_t* q_out, void* workspace,
                                         size_t workspace_bytes, void* stream) {
  clear_error();
  if (const int32_t bad = check_operands(a, batch, M, K, a_zero_point, b, b_batch, N, b_zero_point)) return bad;
  if (!multiplier || !shift || !q_out) return fail(MI355Q_BAD_ARG, "null pointer");
  if (mcount != 1 && mcount != N)
    return fail(MI355Q_BAD_ARG, "mcount must be 1 or N = %lld (got %lld)", static_cast<long long>(N),
                static_cast<long long>(mcount));
  if (out_zero_point < -128 || out_zero_point > 127)
    return fail(MI355Q_BAD_ARG, "output zero point %d is outside int8", out_zero_point);
  if (const int32_t bad = check_bmm_workspace(batch, M, N, b_batch, a_zero_point, b_zero_point, workspace, workspace_bytes))
    return bad;
  BmmArgs g{};
  fill_operands(g, a, batch, M, K, adj_x, a_zero_point, b, b_batch, N, adj_y, b_zero_point);
  g.out.mult = multiplier; g.out.shift = shift; g.out.q = q_out;
  g.out.per_channel = (mcount != 1) ? 1 : 0;
  g.out.zp_y = out_zero_point; g.out.act_min = -128; g.out.act_max = 127;
  return run_bmm(g, b_batch, workspace, workspace_bytes, as_stream(stream));
}
