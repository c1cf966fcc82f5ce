// The staged MFMA route of the int8 FULLY_CONNECTED kernels: acc = Xq W^^T for ANY reduction length 1 <= d <= 65536 and
// ANY byte alignment of xq and w (stored I8, per-tensor or per-channel scales). The two kernels of qfc_staged.hip run
// qfc_staged_loop where qfc.hip's and qfc_out.hip's run qfc_main_loop, and then the same epilogues (qfc_tile_out.h).
// (The aligned route, d % 64 == 0 from 16-byte aligned bases, keeps qfc_main_loop: its fragments come straight from
// global memory.)
//
// Tiling: as qfc_tile.h. 256 threads = 2 x 2 waves, a workgroup owns 128 tokens x 128 channels, a wave 4 x 4 tiles of
// v_mfma_i32_16x16x64_i8 in 64 accumulator registers; lane, row / column and C / D maps are QfcWave's, so
// qfc_walk_outputs applies unchanged.
//
// Stage: kStageK = 64 bytes of the reduction dimension of the workgroup's 128 rows of xq and 128 rows of w, copied
// into LDS once per workgroup. Four threads share a row and take 16 bytes each, 64 rows per pass, four passes (two
// per operand). A thread's 16 bytes begin at byte p = base + row * d + k, of any alignment: it reads the five aligned
// words that cover [p, p + 16) and shifts each pair by p & 3 bytes with v_alignbyte_b32 (p & 3 is the same in every
// stage, a stage being 64 bytes), clears the bytes at k >= d, and stores the 16 bytes with one ds_write_b128. Rows
// t >= n and r >= rows, and every byte at k >= d, are ZERO in LDS, so the padded tail of the last stage adds nothing
// and acc is the sum over the true d (the x_zero_point term, zp * Sum_k w[r, k] from weight_sums_kernel, stays exact).
//
// Bounds: only words that hold at least one wanted byte of the tensor are read. Such a word is aligned and either
// lies wholly inside [base, base + rows * d) -- inside one row or straddling two -- and is read whole, or it is the
// tensor's own first or last partial word (base or end not a multiple of 4): staged_edge_word reads that one byte by
// byte, the bytes inside the tensor only. No load touches a byte outside the tensor.
//
// LDS: two buffers of 256 rows at a pitch of kPitch = 80 bytes (64 + 16) = 40960 bytes. A fragment read is one
// ds_read_b128 per lane at row (lane & 15), k-group (lane >> 4): byte row * 80 + 16 * group. In units of the 4-byte
// banks row r begins at bank 20 r: for r = 0 .. 15 that is 0, 20, 40, 60, 16, 36, 56, 12, 32, 52, 8, 28, 48, 4, 24, 44
// (mod 64), sixteen different multiples of 4, so the sixteen rows of one k-group cover 64 banks once each, four banks
// per lane; mod 32 any eight consecutive rows do the same with 32 banks. A pitch of 64 would put every row on the
// same four banks. The 16-byte stores of the staging threads (four per row, consecutive) follow the same map.
//
// Pipeline: the global loads of stage s + 1 are issued before the MFMAs of stage s, and shifted and stored into the
// other buffer after them; ONE barrier per stage. The store of stage s + 1 goes to the buffer that was read during
// stage s - 1, and every wave has passed the barrier that ended stage s - 1 after its reads.
//
// Barriers and partial tiles: every wave of the workgroup stages and takes every barrier. A wave whose tile lies
// outside the problem (own == false) skips only its fragment reads and MFMAs here, and returns after the loop.
#pragma once

#include "qfc_tile.h"

namespace mi355q {
namespace {

constexpr int kStageK = 64;                    // bytes of the reduction dimension per stage
constexpr int kPitch = kStageK + 16;           // LDS bytes from a row to the next
constexpr int kStageRows = 2 * QfcTile<int8_t>::BTA;          // 128 rows of xq, then 128 rows of w
constexpr int kStagePasses = kStageRows / (kQfcThreads / 4);  // 64 rows per pass
static_assert(QfcTile<int8_t>::BTA == QfcTile<int8_t>::BTB && kStagePasses == 4, "two passes per operand");

// One operand as the staging threads address it: byte offsets from `a0`, the base rounded down to a word.
struct StagedOperand {
  const uint8_t* a0;
  long long lo, hi;       // the tensor is [lo, hi) from a0: lo = base & 3
};

// (pointer arithmetic on `base`, not on its integer value: the loads stay global loads)
__device__ __forceinline__ StagedOperand staged_operand(const uint8_t* base, long long bytes) {
  const long long lo = static_cast<long long>(reinterpret_cast<uintptr_t>(base) & 3);
  return StagedOperand{base - lo, lo, lo + bytes};
}

// The tensor's first or last partial word, at word offset o: its bytes inside the tensor, the others 0.
__device__ __forceinline__ uint32_t staged_edge_word(const StagedOperand& op, long long o) {
  uint32_t v = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b)
    if (o + b >= op.lo && o + b < op.hi) v |= static_cast<uint32_t>(op.a0[o + b]) << (8 * b);
  return v;
}

// A staging thread's 16 bytes of one row: `off` = their offset from a0 in stage 0 (or < 0: the row lies outside the
// problem), kc = 16 * (thread & 3).
struct StagedChunk {
  long long off;
  int kc;
};

// the wanted bytes of the chunk in the stage that begins at k0: min(16, d - k0 - kc), none beyond the row's end
__device__ __forceinline__ int staged_len(const StagedChunk& c, long long d, int k0) {
  if (c.off < 0) return 0;
  const long long left = d - k0 - c.kc;
  return left >= 16 ? 16 : left > 0 ? static_cast<int>(left) : 0;
}

// raw[0 .. 4] = the aligned words that cover the chunk; a word without a wanted byte is not read (0).
__device__ __forceinline__ void staged_load(const StagedOperand& op, const StagedChunk& c, long long d, int k0,
                                            uint32_t (&raw)[5]) {
  const int len = staged_len(c, d, k0);
  const long long p = c.off + k0;
  const int sh = static_cast<int>(p & 3);
  const long long o0 = p - sh;
  if (len == 16 && o0 >= op.lo && o0 + 20 <= op.hi) {      // (the common case: five whole words inside the tensor)
#pragma unroll
    for (int j = 0; j < 5; ++j) raw[j] = *reinterpret_cast<const uint32_t*>(op.a0 + o0 + 4 * j);
    return;
  }
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const long long o = o0 + 4 * j;
    // word j holds the chunk's bytes [4 j - sh, 4 j + 4 - sh): wanted if that meets [0, len)
    if (len == 0 || 4 * j >= sh + len) raw[j] = 0;
    else if (o >= op.lo && o + 4 <= op.hi) raw[j] = *reinterpret_cast<const uint32_t*>(op.a0 + o);
    else raw[j] = staged_edge_word(op, o);
  }
}

// The chunk's 16 bytes, shifted into place, zero from byte `len` on.
__device__ __forceinline__ I32x4 staged_shift(const uint32_t (&raw)[5], int sh, int len) {
  I32x4 out;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t v = __builtin_amdgcn_alignbyte(raw[i + 1], raw[i], static_cast<uint32_t>(sh));
    const int keep = len - 4 * i;      // bytes of this word below d
    out[i] = static_cast<int>(keep >= 4 ? v : keep <= 0 ? 0u : v & ((1u << (8 * keep)) - 1u));
  }
  return out;
}

// acc = the wave's tile of Xq W^^T (w stored I8) for any d >= 1 and any alignment; see the head of the file.
// Every thread of the workgroup calls this, `own` or not.
__device__ __forceinline__ void qfc_staged_loop(const QfcWave& wv, bool own, const int8_t* xq, const uint8_t* w,
                                                long long n, long long rows, long long d,
                                                I32x4 (&acc)[QfcTile<int8_t>::TM][TB]) {
  using T = QfcTile<int8_t>;
  __shared__ __attribute__((aligned(16))) uint8_t lds[2][kStageRows * kPitch];

  const StagedOperand ox = staged_operand(reinterpret_cast<const uint8_t*>(xq), n * d), ow = staged_operand(w, rows * d);
  const int tid = threadIdx.x, wave = tid / kWave;
  StagedChunk ch[kStagePasses];
  int sh[kStagePasses];
#pragma unroll
  for (int q = 0; q < kStagePasses; ++q) {
    const bool is_x = q < kStagePasses / 2;
    const int local = (tid >> 2) + (q % (kStagePasses / 2)) * (kQfcThreads / 4);      // row of the operand's 128
    const long long row = is_x ? static_cast<long long>(blockIdx.y) * T::BTA + local
                               : static_cast<long long>(blockIdx.x) * T::BTB + local;
    const bool ok = row < (is_x ? n : rows);
    ch[q].kc = (tid & 3) * 16;
    ch[q].off = ok ? (is_x ? ox.lo : ow.lo) + row * d + ch[q].kc : -1;
    sh[q] = static_cast<int>(ch[q].off & 3);
  }
  // LDS rows 0 .. 127 hold xq, 128 .. 255 hold w; pass q stores row (tid >> 2) + 64 q
  const int store_at = (tid >> 2) * kPitch + (tid & 3) * 16;
  int xa[T::TA], wb[TB];      // the lane's fragment reads
#pragma unroll
  for (int a = 0; a < T::TA; ++a) xa[a] = ((wave >> 1) * T::WTA + a * MF + wv.fr) * kPitch + wv.fg * 16;
#pragma unroll
  for (int b = 0; b < TB; ++b) wb[b] = (T::BTA + (wave & 1) * T::WTB + b * MF + wv.fr) * kPitch + wv.fg * 16;

#pragma unroll
  for (int m = 0; m < T::TM; ++m)
#pragma unroll
    for (int b = 0; b < TB; ++b) acc[m][b] = I32x4{0, 0, 0, 0};

  uint32_t raw[kStagePasses][5];
  auto load = [&](int k0) {
#pragma unroll
    for (int q = 0; q < kStagePasses; ++q) staged_load(q < kStagePasses / 2 ? ox : ow, ch[q], d, k0, raw[q]);
  };
  auto store = [&](int k0, int buf) {
#pragma unroll
    for (int q = 0; q < kStagePasses; ++q)
      *reinterpret_cast<I32x4*>(&lds[buf][store_at + q * (kQfcThreads / 4) * kPitch]) =
          staged_shift(raw[q], sh[q], staged_len(ch[q], d, k0));
  };

  const int stages = static_cast<int>((d + kStageK - 1) / kStageK);
  load(0);
  store(0, 0);
  __syncthreads();
  for (int s = 0; s < stages; ++s) {
    const int buf = s & 1;
    const bool more = s + 1 < stages;
    if (more) load((s + 1) * kStageK);      // in flight while this stage's MFMAs run
    if (own) {
      I32x4 xf[T::TA], wf[TB];
#pragma unroll
      for (int a = 0; a < T::TA; ++a) xf[a] = *reinterpret_cast<const I32x4*>(&lds[buf][xa[a]]);
#pragma unroll
      for (int b = 0; b < TB; ++b) wf[b] = *reinterpret_cast<const I32x4*>(&lds[buf][wb[b]]);
#pragma unroll
      for (int a = 0; a < T::TA; ++a)
#pragma unroll
        for (int b = 0; b < TB; ++b) acc[a][b] = mfma_i8<kStageK>(xf[a], wf[b], acc[a][b]);
    }
    if (more) store((s + 1) * kStageK, buf ^ 1);
    __syncthreads();
  }
}

}  // namespace
}  // namespace mi355q
