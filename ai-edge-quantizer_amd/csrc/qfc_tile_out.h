// What the int8 MFMA kernels do with a finished accumulator tile, once for both main loops: qfc.hip and qfc_out.hip
// (qfc_main_loop: fragments straight from global memory) and qfc_staged.hip (qfc_staged_loop: operands staged through
// LDS) run these on the same integers and so store the same bits.
//   qfc_store_float    the float rescale of mi355q_qfc_forward_i8 with per-tensor / per-channel scales (and acc_out);
//   qfc_store_output8  the fixed-point epilogue of mi355q_qfc_output_i8 (qfc_epilogue.h's output8) and its int8 store.
// Also the argument block of the forward kernels and the staged launches that qfc.hip and qfc_out.hip call.
#pragma once

#include "qfc_epilogue.h"
#include "qfc_tile.h"

namespace mi355q {

struct FwdArgs {
  const int8_t* xq;        // [n, d]
  const uint8_t* w;        // [rows, d] stored
  const float* x_scale;    // 1 or n
  const float* w_scale;    // 1, rows or rows * nblocks
  const int32_t* wsum;     // [rows, nblocks] (read only when zp != 0)
  float* y;                // [n, rows]
  int32_t* acc;            // [n, rows] or null
  long long n, rows, d;
  int x_per_row;           // x_scale has n entries
  int w_mode;              // 0 per tensor, 1 per channel, 2 blockwise
  int nblocks;             // blocks per weight row (1 unless blockwise)
  int block;               // elements per block (d unless blockwise)
  int zp;
  int kind;
};

// qfc_staged.hip: the staged kernels on tile_grid<int8_t>'s grid (the callers check the launch)
void launch_qfc_staged(const FwdArgs& g, dim3 grid, hipStream_t st);
void launch_qfc_out_staged(const OutArgs& g, dim3 grid, hipStream_t st);

namespace {

struct ChanF {
  float sw;      // the channel's weight scale
  int corr;      // zp * Sum_k q_w[r][k]
};

// y = float(acc - zp * wsum) * (s_x * s_w), and acc_out (not blockwise)
__device__ __forceinline__ void qfc_store_float(const FwdArgs& g, const QfcWave& wv,
                                                const I32x4 (&acc)[QfcTile<int8_t>::TM][TB]) {
  qfc_walk_outputs<int8_t>(
      wv, g.n, g.rows,
      [=](long long r) { return ChanF{g.w_scale[g.w_mode == 1 ? r : 0], g.zp != 0 ? g.zp * g.wsum[r] : 0}; },
      [=, &acc](const ChanF& c, int a, int b, int i, long long t, long long r) {
        const int v = acc[a][b][i] - c.corr;
        const float sc = g.x_scale[g.x_per_row ? t : 0] * c.sw;
        g.y[t * g.rows + r] = static_cast<float>(v) * sc;
        if (g.acc) g.acc[t * g.rows + r] = v;
      });
}

// q = output8(acc - zp_x * wsum)
__device__ __forceinline__ void qfc_store_output8(const OutArgs& g, const QfcWave& wv,
                                                  const I32x4 (&acc)[QfcTile<int8_t>::TM][TB]) {
  struct Chan {
    Chan8 c;
    int corr;      // zp_x * Sum_k q_w[r][k]
  };
  int8_t* q = static_cast<int8_t*>(g.q);
  qfc_walk_outputs<int8_t>(
      wv, g.n, g.rows, [=](long long r) { return Chan{chan8(g, r), g.zp_x != 0 ? g.zp_x * g.wsum[r] : 0}; },
      [=, &acc](const Chan& c, int a, int b, int i, long long t, long long r) {
        q[t * g.rows + r] = output8(acc[a][b][i] - c.corr, c.c, g);
      });
}

}  // namespace
}  // namespace mi355q
