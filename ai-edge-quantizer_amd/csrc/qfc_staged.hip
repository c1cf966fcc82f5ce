// The staged MFMA route of mi355q_qfc_forward_i8 and mi355q_qfc_output_i8 (include/mi355q.h, "Staged route"): a
// stored I8 weight with per-tensor or per-channel scales at any reduction length and any byte alignment of xq and w.
//
//   qfc_staged_kernel      qfc_staged.h's main loop (both operands through LDS, zero beyond d, n and rows) into the
//                          float rescale of qfc.hip's kernel;
//   qfc_out_staged_kernel  the same loop into the fixed-point epilogue of qfc_out.hip's kernel.
// Both epilogues are qfc_tile_out.h's, one piece of code each with the aligned route, on the same exact integers: the
// outputs are the aligned and the generic kernels' bit for bit. Every wave of a workgroup runs the loop (it holds the
// barriers); a wave without a tile leaves after it.
//
// As the compiler reports them for gfx950: 136 VGPRs, no scratch, 40960 bytes of LDS, so two workgroups fit a CU's LDS
// and registers allow three waves per SIMD.
//
// The host side here is the routing of the three routes: mi355q_qfc_route, and the switch that takes this one away.
#include <atomic>

#include "common.h"
#include "compare_target.h"
#include "qfc_staged.h"
#include "qfc_tile_out.h"

namespace mi355q {
namespace {

__global__ __launch_bounds__(kQfcThreads) void qfc_staged_kernel(FwdArgs g) {
  QfcWave wv;
  const bool own = qfc_wave<int8_t>(wv, g.n, g.rows);
  I32x4 acc[QfcTile<int8_t>::TM][TB];
  qfc_staged_loop(wv, own, g.xq, g.w, g.n, g.rows, g.d, acc);
  if (!own) return;
  qfc_store_float(g, wv, acc);
}

__global__ __launch_bounds__(kQfcThreads) void qfc_out_staged_kernel(OutArgs g) {
  QfcWave wv;
  const bool own = qfc_wave<int8_t>(wv, g.n, g.rows);
  I32x4 acc[QfcTile<int8_t>::TM][TB];
  qfc_staged_loop(wv, own, static_cast<const int8_t*>(g.xq), g.w, g.n, g.rows, g.d, acc);
  if (!own) return;
  qfc_store_output8(g, wv, acc);
}

std::atomic<int> g_staged{1};

}  // namespace

void launch_qfc_staged(const FwdArgs& g, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL(qfc_staged_kernel, grid, dim3(kQfcThreads), 0, st, g);
}

void launch_qfc_out_staged(const OutArgs& g, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL(qfc_out_staged_kernel, grid, dim3(kQfcThreads), 0, st, g);
}

}  // namespace mi355q

using namespace mi355q;

// (a switch and a query, not statuses: int64_t, as mi355q_qbmm_mfma_route is)
extern "C" int64_t mi355q_qfc_set_staged(int32_t enabled) { return g_staged.exchange(enabled ? 1 : 0); }

extern "C" int64_t mi355q_qfc_route(const void* xq, const void* w, int64_t d, int32_t w_kind, int32_t block,
                                    int32_t blockwise) {
  if (d < 1) return MI355Q_QFC_ROUTE_GENERIC;      // (refused or empty: nothing is launched)
  if (mfma_route(xq, w, d, blockwise && block == 32 ? 32 : 64)) return MI355Q_QFC_ROUTE_MFMA;
  if (d <= kQfcMaxD && w_kind == MI355Q_CMP_I8 && !blockwise && g_staged.load()) return MI355Q_QFC_ROUTE_STAGED;
  return MI355Q_QFC_ROUTE_GENERIC;
}
