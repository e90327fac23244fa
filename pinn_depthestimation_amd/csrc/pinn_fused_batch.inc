// pinn_fused_batch.inc — launchers of the batch kernel (fused_batch_kernel.h) for ONE (padded width, K1): the includer
// defines BATCH_WP (16 / 32) and BATCH_K1 (3 / 4).  One translation unit per pair keeps the build parallel: every
// instance is a fully unrolled T-tile layer body.
// BATCH_EPI (optional) picks the epilogue: left undefined, the loss instances behind launch_fused_batch_k; defined as
// EPI_ADJ (pinn_fused_batch_adj_w*_k*.hip), the external-adjoint instances of pinn_jet_backward behind
// launch_fused_batch_adj_k.  Own translation units, so that the loss instances are compiled exactly as before.
#include <type_traits>
#include "fused_batch_kernel.h"

// An includer that sets BATCH_EPI to anything else (EPI_PEC: pinn_fused_batch_pec_w*_k3.hip, launch_fused_batch_pec_k) names
// its launcher and its launch-error text itself: BATCH_LAUNCH, BATCH_WHAT.
#ifndef BATCH_EPI
#define BATCH_EPI EPI_GENERIC
#define BATCH_LAUNCH launch_fused_batch_k
#define BATCH_WHAT "fused batch kernel"
#elif !defined(BATCH_LAUNCH)
#define BATCH_LAUNCH launch_fused_batch_adj_k
#define BATCH_WHAT "fused batch kernel (external adjoint)"
#endif

namespace pinn {

namespace {

template <int KS, int KS0, int SINK, int T>
int bgo_t(const FusedParams& P, int grid, size_t lds, hipStream_t s) {
  auto kern = k_fused_batch<BATCH_WP, KS, KS0, BATCH_K1, T, SINK, PINN_ACT_TANH, BATCH_EPI>;
  if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds)) return rc;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(BATCH_THREADS), lds, s, P);
  return check_launch(BATCH_WHAT);
}
// two batch sizes per instance: the register-filling one for large point sets, ONE tile per wave for small ones
// (P.batch_T, chosen by the host from the tile count: the latency of a layer step scales with T)
template <int KS, int KS0, int SINK>
int bgo(const FusedParams& P, int grid, size_t lds, hipStream_t s) {
  return P.batch_T == 1 ? bgo_t<KS, KS0, SINK, 1>(P, grid, lds, s)
                        : bgo_t<KS, KS0, SINK, batch_tiles(BATCH_WP, BATCH_K1)>(P, grid, lds, s);
}
template <int KS>
int bgo_ks(int d_in, const FusedParams& P, int grid, size_t lds, hipStream_t s) {
  if (d_in <= 4) return P.acc_lds ? bgo<KS, 1, BSINK_LDS_WAVE>(P, grid, lds, s) : bgo<KS, 1, BSINK_ATOMIC>(P, grid, lds, s);
  return P.acc_lds ? bgo<KS, 2, BSINK_LDS_WAVE>(P, grid, lds, s) : bgo<KS, 2, BSINK_ATOMIC>(P, grid, lds, s);
}

}  // namespace

template <int WP, int K1>
int BATCH_LAUNCH(int W, int d_in, const FusedParams& P, int grid, size_t lds, hipStream_t s);

template <>
int BATCH_LAUNCH<BATCH_WP, BATCH_K1>(int W, int d_in, const FusedParams& P, int grid, size_t lds, hipStream_t s) {
  constexpr int KS_LO = BATCH_WP == 16 ? 3 : 5, KS_HI = BATCH_WP == 16 ? 4 : 8;
  return (W + 3) / 4 <= KS_LO ? bgo_ks<KS_LO>(d_in, P, grid, lds, s) : bgo_ks<KS_HI>(d_in, P, grid, lds, s);
}

}  // namespace pinn
