// pinn_fused_batch.hip — every instance of the batch kernel (fused_batch_kernel.h: k_fused_batch) and its launcher.  Compiled
// once per translation unit, the unit named on the command line (Makefile): -DUNIT_<family> -DBATCH_WP=<16|32> -DBATCH_K1=<3|4>.
// One unit per (family, padded width, K1) keeps the build parallel — every instance is a fully unrolled T-tile layer body —
// and leaves the instances of the other families compiled exactly as before.  The families differ in the epilogue only;
// the entry point is batch_unit<family, WP, K1> (fused_launch.h).
#include "fused_launch.h"
#include "fused_batch_kernel.h"

namespace pinn {

#if defined(UNIT_loss)     // BF_LOSS: the loss instances
#define BATCH_FAMILY BF_LOSS
#define BATCH_EPI EPI_GENERIC
#define BATCH_WHAT "fused batch kernel"
#elif defined(UNIT_adj)    // BF_ADJ: the external-adjoint instances of pinn_jet_backward
#define BATCH_FAMILY BF_ADJ
#define BATCH_EPI EPI_ADJ
#define BATCH_WHAT "fused batch kernel (external adjoint)"
#elif defined(UNIT_pec)    // BF_PEC: the corrected-radiation-stress loss instances (K1 = 3)
#define BATCH_FAMILY BF_PEC
#define BATCH_EPI EPI_PEC
#define BATCH_WHAT "fused batch kernel (corrected residual)"
#else
#error "pinn_fused_batch.hip: name the unit, -DUNIT_<family> (Makefile, BATCH_UNITS)"
#endif

namespace {

// two batch sizes per instance: the register-filling one for large point sets, ONE tile per wave for small ones
// (P.batch_T, chosen by the host from the tile count: the latency of a layer step scales with T)
template <int KS, int KS0, int SINK>
int bgo(const BatchLaunch& a) {
  constexpr int T = batch_tiles(BATCH_WP, BATCH_K1);
  return a.P.batch_T == 1
             ? launch_kernel(k_fused_batch<BATCH_WP, KS, KS0, BATCH_K1, 1, SINK, PINN_ACT_TANH, BATCH_EPI>, dim3(a.grid), BATCH_THREADS, a.lds_bytes, a.s, BATCH_WHAT, a.P)
             : launch_kernel(k_fused_batch<BATCH_WP, KS, KS0, BATCH_K1, T, SINK, PINN_ACT_TANH, BATCH_EPI>, dim3(a.grid), BATCH_THREADS, a.lds_bytes, a.s, BATCH_WHAT, a.P);
}
// KS0 = 1 or 2 first-layer k-steps (d_in <= 4 or not); a gradient copy per wave in LDS, or atomics into shared copies
template <int KS>
int bgo_ks(const BatchLaunch& a) {
  if (a.d_in <= 4) return a.P.acc_lds ? bgo<KS, 1, BSINK_LDS_WAVE>(a) : bgo<KS, 1, BSINK_ATOMIC>(a);
  return a.P.acc_lds ? bgo<KS, 2, BSINK_LDS_WAVE>(a) : bgo<KS, 2, BSINK_ATOMIC>(a);
}

}  // namespace

template <>
int batch_unit<BATCH_FAMILY, BATCH_WP, BATCH_K1>(const BatchLaunch& a) {
  constexpr int KS_LO = BATCH_WP == 16 ? 3 : 5, KS_HI = BATCH_WP == 16 ? 4 : 8;   // hidden-layer k-steps: ceil(W / 4) rounded up to an instance
  return (a.W + 3) / 4 <= KS_LO ? bgo_ks<KS_LO>(a) : bgo_ks<KS_HI>(a);
}

}  // namespace pinn
