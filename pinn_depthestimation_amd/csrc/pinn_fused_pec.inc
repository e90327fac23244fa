// pinn_fused_pec.inc — launchers of the fused tile kernel with the corrected-radiation-stress epilogues (fused_kernel.h,
// EPI_PEC: the loss epilogue with ResPhysicsEquationCorrected; EPI_FIELD_PEC: its per-point fields) for ONE padded hidden
// width: the includer defines FUSED_WP (16, 32 or 64).  K1 = 3, tanh, natural unit order: a forward-only loss instance, a
// gradient instance with the workgroup's gradient copy in LDS, one with it in global memory, and a forward-only field
// instance.  Own translation units, so that the kernels of the other pinn_fused_*_wXX.hip are compiled exactly as before.
#include <type_traits>
#include "fused_kernel.h"

namespace pinn {

constexpr int WP_ = FUSED_WP;

template <class K>
static int pgo(K kern, const FusedParams& P, int grid, size_t lds, hipStream_t s, const char* what) {
  if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds)) return rc;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(FUSED_THREADS), lds, s, P);
  return check_launch(what);
}

template <>
int launch_fused_pec<WP_>(bool grad, const FusedParams& P, int grid, size_t lds, hipStream_t s) {
  const char* what = WP_ == 16 ? "fused kernel (WP=16, corrected residual)" : WP_ == 32 ? "fused kernel (WP=32, corrected residual)"
                                                                                         : "fused kernel (WP=64, corrected residual)";
  if (!grad) return pgo(k_fused<WP_, 3, false, false, PINN_ACT_TANH, EPI_PEC>, P, grid, lds, s, what);
  return P.acc_lds ? pgo(k_fused<WP_, 3, true, true, PINN_ACT_TANH, EPI_PEC>, P, grid, lds, s, what)
                   : pgo(k_fused<WP_, 3, true, false, PINN_ACT_TANH, EPI_PEC>, P, grid, lds, s, what);
}

template <>
int launch_fused_field_pec<WP_>(const FusedParams& P, int grid, size_t lds, hipStream_t s) {
  return pgo(k_fused<WP_, 3, false, false, PINN_ACT_TANH, EPI_FIELD_PEC>, P, grid, lds, s,
             WP_ == 16 ? "fused kernel (WP=16, corrected fields)" : WP_ == 32 ? "fused kernel (WP=32, corrected fields)"
                                                                             : "fused kernel (WP=64, corrected fields)");
}

}  // namespace pinn
