// pinn_fused_wt.inc — launchers of the fused tile kernel with the point-weighted epilogue (fused_kernel.h, EPI_WEIGHTED: the
// residual epilogue with one weight per point and weighted term, and an optional store of the signed fields) for ONE padded
// hidden width: the includer defines FUSED_WP (16, 32 or 64).  K1 = 4 (Navier_Stokes) and K1 = 3 (physics_equation,
// continuity_ftemp, continuity_only), tanh, natural unit order: a forward-only instance, a gradient instance with the workgroup's gradient
// copy in LDS and one with it in global memory each.  Own translation units, so that the kernels of the other
// pinn_fused_*_wXX.hip are compiled exactly as before.
#include <type_traits>
#include "fused_kernel.h"

namespace pinn {

constexpr int WP_ = FUSED_WP;

template <class K>
static int wgo(K kern, const FusedParams& P, int grid, size_t lds, hipStream_t s, const char* what) {
  if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds)) return rc;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(FUSED_THREADS), lds, s, P);
  return check_launch(what);
}

template <int K1>
static int launch_wt_k(bool grad, const FusedParams& P, int grid, size_t lds, hipStream_t s, const char* what) {
  if (!grad) return wgo(k_fused<WP_, K1, false, false, PINN_ACT_TANH, EPI_WEIGHTED>, P, grid, lds, s, what);
  return P.acc_lds ? wgo(k_fused<WP_, K1, true, true, PINN_ACT_TANH, EPI_WEIGHTED>, P, grid, lds, s, what)
                   : wgo(k_fused<WP_, K1, true, false, PINN_ACT_TANH, EPI_WEIGHTED>, P, grid, lds, s, what);
}

template <>
int launch_fused_wt<WP_>(int K1, bool grad, const FusedParams& P, int grid, size_t lds, hipStream_t s) {
  const char* what = WP_ == 16 ? "fused kernel (WP=16, weighted residual)" : WP_ == 32 ? "fused kernel (WP=32, weighted residual)"
                                                                                           : "fused kernel (WP=64, weighted residual)";
  if (K1 == 4) return launch_wt_k<4>(grad, P, grid, lds, s, what);
  if (K1 == 3) return launch_wt_k<3>(grad, P, grid, lds, s, what);
  set_error("fused engine: no weighted kernel for k = %d", K1 - 1);
  return PINN_ERR_UNSUPPORTED;
}

}  // namespace pinn
