// pinn_fused_ens.inc — launchers of the fused tile kernel's ENSEMBLE instances (fused_kernel.h, k_fused_ens: a 2-D grid (gx, M),
// member = blockIdx.y, the single-network body behind one pointer shift) for ONE padded hidden width: the includer defines
// FUSED_WP (16, 32 or 64).  Gradient passes of tanh networks with the generic loss epilogue in natural unit order, K1 = 3 or
// 4, the workgroup's gradient copy in LDS or in global memory: four kernels per width.  Own translation units, so that the
// kernels of the other pinn_fused_*_wXX.hip are compiled exactly as before.
#include <type_traits>
#include "fused_kernel.h"

namespace pinn {

constexpr int WP_ = FUSED_WP;

template <class K>
static int ego(K kern, const FusedParams& P, int gx, int M, size_t lds, hipStream_t s) {
  if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds)) return rc;
  hipLaunchKernelGGL(kern, dim3(gx, M), dim3(FUSED_THREADS), lds, s, P);
  return check_launch(WP_ == 16 ? "fused kernel (WP=16, ensemble)" : WP_ == 32 ? "fused kernel (WP=32, ensemble)"
                                                                                 : "fused kernel (WP=64, ensemble)");
}

template <int K1>
static int launch_ens_k(const FusedParams& P, int gx, int M, size_t lds, hipStream_t s) {
  return P.acc_lds ? ego(k_fused_ens<WP_, K1, true>, P, gx, M, lds, s) : ego(k_fused_ens<WP_, K1, false>, P, gx, M, lds, s);
}

template <>
int launch_fused_ens<WP_>(int K1, const FusedParams& P, int gx, int M, size_t lds, hipStream_t s) {
  if (K1 == 3) return launch_ens_k<3>(P, gx, M, lds, s);
  if (K1 == 4) return launch_ens_k<4>(P, gx, M, lds, s);
  set_error("fused engine: no ensemble kernel for K1=%d", K1);
  return PINN_ERR_UNSUPPORTED;
}

}  // namespace pinn
