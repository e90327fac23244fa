// pinn_fused_adj.inc — launchers of the fused tile kernel with the external-adjoint epilogue (fused_kernel.h, EPI_ADJ:
// pinn_jet_backward on the MFMA path) for ONE padded hidden width: the includer defines FUSED_WP (16, 32 or 64).  Own
// translation units, so that the kernels of pinn_fused_wXX.hip are compiled exactly as before.
#include <type_traits>
#include "fused_kernel.h"

namespace pinn {

constexpr int WP_ = FUSED_WP;

template <int K1, bool LDSACC, int ACT>
static int launch_adj_act(const FusedParams& P, int grid, size_t lds, hipStream_t s) {
  auto kern = k_fused<WP_, K1, true, LDSACC, ACT, EPI_ADJ>;
  if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds)) return rc;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(FUSED_THREADS), lds, s, P);
  return check_launch(WP_ == 16 ? "fused kernel (WP=16, external adjoint)" : WP_ == 32 ? "fused kernel (WP=32, external adjoint)"
                                                                                      : "fused kernel (WP=64, external adjoint)");
}

template <int K1>
static int launch_adj(const FusedParams& P, int grid, size_t lds, hipStream_t s) {
  if (P.act == PINN_ACT_TANH)
    return P.acc_lds ? launch_adj_act<K1, true, PINN_ACT_TANH>(P, grid, lds, s) : launch_adj_act<K1, false, PINN_ACT_TANH>(P, grid, lds, s);
  return P.acc_lds ? launch_adj_act<K1, true, PINN_ACT_LEAKY_RELU>(P, grid, lds, s)
                   : launch_adj_act<K1, false, PINN_ACT_LEAKY_RELU>(P, grid, lds, s);
}

template <>
int launch_fused_adj<WP_>(int K1, const FusedParams& P, int grid, size_t lds, hipStream_t s) {
  switch (K1) {
    case 1: return launch_adj<1>(P, grid, lds, s);
    case 3: return launch_adj<3>(P, grid, lds, s);
    case 4: return launch_adj<4>(P, grid, lds, s);
  }
  set_error("fused engine: no external-adjoint kernel for K1=%d", K1);
  return PINN_ERR_UNSUPPORTED;
}

}  // namespace pinn
