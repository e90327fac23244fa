// pinn_fused_field.inc — launchers of the fused tile kernel with the field epilogue (fused_kernel.h, EPI_FIELD:
// pinn_residual_fields on the MFMA path) for ONE padded hidden width: the includer defines FUSED_WP (16, 32 or 64).
// Forward-only instances, K1 = 3 or 4 (1 + the residual's directions), tanh or LeakyReLU.  Own translation units, so
// that the kernels of pinn_fused_wXX.hip and pinn_fused_adj_wXX.hip are compiled exactly as before.
#include <type_traits>
#include "fused_kernel.h"

namespace pinn {

constexpr int WP_ = FUSED_WP;

template <int K1, int ACT>
static int launch_field_act(const FusedParams& P, int grid, size_t lds, hipStream_t s) {
  auto kern = k_fused<WP_, K1, false, false, ACT, EPI_FIELD>;
  if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds)) return rc;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(FUSED_THREADS), lds, s, P);
  return check_launch(WP_ == 16 ? "fused kernel (WP=16, fields)" : WP_ == 32 ? "fused kernel (WP=32, fields)" : "fused kernel (WP=64, fields)");
}

template <int K1>
static int launch_field(const FusedParams& P, int grid, size_t lds, hipStream_t s) {
  return P.act == PINN_ACT_TANH ? launch_field_act<K1, PINN_ACT_TANH>(P, grid, lds, s)
                                : launch_field_act<K1, PINN_ACT_LEAKY_RELU>(P, grid, lds, s);
}

template <>
int launch_fused_field<WP_>(int K1, const FusedParams& P, int grid, size_t lds, hipStream_t s) {
  switch (K1) {
    case 3: return launch_field<3>(P, grid, lds, s);
    case 4: return launch_field<4>(P, grid, lds, s);
  }
  set_error("fused engine: no field kernel for K1=%d", K1);
  return PINN_ERR_UNSUPPORTED;
}

}  // namespace pinn
