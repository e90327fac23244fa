// pinn_fused_sin.inc — launchers of the fused tile kernel for networks with a sine first layer (fused_kernel.h,
// PINN_ACT_SIN_TANH: a_1 = sin(W_0 x + b_0), tanh on the other hidden layers) for ONE padded hidden width: the includer defines
// FUSED_WP (16, 32 or 64).  Generic epilogue, natural unit order, no dropout; K1 = 1, 3 and 4: a forward-only instance, a
// gradient instance with the workgroup's gradient copy in LDS and one with it in global memory each.  Own translation
// units, so that the kernels of the other pinn_fused_*_wXX.hip are compiled exactly as before.
#include <type_traits>
#include "fused_kernel.h"

namespace pinn {

constexpr int WP_ = FUSED_WP;

#if FUSED_WP == 64
// (this one instance is compiled in pinn_fused_sin_w64_g4.hip, without -amdgpu-mfma-vgpr-form: see there)
extern template __global__ void k_fused<64, 4, true, false, PINN_ACT_SIN_TANH, EPI_GENERIC>(const FusedParams);
#endif

template <class K>
static int sgo(K kern, const FusedParams& P, int grid, size_t lds, hipStream_t s, const char* what) {
  if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds)) return rc;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(FUSED_THREADS), lds, s, P);
  return check_launch(what);
}

template <int K1>
static int launch_sin_k(bool grad, const FusedParams& P, int grid, size_t lds, hipStream_t s, const char* what) {
  if (!grad) return sgo(k_fused<WP_, K1, false, false, PINN_ACT_SIN_TANH, EPI_GENERIC>, P, grid, lds, s, what);
  return P.acc_lds ? sgo(k_fused<WP_, K1, true, true, PINN_ACT_SIN_TANH, EPI_GENERIC>, P, grid, lds, s, what)
                   : sgo(k_fused<WP_, K1, true, false, PINN_ACT_SIN_TANH, EPI_GENERIC>, P, grid, lds, s, what);
}

template <>
int launch_fused_sin<WP_>(int K1, bool grad, const FusedParams& P, int grid, size_t lds, hipStream_t s) {
  const char* what = WP_ == 16 ? "fused kernel (WP=16, sine first layer)" : WP_ == 32 ? "fused kernel (WP=32, sine first layer)"
                                                                                       : "fused kernel (WP=64, sine first layer)";
  if (P.act != PINN_ACT_SIN_TANH) { set_error("fused engine: the sine instances serve activation 2 only (got %d)", P.act); return PINN_ERR_UNSUPPORTED; }
  if (K1 == 4) return launch_sin_k<4>(grad, P, grid, lds, s, what);
  if (K1 == 3) return launch_sin_k<3>(grad, P, grid, lds, s, what);
  if (K1 == 1) return launch_sin_k<1>(grad, P, grid, lds, s, what);
  set_error("fused engine: no sine-first-layer kernel for k = %d", K1 - 1);
  return PINN_ERR_UNSUPPORTED;
}

}  // namespace pinn
