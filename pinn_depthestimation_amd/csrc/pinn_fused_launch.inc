// pinn_fused_launch.inc — launchers of the fused MFMA chain kernel (fused_kernel.h) for ONE padded hidden width: the
// includer defines FUSED_WP (16, 32 or 64).  One translation unit per width because the Makefile gives each its own
// compiler flags.  Width 64 adds the residual-only gradient kernels with a specialised epilogue.
#include <type_traits>
#include "fused_kernel.h"

namespace pinn {

constexpr int WP_ = FUSED_WP;

template <class K>
static int fgo(K kern, const FusedParams& P, int grid, size_t lds, hipStream_t s, const char* what) {
  if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds)) return rc;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(FUSED_THREADS), lds, s, P);
  return check_launch(what);
}

template <int K1, bool GRAD, bool LDSACC, int ACT>
static int launch_one_act(const FusedParams& P, int grid, size_t lds, hipStream_t s) {
  return fgo(k_fused<WP_, K1, GRAD, LDSACC, ACT>, P, grid, lds, s,
             WP_ == 16 ? "fused kernel (WP=16)" : WP_ == 32 ? "fused kernel (WP=32)" : "fused kernel (WP=64)");
}

// residual-only gradient kernels with the epilogue specialised to one residual family (fused_kernel.h, EPI)
template <int K1, int EPI>
static int launch_special(const FusedParams& P, int grid, size_t lds, hipStream_t s) {
  // k-step-major inputs / outputs (fused_kernel.h, KRO): ceil(d_out / 4) k-steps in the output layer's reverse GEMM
  constexpr int KRO = EPI == EPI_PE ? 2 : 1;
  return fgo(k_fused<WP_, K1, true, true, PINN_ACT_TANH, EPI, KRO>, P, grid, lds, s,
             "fused kernel (WP=64, specialised epilogue)");
}

template <int K1, bool GRAD, bool LDSACC>
static int launch_one(const FusedParams& P, int grid, size_t lds, hipStream_t s) {
  if constexpr (WP_ == 64 && GRAD && LDSACC && K1 >= 3) {
    if (P.io1) {   // (pinn_fused.hip decides: tanh, residual only, no outputs wanted, d_in <= 4, d_out within the epilogue's k-steps)
      if constexpr (K1 == 4) {
        if (P.residual_id == PINN_RES_NAVIER_STOKES) return launch_special<4, EPI_NS>(P, grid, lds, s);
      }
      if constexpr (K1 == 3) {
        if (P.residual_id == PINN_RES_PHYSICS_EQUATION) return launch_special<3, EPI_PE>(P, grid, lds, s);
        if (P.residual_id == PINN_RES_CONTINUITY_ONLY || P.residual_id == PINN_RES_CONTINUITY_FTEMP)
          return launch_special<3, EPI_CONT>(P, grid, lds, s);
      }
    }
  }
  // (never a tanh or LeakyReLU kernel on anything else: the sine first layer has launchers of its own, pinn_fused_sin.inc)
  if (P.act != PINN_ACT_TANH && P.act != PINN_ACT_LEAKY_RELU) { set_error("fused engine: no kernel for activation %d here", P.act); return PINN_ERR_UNSUPPORTED; }
  return P.act == PINN_ACT_TANH ? launch_one_act<K1, GRAD, LDSACC, PINN_ACT_TANH>(P, grid, lds, s)
                                : launch_one_act<K1, GRAD, LDSACC, PINN_ACT_LEAKY_RELU>(P, grid, lds, s);
}

template <>
int launch_fused<WP_>(int K1, bool grad, const FusedParams& P, int grid, size_t lds, hipStream_t s) {
  if (!grad) {
    switch (K1) {
      case 1: return launch_one<1, false, false>(P, grid, lds, s);
      case 2: return launch_one<2, false, false>(P, grid, lds, s);
      case 3: return launch_one<3, false, false>(P, grid, lds, s);
      case 4: return launch_one<4, false, false>(P, grid, lds, s);
    }
  } else {
    switch (K1) {
      case 1: return P.acc_lds ? launch_one<1, true, true>(P, grid, lds, s) : launch_one<1, true, false>(P, grid, lds, s);
      case 3: return P.acc_lds ? launch_one<3, true, true>(P, grid, lds, s) : launch_one<3, true, false>(P, grid, lds, s);
      case 4: return P.acc_lds ? launch_one<4, true, true>(P, grid, lds, s) : launch_one<4, true, false>(P, grid, lds, s);
    }
  }
  set_error("fused engine: no kernel for K1=%d grad=%d", K1, (int)grad);
  return PINN_ERR_UNSUPPORTED;
}

}  // namespace pinn
