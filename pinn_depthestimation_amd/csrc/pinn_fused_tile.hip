// pinn_fused_tile.hip — every instance of the fused tile kernel (fused_kernel.h: k_fused, k_fused_ens) and its launcher.
// Compiled once per translation unit, the unit named on the command line (Makefile): -DUNIT_<family> -DFUSED_WP=<16|32|64>.
// One unit per (family, padded width) because the Makefile gives the units their own compiler flags, and so that a new
// family leaves the kernels of the others compiled exactly as before.  Each family below is one block: which instances
// exist, and how the run-time arguments pick one (K1, gradient or not, the workgroup's gradient copy in LDS or in global
// memory, the activation; io1 + residual for the width-64 specialised epilogues).  Its entry point is tile_unit<family, WP>
// (fused_launch.h); a K1 without an instance is refused here.
#include "fused_launch.h"

namespace pinn {

namespace {

constexpr int WP_ = FUSED_WP;

// the label a failed launch is reported under: "fused kernel (WP=16)", "fused kernel (WP=64, fields)", ...
#define STR_(x) #x
#define STR(x) STR_(x)
#define WHAT(tail) "fused kernel (WP=" STR(FUSED_WP) tail ")"

template <class K>
int go(K kern, const TileLaunch& a, const char* what) {
  return launch_kernel(kern, a.grid, FUSED_THREADS, a.lds_bytes, a.s, what, a.P);
}
// a forward-only instance
template <int K1, int ACT, int EPI>
int fwd(const TileLaunch& a, const char* what) {
  return go(k_fused<WP_, K1, false, false, ACT, EPI>, a, what);
}
// a gradient instance with the workgroup's gradient copy in LDS and one with it in global memory
template <int K1, int ACT, int EPI>
int bwd(const TileLaunch& a, const char* what) {
  return a.P.acc_lds ? go(k_fused<WP_, K1, true, true, ACT, EPI>, a, what) : go(k_fused<WP_, K1, true, false, ACT, EPI>, a, what);
}
// ... all three
template <int K1, int ACT, int EPI>
int fwd_or_bwd(const TileLaunch& a, const char* what) {
  return a.grad ? bwd<K1, ACT, EPI>(a, what) : fwd<K1, ACT, EPI>(a, what);
}

}  // namespace

#if defined(UNIT_loss)
// TF_LOSS — generic epilogue, tanh and LeakyReLU: forward K1 = 1..4, gradient K1 = 1, 3, 4.  Width 64 adds the residual-only
// gradient kernels with the epilogue specialised to one residual family (fused_kernel.h, EPI), gradient copy in LDS.
template <int K1, int EPI>
static int special(const TileLaunch& a) {
  // k-step-major inputs / outputs (fused_kernel.h, KRO): ceil(d_out / 4) k-steps in the output layer's reverse GEMM
  constexpr int KRO = EPI == EPI_PE ? 2 : 1;
  return go(k_fused<WP_, K1, true, true, PINN_ACT_TANH, EPI, KRO>, a, "fused kernel (WP=64, specialised epilogue)");
}
template <int K1, bool GRAD>
static int loss_k(const TileLaunch& a) {
  const FusedParams& P = a.P;
  if constexpr (WP_ == 64 && GRAD && K1 >= 3) {
    if (P.acc_lds && P.io1) {   // (pinn_fused.hip decides: tanh, residual only, no outputs wanted, d_in <= 4, d_out within the epilogue's k-steps)
      if constexpr (K1 == 4) {
        if (P.residual_id == PINN_RES_NAVIER_STOKES) return special<4, EPI_NS>(a);
      }
      if constexpr (K1 == 3) {
        if (P.residual_id == PINN_RES_PHYSICS_EQUATION) return special<3, EPI_PE>(a);
        if (P.residual_id == PINN_RES_CONTINUITY_ONLY || P.residual_id == PINN_RES_CONTINUITY_FTEMP) return special<3, EPI_CONT>(a);
      }
    }
  }
  // (never a tanh or LeakyReLU kernel on anything else: the sine first layer has a family of its own, TF_SIN)
  if (P.act != PINN_ACT_TANH && P.act != PINN_ACT_LEAKY_RELU) { set_error("fused engine: no kernel for activation %d here", P.act); return PINN_ERR_UNSUPPORTED; }
  if constexpr (GRAD)
    return P.act == PINN_ACT_TANH ? bwd<K1, PINN_ACT_TANH, EPI_GENERIC>(a, WHAT("")) : bwd<K1, PINN_ACT_LEAKY_RELU, EPI_GENERIC>(a, WHAT(""));
  else
    return P.act == PINN_ACT_TANH ? fwd<K1, PINN_ACT_TANH, EPI_GENERIC>(a, WHAT("")) : fwd<K1, PINN_ACT_LEAKY_RELU, EPI_GENERIC>(a, WHAT(""));
}
template <>
int tile_unit<TF_LOSS, WP_>(const TileLaunch& a) {
  const int rc = a.grad ? with_k1<1, 3, 4>(a.K1, [&](auto k) { return loss_k<decltype(k)::value, true>(a); })
                        : with_k1<1, 2, 3, 4>(a.K1, [&](auto k) { return loss_k<decltype(k)::value, false>(a); });
  if (rc != NO_INSTANCE) return rc;
  set_error("fused engine: no kernel for K1=%d grad=%d", a.K1, (int)a.grad);
  return PINN_ERR_UNSUPPORTED;
}

#elif defined(UNIT_adj)
// TF_ADJ — external-adjoint epilogue (EPI_ADJ: pinn_jet_backward on the MFMA path): gradient passes, K1 = 1, 3, 4, tanh and
// LeakyReLU.
template <>
int tile_unit<TF_ADJ, WP_>(const TileLaunch& a) {
  const int rc = with_k1<1, 3, 4>(a.K1, [&](auto k) {
    constexpr int K1 = decltype(k)::value;
    return a.P.act == PINN_ACT_TANH ? bwd<K1, PINN_ACT_TANH, EPI_ADJ>(a, WHAT(", external adjoint"))
                                    : bwd<K1, PINN_ACT_LEAKY_RELU, EPI_ADJ>(a, WHAT(", external adjoint"));
  });
  if (rc != NO_INSTANCE) return rc;
  set_error("fused engine: no external-adjoint kernel for K1=%d", a.K1);
  return PINN_ERR_UNSUPPORTED;
}

#elif defined(UNIT_field)
// TF_FIELD — field epilogue (EPI_FIELD: pinn_residual_fields on the MFMA path): forward only, K1 = 3 or 4 (1 + the
// residual's directions), tanh and LeakyReLU.
template <>
int tile_unit<TF_FIELD, WP_>(const TileLaunch& a) {
  const int rc = with_k1<3, 4>(a.K1, [&](auto k) {
    constexpr int K1 = decltype(k)::value;
    return a.P.act == PINN_ACT_TANH ? fwd<K1, PINN_ACT_TANH, EPI_FIELD>(a, WHAT(", fields")) : fwd<K1, PINN_ACT_LEAKY_RELU, EPI_FIELD>(a, WHAT(", fields"));
  });
  if (rc != NO_INSTANCE) return rc;
  set_error("fused engine: no field kernel for K1=%d", a.K1);
  return PINN_ERR_UNSUPPORTED;
}

#elif defined(UNIT_pec)
// TF_PEC, TF_FIELD_PEC — corrected-radiation-stress epilogues (EPI_PEC: the loss epilogue with ResPhysicsEquationCorrected;
// EPI_FIELD_PEC: its per-point fields): K1 = 3, tanh; forward, gradient (LDS / global copy), and a forward-only field instance.
template <>
int tile_unit<TF_PEC, WP_>(const TileLaunch& a) {
  return fwd_or_bwd<3, PINN_ACT_TANH, EPI_PEC>(a, WHAT(", corrected residual"));
}
template <>
int tile_unit<TF_FIELD_PEC, WP_>(const TileLaunch& a) {
  return fwd<3, PINN_ACT_TANH, EPI_FIELD_PEC>(a, WHAT(", corrected fields"));
}

#elif defined(UNIT_wave)
// TF_WAVE, TF_FIELD_WAVE — wave-closure epilogues (EPI_WAVE: the corrected residual's loss epilogue with
// ResPhysicsEquationWave, five terms; EPI_FIELD_WAVE: its per-point fields): the instances of the pec units, K1 = 3, tanh;
// forward, gradient (LDS / global copy), and a forward-only field instance.
template <>
int tile_unit<TF_WAVE, WP_>(const TileLaunch& a) {
  return fwd_or_bwd<3, PINN_ACT_TANH, EPI_WAVE>(a, WHAT(", wave closure"));
}
template <>
int tile_unit<TF_FIELD_WAVE, WP_>(const TileLaunch& a) {
  return fwd<3, PINN_ACT_TANH, EPI_FIELD_WAVE>(a, WHAT(", wave-closure fields"));
}

#elif defined(UNIT_coef)
// TF_COEF — runtime-coefficient epilogue (EPI_COEF: the EPI_NS / EPI_PE epilogue with gamma_b resp. Cd read from a device
// array and the coefficient gradient summed beside the term sums): K1 = 4 (Navier_Stokes) and 3 (physics_equation), tanh.
template <>
int tile_unit<TF_COEF, WP_>(const TileLaunch& a) {
  const int rc = with_k1<4, 3>(a.K1, [&](auto k) { return fwd_or_bwd<decltype(k)::value, PINN_ACT_TANH, EPI_COEF>(a, WHAT(", coefficient residual")); });
  if (rc != NO_INSTANCE) return rc;
  set_error("fused engine: no coefficient kernel for k = %d", a.K1 - 1);
  return PINN_ERR_UNSUPPORTED;
}

#elif defined(UNIT_wt)
// TF_WEIGHTED — point-weighted epilogue (EPI_WEIGHTED: the residual epilogue with one weight per point and weighted term, and
// an optional store of the signed fields): K1 = 4 (Navier_Stokes) and 3 (physics_equation, continuity_ftemp,
// continuity_only), tanh.
template <>
int tile_unit<TF_WEIGHTED, WP_>(const TileLaunch& a) {
  const int rc = with_k1<4, 3>(a.K1, [&](auto k) { return fwd_or_bwd<decltype(k)::value, PINN_ACT_TANH, EPI_WEIGHTED>(a, WHAT(", weighted residual")); });
  if (rc != NO_INSTANCE) return rc;
  set_error("fused engine: no weighted kernel for k = %d", a.K1 - 1);
  return PINN_ERR_UNSUPPORTED;
}

#elif defined(UNIT_sin)
// TF_SIN — sine first layer (PINN_ACT_SIN_TANH: a_1 = sin(W_0 x + b_0), tanh on the other hidden layers): generic epilogue,
// K1 = 1, 3, 4.
#if FUSED_WP == 64
// (this one instance is compiled in the unit UNIT_sin_g4 below, without -amdgpu-mfma-vgpr-form: see there)
extern template __global__ void k_fused<64, 4, true, false, PINN_ACT_SIN_TANH, EPI_GENERIC>(const FusedParams);
#endif
template <>
int tile_unit<TF_SIN, WP_>(const TileLaunch& a) {
  if (a.P.act != PINN_ACT_SIN_TANH) { set_error("fused engine: the sine instances serve activation 2 only (got %d)", a.P.act); return PINN_ERR_UNSUPPORTED; }
  const int rc = with_k1<4, 3, 1>(a.K1, [&](auto k) { return fwd_or_bwd<decltype(k)::value, PINN_ACT_SIN_TANH, EPI_GENERIC>(a, WHAT(", sine first layer")); });
  if (rc != NO_INSTANCE) return rc;
  set_error("fused engine: no sine-first-layer kernel for k = %d", a.K1 - 1);
  return PINN_ERR_UNSUPPORTED;
}

#elif defined(UNIT_sin_g4)
// ONE instance of TF_SIN, alone in its translation unit (pinn_fused_sin_w64_g4.o): padded width 64, K1 = 4, gradient pass with
// the workgroup's gradient copy in global memory.  With -amdgpu-mfma-vgpr-form (the switch of the other width-64 translation
// units, Makefile) clang 22 crashes on it in its 'Rewrite AGPR-Copy-MFMA' pass (eliminateSpillsOfReassignedVGPRs) once the
// GEMM streams and the weight gradient issue their memory and LDS instructions from slots between the MFMAs (fused_kernel.h)
// — whatever the slot spacing, and with the pacing of this instance switched off as well: the same pass and the same family
// (width 64, K1 = 4, global gradient copy) as the two crashes recorded in DESIGN 3.3.  Built without the switch the instance
// keeps 208 bytes per lane in scratch memory (244 before, with it); its eight siblings stay in pinn_fused_sin_w64.o and keep
// the switch (without it one of them would start to spill).
static_assert(WP_ == 64, "the unit of the one instance that crashes clang: width 64");
template __global__ void k_fused<64, 4, true, false, PINN_ACT_SIN_TANH, EPI_GENERIC>(const FusedParams);

#elif defined(UNIT_drop)
// TF_DROP — nn.Dropout(p > 0) in training mode (fused_kernel.h, DROP): padded width 64, tanh, gradient passes with the
// gradient copy in LDS, K1 = 1, 3, 4 (the harness's loss + gradient calls; train.py:186 puts the module in training mode).
// Forward-only and jet calls with dropout stay on the generic engine, whose pinn_jet_backward is the other half of the
// autograd route.
template <>
int tile_unit<TF_DROP, WP_>(const TileLaunch& a) {
  static_assert(WP_ == 64, "dropout instances: width 64");
  const int rc = with_k1<1, 3, 4>(a.K1, [&](auto k) {
    return go(k_fused<64, decltype(k)::value, true, true, PINN_ACT_TANH, EPI_GENERIC, 0, true>, a, WHAT(", dropout"));
  });
  if (rc != NO_INSTANCE) return rc;
  set_error("fused engine: no dropout kernel for K1=%d", a.K1);
  return PINN_ERR_UNSUPPORTED;
}

#elif defined(UNIT_ens)
// TF_ENS — the ensemble instances (k_fused_ens: a 2-D grid (gx, M), member = blockIdx.y, the single-network body behind one
// pointer shift): gradient passes of tanh networks with the generic loss epilogue, K1 = 3 or 4.
template <>
int tile_unit<TF_ENS, WP_>(const TileLaunch& a) {
  const int rc = with_k1<3, 4>(a.K1, [&](auto k) {
    constexpr int K1 = decltype(k)::value;
    return a.P.acc_lds ? go(k_fused_ens<WP_, K1, true>, a, WHAT(", ensemble")) : go(k_fused_ens<WP_, K1, false>, a, WHAT(", ensemble"));
  });
  if (rc != NO_INSTANCE) return rc;
  set_error("fused engine: no ensemble kernel for K1=%d", a.K1);
  return PINN_ERR_UNSUPPORTED;
}

#else
#error "pinn_fused_tile.hip: name the unit, -DUNIT_<family> (Makefile, TILE_FAMILIES)"
#endif

}  // namespace pinn
