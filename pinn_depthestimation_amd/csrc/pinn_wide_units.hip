// pinn_wide_units.hip — the instances of the wide engine's per-layer kernels (wide_kernel.h) and their launchers.  ONE source,
// compiled once per unit (csrc/Makefile): -DWIDE_WP=<128|256> names the padded width, -DUNIT_f32 or -DUNIT_bf16 the precision
// mode the unit serves (pinn_wide_w<WP>.o, pinn_wide_w<WP>_bf16.o).  Two units per width because the two modes want
// different compiler scheduling: without LLVM's pre-RA machine scheduler (-mllvm -enable-misched=0) the fp32 kernels are
// 13 % faster and the bf16-mode kernels 14 % slower (measured, 12x256, tools/ab_multi.sh).
#include "wide_launch.h"

namespace pinn {

constexpr int NTW_ = WIDE_WP / 16;
constexpr int A_ = PINN_ACT_TANH;
constexpr size_t PADS_LDS = (size_t)(WIDE_WAVES * WIDE_MAX_PADS * TB_FLOATS + WIDE_WAVES * MAX_SUMS) * 4;

// f(K1 as a constant) for K1 in {1, 3, 4}; the engine's one refusal of any other
template <class F>
static int for_k1(int K1, F f) {
  const int rc = with_k1<1, 3, 4>(K1, f);
  if (rc != NO_INSTANCE) return rc;
  set_error("wide engine: no kernel for K1=%d", K1);
  return PINN_ERR_UNSUPPORTED;
}
template <class K>
static int go(K kern, int grid, size_t lds, hipStream_t s, const char* what, const FusedParams& P, const WideLayer& Lp) {
  return launch_kernel(kern, dim3(grid), WIDE_THREADS, lds, s, what, P, Lp);
}

#if defined(UNIT_f32)
template <>
int launch_wide_fwd<NTW_>(WidePlace at, int K1, bool grad, const FusedParams& P, const WideLayer& Lp, int grid, hipStream_t s) {
  return for_k1(K1, [&](auto k) {
    constexpr int K = decltype(k)::value;
    switch (at) {
      case WIDE_FIRST: return go(k_wide_fwd<1, NTW_, K, A_, true, false, false>, grid, 0, s, "wide fwd first", P, Lp);
      case WIDE_HIDDEN: return go(k_wide_fwd<NTW_, NTW_, K, A_, false, false, false>, grid, 0, s, "wide fwd hidden", P, Lp);
      default:
        return grad ? go(k_wide_fwd<NTW_, 1, K, A_, false, true, true>, grid, PADS_LDS, s, "wide fwd last", P, Lp)
                    : go(k_wide_fwd<NTW_, 1, K, A_, false, true, false>, grid, PADS_LDS, s, "wide fwd last", P, Lp);
    }
  });
}
template <>
int launch_wide_bwd<NTW_>(WidePlace at, int K1, const FusedParams& P, const WideLayer& Lp, int grid, hipStream_t s) {
  return for_k1(K1, [&](auto k) {
    constexpr int K = decltype(k)::value;
    switch (at) {
      case WIDE_FIRST: return go(k_wide_bwd<NTW_, 1, K, A_, true, false>, grid, 0, s, "wide bwd first", P, Lp);
      case WIDE_HIDDEN: return go(k_wide_bwd<NTW_, NTW_, K, A_, true, true>, grid, 0, s, "wide bwd hidden", P, Lp);
      default: return go(k_wide_bwd<1, NTW_, K, A_, false, true>, grid, 0, s, "wide bwd last", P, Lp);
    }
  });
}
template <>
int launch_wide_wgrad<NTW_>(WidePlace at, int K1, const FusedParams& P, const WideLayer& Lp, int grid, hipStream_t s) {
  return for_k1(K1, [&](auto k) {
    constexpr int K = decltype(k)::value;
    switch (at) {
      case WIDE_FIRST: return go(k_wide_wgrad<4, NTW_, 1, K, true>, grid, PADS_LDS, s, "wide wgrad first", P, Lp);
      case WIDE_HIDDEN: return go(k_wide_wgrad<4, NTW_, NTW_, K, false>, grid, PADS_LDS, s, "wide wgrad hidden", P, Lp);
      default: return go(k_wide_wgrad<1, 1, NTW_, K, false>, grid, PADS_LDS, s, "wide wgrad last", P, Lp);
    }
  });
}

#elif defined(UNIT_bf16)
// the jets are stored as bf16 in the chain layout (wide_kernel.h, FMT bits) while the thin layers' MFMAs stay fp32
template <>
int launch_wide_thin<NTW_>(WideThin which, int K1, const FusedParams& P, const WideLayer& Lp, int grid, hipStream_t s) {
  return for_k1(K1, [&](auto k) {
    constexpr int K = decltype(k)::value;
    switch (which) {
      case THIN_FIRST_FWD:
        return go(k_wide_fwd<1, NTW_, K, A_, true, false, false, FMT_OUT16>, grid, 0, s, "wide fwd first", P, Lp);
      case THIN_FIRST_BWD:
        return go(k_wide_bwd<NTW_, 1, K, A_, true, false, FMT_IN16 | FMT_GIN16 | FMT_OUT16>, grid, 0, s, "wide bwd first", P, Lp);
      case THIN_FIRST_WGRAD:
        return go(k_wide_wgrad<4, NTW_, 1, K, true, FMT_GIN16>, grid, PADS_LDS, s, "wide wgrad first", P, Lp);
      case THIN_LAST_WGRAD:
        return go(k_wide_wgrad<1, 1, NTW_, K, false, FMT_IN16>, grid, PADS_LDS, s, "wide wgrad last", P, Lp);
      default:
        return go(k_wide_bwd<1, NTW_, K, A_, false, true, FMT_OUT16>, grid, 0, s, "wide bwd last", P, Lp);
    }
  });
}

#else
#error "pinn_wide_units.hip: name the unit with -DUNIT_f32 or -DUNIT_bf16 (csrc/Makefile)"
#endif

}  // namespace pinn
