// pinn_chain_launch.inc — launchers of the bf16-mode chain kernels (chain_kernel.h), one translation unit per
// padded width: the includer defines CHAIN_NTW (16: W <= 256, 8: W <= 128).
#include "chain_kernel.h"

namespace pinn {

constexpr int CNTW_ = CHAIN_NTW;
constexpr size_t CHAIN_RING_LDS = (size_t)CHAIN_RING * (CNTW_ / 2) * 2 * 1024;
constexpr size_t CHAIN_WG_LDS = (size_t)WG_UNITS * 4 * (CNTW_ / 2) * 1024;

template <class K>
static int cgo(K kern, const ChainParams& P, int grid, size_t lds, hipStream_t s, const char* what) {
  if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds)) return rc;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(CHAIN_THREADS), lds, s, P);
  return check_launch(what);
}

template <class K>
static int cgo8(K kern, const ChainParams& P, int grid, size_t lds, hipStream_t s, const char* what) {
  if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds)) return rc;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(P8_THREADS), lds, s, P);
  return check_launch(what);
}
template <>
int launch_chain_fwd8<CNTW_>(int K1, bool fold_first, const ChainParams& P, int grid, hipStream_t s) {
  const size_t lds = chain_fwd8_lds_bytes(CNTW_, P.L, fold_first);
  if (lds > CHAIN_LDS_LIMIT) { set_error("chain engine: %d hidden layers need %zu bytes of LDS (limit %zu)", P.L, lds, CHAIN_LDS_LIMIT); return PINN_ERR_UNSUPPORTED; }
  if (fold_first) switch (K1) {
    case 1: return cgo8(k_chain_fwd8<CNTW_, 1, true>, P, grid, lds, s, "chain fwd8");
    case 3: return cgo8(k_chain_fwd8<CNTW_, 3, true>, P, grid, lds, s, "chain fwd8");
    case 4: return cgo8(k_chain_fwd8<CNTW_, 4, true>, P, grid, lds, s, "chain fwd8");
  }
  else switch (K1) {
    case 1: return cgo8(k_chain_fwd8<CNTW_, 1, false>, P, grid, lds, s, "chain fwd8");
    case 3: return cgo8(k_chain_fwd8<CNTW_, 3, false>, P, grid, lds, s, "chain fwd8");
    case 4: return cgo8(k_chain_fwd8<CNTW_, 4, false>, P, grid, lds, s, "chain fwd8");
  }
  set_error("chain engine: no kernel for K1=%d", K1); return PINN_ERR_UNSUPPORTED;
}

template <>
int launch_chain_bwd<CNTW_>(int K1, const ChainParams& P, int grid, hipStream_t s) {
  switch (K1) {
    // ring + per-wave prefetch areas (chain_pf_pieces k-step pieces of the next phase's a_l)
    case 1: return cgo(k_chain_bwd<CNTW_, 1>, P, grid, CHAIN_RING_LDS + (size_t)CHAIN_WAVES * chain_pf_pieces(CNTW_, 1) * 1 * 1024, s, "chain bwd");
    case 3: return cgo(k_chain_bwd<CNTW_, 3>, P, grid, CHAIN_RING_LDS + (size_t)CHAIN_WAVES * chain_pf_pieces(CNTW_, 3) * 3 * 1024, s, "chain bwd");
    case 4: return cgo(k_chain_bwd<CNTW_, 4>, P, grid, CHAIN_RING_LDS + (size_t)CHAIN_WAVES * chain_pf_pieces(CNTW_, 4) * 4 * 1024, s, "chain bwd");
  }
  set_error("chain engine: no kernel for K1=%d", K1); return PINN_ERR_UNSUPPORTED;
}
template <>
int launch_chain_wgrad8<CNTW_>(int K1, const ChainParams& P, int grid, hipStream_t s) {
  switch (K1) {
    case 1: return cgo8(k_chain_wgrad8<CNTW_, 1>, P, grid, CHAIN_WG_LDS, s, "chain wgrad8");
    case 3: return cgo8(k_chain_wgrad8<CNTW_, 3>, P, grid, CHAIN_WG_LDS, s, "chain wgrad8");
    case 4: return cgo8(k_chain_wgrad8<CNTW_, 4>, P, grid, CHAIN_WG_LDS, s, "chain wgrad8");
  }
  set_error("chain engine: no kernel for K1=%d", K1); return PINN_ERR_UNSUPPORTED;
}

template <>
int launch_chain_first_bwd<CNTW_>(int K1, const ChainParams& P, int grid, hipStream_t s) {
  const size_t lds = (size_t)64 * CNTW_ * 4;
  switch (K1) {
    case 1: return cgo(k_chain_first_bwd<CNTW_, 1>, P, grid, lds, s, "chain first-layer bwd");
    case 3: return cgo(k_chain_first_bwd<CNTW_, 3>, P, grid, lds, s, "chain first-layer bwd");
    case 4: return cgo(k_chain_first_bwd<CNTW_, 4>, P, grid, lds, s, "chain first-layer bwd");
  }
  set_error("chain engine: no kernel for K1=%d", K1); return PINN_ERR_UNSUPPORTED;
}

template <>
int launch_chain_last_bwd<CNTW_>(int K1, const ChainParams& P, int grid, hipStream_t s) {
  const size_t lds = (size_t)16 * CNTW_ * 16 + (size_t)(64 * CNTW_ + 4) * 4;
  switch (K1) {
    case 1: return cgo(k_chain_last_bwd<CNTW_, 1>, P, grid, lds, s, "chain last-layer bwd");
    case 3: return cgo(k_chain_last_bwd<CNTW_, 3>, P, grid, lds, s, "chain last-layer bwd");
    case 4: return cgo(k_chain_last_bwd<CNTW_, 4>, P, grid, lds, s, "chain last-layer bwd");
  }
  set_error("chain engine: no kernel for K1=%d", K1); return PINN_ERR_UNSUPPORTED;
}

template <class K>
static int cgo_last(K kern, const FusedParams& P, const WideLayer& Lp, int grid, hipStream_t s) {
  const size_t lds = ((size_t)2 * (CNTW_ / 2) * 64 * 4 + (size_t)WIDE_WAVES * LAST_PADS * TB_FLOATS + (size_t)WIDE_WAVES * MAX_SUMS) * 4;
  if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds)) return rc;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(WIDE_THREADS), lds, s, P, Lp);
  return check_launch("chain last-layer fwd");
}
template <>
int launch_chain_last_fwd<CNTW_>(int K1, bool grad, const FusedParams& P, const WideLayer& Lp, int grid, hipStream_t s) {
  if (grad) switch (K1) {
    case 1: return cgo_last(k_chain_last_fwd<CNTW_, 1, true>, P, Lp, grid, s);
    case 3: return cgo_last(k_chain_last_fwd<CNTW_, 3, true>, P, Lp, grid, s);
    case 4: return cgo_last(k_chain_last_fwd<CNTW_, 4, true>, P, Lp, grid, s);
  }
  else switch (K1) {
    case 1: return cgo_last(k_chain_last_fwd<CNTW_, 1, false>, P, Lp, grid, s);
    case 3: return cgo_last(k_chain_last_fwd<CNTW_, 3, false>, P, Lp, grid, s);
    case 4: return cgo_last(k_chain_last_fwd<CNTW_, 4, false>, P, Lp, grid, s);
  }
  set_error("chain engine: no kernel for K1=%d", K1); return PINN_ERR_UNSUPPORTED;
}

}  // namespace pinn
