// pinn_chain_units.hip — the instances of the bf16-mode chain kernels (chain_kernel.h) and their launchers.  ONE source, compiled
// once per padded width (csrc/Makefile): -DCHAIN_WP=<128|256> -> pinn_chain_w<WP>.o.
#include "wide_launch.h"

namespace pinn {

constexpr int NTW_ = CHAIN_WP / 16;
constexpr size_t CHAIN_RING_LDS = (size_t)CHAIN_RING * (NTW_ / 2) * 2 * 1024;
constexpr size_t CHAIN_WG_LDS = (size_t)WG_UNITS * 4 * (NTW_ / 2) * 1024;

// f(K1 as a constant) for K1 in {1, 3, 4}; the engine's one refusal of any other
template <class F>
static int for_k1(int K1, F f) {
  const int rc = with_k1<1, 3, 4>(K1, f);
  if (rc != NO_INSTANCE) return rc;
  set_error("chain engine: no kernel for K1=%d", K1);
  return PINN_ERR_UNSUPPORTED;
}

template <>
int launch_chain_fwd8<NTW_>(int K1, bool fold_first, const ChainParams& P, int grid, hipStream_t s) {
  const size_t lds = chain_fwd8_lds_bytes(NTW_, P.L, fold_first);
  if (lds > CHAIN_LDS_LIMIT) { set_error("chain engine: %d hidden layers need %zu bytes of LDS (limit %zu)", P.L, lds, CHAIN_LDS_LIMIT); return PINN_ERR_UNSUPPORTED; }
  return for_k1(K1, [&](auto k) {
    constexpr int K = decltype(k)::value;
    return fold_first ? launch_kernel(k_chain_fwd8<NTW_, K, true>, dim3(grid), P8_THREADS, lds, s, "chain fwd8", P)
                      : launch_kernel(k_chain_fwd8<NTW_, K, false>, dim3(grid), P8_THREADS, lds, s, "chain fwd8", P);
  });
}

template <>
int launch_chain_bwd<NTW_>(int K1, const ChainParams& P, int grid, hipStream_t s) {
  return for_k1(K1, [&](auto k) {
    constexpr int K = decltype(k)::value;
    // ring + per-wave prefetch areas (chain_pf_pieces k-step pieces of the next phase's a_l)
    const size_t lds = CHAIN_RING_LDS + (size_t)CHAIN_WAVES * chain_pf_pieces(NTW_, K) * K * 1024;
    return launch_kernel(k_chain_bwd<NTW_, K>, dim3(grid), CHAIN_THREADS, lds, s, "chain bwd", P);
  });
}

template <>
int launch_chain_wgrad8<NTW_>(int K1, const ChainParams& P, int grid, hipStream_t s) {
  return for_k1(K1, [&](auto k) {
    return launch_kernel(k_chain_wgrad8<NTW_, decltype(k)::value>, dim3(grid), P8_THREADS, CHAIN_WG_LDS, s, "chain wgrad8", P);
  });
}

template <>
int launch_chain_first_bwd<NTW_>(int K1, const ChainParams& P, int grid, hipStream_t s) {
  const size_t lds = (size_t)64 * NTW_ * 4;
  return for_k1(K1, [&](auto k) {
    return launch_kernel(k_chain_first_bwd<NTW_, decltype(k)::value>, dim3(grid), CHAIN_THREADS, lds, s, "chain first-layer bwd", P);
  });
}

template <>
int launch_chain_last_bwd<NTW_>(int K1, const ChainParams& P, int grid, hipStream_t s) {
  const size_t lds = (size_t)16 * NTW_ * 16 + (size_t)(64 * NTW_ + 4) * 4;
  return for_k1(K1, [&](auto k) {
    return launch_kernel(k_chain_last_bwd<NTW_, decltype(k)::value>, dim3(grid), CHAIN_THREADS, lds, s, "chain last-layer bwd", P);
  });
}

template <>
int launch_chain_last_fwd<NTW_>(int K1, bool grad, const FusedParams& P, const WideLayer& Lp, int grid, hipStream_t s) {
  const size_t lds = ((size_t)2 * (NTW_ / 2) * 64 * 4 + (size_t)WIDE_WAVES * LAST_PADS * TB_FLOATS + (size_t)WIDE_WAVES * MAX_SUMS) * 4;
  return for_k1(K1, [&](auto k) {
    constexpr int K = decltype(k)::value;
    return grad ? launch_kernel(k_chain_last_fwd<NTW_, K, true>, dim3(grid), WIDE_THREADS, lds, s, "chain last-layer fwd", P, Lp)
                : launch_kernel(k_chain_last_fwd<NTW_, K, false>, dim3(grid), WIDE_THREADS, lds, s, "chain last-layer fwd", P, Lp);
  });
}

}  // namespace pinn
