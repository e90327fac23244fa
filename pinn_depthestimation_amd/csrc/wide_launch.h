// wide_launch.h — host side of every launch of the wide and chain engines' kernels: the entry points through which
// pinn_wide.hip reaches the translation units that hold the instances (pinn_wide_units.hip, pinn_chain_units.hip: one
// source each, compiled once per unit with the unit named on the command line — Makefile).  Each is defined once per
// padded width (NTW = 8: W <= 128, 16: W <= 256).  Host only: nothing here is seen by a kernel.
#pragma once
#include "launch.h"
#include "chain_kernel.h"

namespace pinn {

enum WidePlace { WIDE_FIRST, WIDE_HIDDEN, WIDE_LAST };   // which layer of the network a per-layer launch serves

// ---- fp32 mode: one launch per layer and direction (wide_kernel.h), units pinn_wide_w{128,256}.o --------------------------------
template <int NTW> int launch_wide_fwd(WidePlace at, int K1, bool grad, const FusedParams& P, const WideLayer& Lp, int grid, hipStream_t s);
template <int NTW> int launch_wide_bwd(WidePlace at, int K1, const FusedParams& P, const WideLayer& Lp, int grid, hipStream_t s);
template <int NTW> int launch_wide_wgrad(WidePlace at, int K1, const FusedParams& P, const WideLayer& Lp, int grid, hipStream_t s);

// ---- bf16 mode: the thin first / last layers on the per-layer kernels, reading and writing the chain kernels' bf16 jets:
// the five instances run_w can launch, units pinn_wide_w{128,256}_bf16.o ---------------------------------------------------------
enum WideThin {
  THIN_FIRST_FWD,     // d_in > 3 only (otherwise the first layer is folded into k_chain_fwd8)
  THIN_FIRST_BWD,     // ... and its activation adjoint
  THIN_FIRST_WGRAD,   // ... and its weight gradient
  THIN_LAST_WGRAD,    // d_out > 4 only (otherwise k_chain_last_bwd does both)
  THIN_LAST_BWD,
};
template <int NTW> int launch_wide_thin(WideThin which, int K1, const FusedParams& P, const WideLayer& Lp, int grid, hipStream_t s);

// ---- bf16 mode: the chain kernels (chain_kernel.h), units pinn_chain_w{128,256}.o ----------------------------------------------
template <int NTW> int launch_chain_fwd8(int K1, bool fold_first, const ChainParams& P, int grid, hipStream_t s);
template <int NTW> int launch_chain_bwd(int K1, const ChainParams& P, int grid, hipStream_t s);
template <int NTW> int launch_chain_wgrad8(int K1, const ChainParams& P, int grid, hipStream_t s);
template <int NTW> int launch_chain_first_bwd(int K1, const ChainParams& P, int grid, hipStream_t s);
template <int NTW> int launch_chain_last_bwd(int K1, const ChainParams& P, int grid, hipStream_t s);
template <int NTW> int launch_chain_last_fwd(int K1, bool grad, const FusedParams& P, const WideLayer& Lp, int grid, hipStream_t s);

}  // namespace pinn
