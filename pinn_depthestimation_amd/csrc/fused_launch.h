// fused_launch.h — host side of every launch of the fused engine's kernels: the launch helper (launch.h), and the one entry point
// per kernel through which pinn_fused.hip reaches the translation units that hold the instances (pinn_fused_tile.hip,
// pinn_fused_batch.hip: one source each, compiled once per unit with the unit named on the command line — Makefile).
// Host only: nothing here is seen by a kernel.
#pragma once
#include "launch.h"
#include "fused_kernel.h"

namespace pinn {

// ---- the tile kernel (fused_kernel.h: k_fused, k_fused_ens) -----------------------------------------------------------------
// A family is a set of instances with one epilogue / activation / grid shape, in translation units of its own per padded
// width (pinn_fused_tile.hip says which instances each has, the Makefile which flags its units get).
enum TileFamily {
  TF_LOSS,        // generic epilogue, tanh / LeakyReLU; width 64 adds the residual-only specialised epilogues
  TF_ADJ,         // external adjoint (pinn_jet_backward)
  TF_FIELD,       // per-point residual fields, forward only
  TF_PEC,         // corrected radiation stress, loss
  TF_FIELD_PEC,   // corrected radiation stress, fields (in TF_PEC's units)
  TF_COEF,        // runtime closure coefficients
  TF_WEIGHTED,    // point weights
  TF_SIN,         // sine first layer
  TF_DROP,        // training-mode dropout (width 64 only)
  TF_ENS,         // ensemble: k_fused_ens on a grid (gx, M)
  TF_WAVE,        // wave closure (corrected stress + dispersion + wave-energy balance), loss
  TF_FIELD_WAVE,  // wave closure, fields (in TF_WAVE's units)
  TF_COUNT
};
struct TileLaunch {
  int K1;
  bool grad;
  const FusedParams& P;
  dim3 grid;
  size_t lds_bytes;
  hipStream_t s;
};
// defined once per (family, width) unit; launch_tile (pinn_fused.hip) holds the table of them
template <TileFamily F, int WP>
int tile_unit(const TileLaunch& a);
int launch_tile(TileFamily f, int WP, const TileLaunch& a);

// ---- the batch kernel (fused_batch_kernel.h: k_fused_batch) -----------------------------------------------------------------
enum BatchFamily { BF_LOSS, BF_ADJ, BF_PEC, BF_COUNT };   // generic loss, external adjoint, corrected radiation stress (K1 = 3 only)
struct BatchLaunch {
  int W, d_in;
  const FusedParams& P;
  int grid;
  size_t lds_bytes;
  hipStream_t s;
};
// defined once per (family, width, K1) unit; launch_batch (pinn_fused.hip) holds the table of them
template <BatchFamily F, int WP, int K1>
int batch_unit(const BatchLaunch& a);
int launch_batch(BatchFamily f, int WP, int K1, const BatchLaunch& a);

}  // namespace pinn
