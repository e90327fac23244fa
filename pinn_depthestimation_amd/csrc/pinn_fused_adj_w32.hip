// pinn_fused_adj_w32.hip — external-adjoint instances of the fused tile kernel, padded hidden width 32 (see pinn_fused_adj.inc)
#define FUSED_WP 32
#include "pinn_fused_adj.inc"
