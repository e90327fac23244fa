// pinn_fused_adj_w64.hip — external-adjoint instances of the fused tile kernel, padded hidden width 64 (see pinn_fused_adj.inc)
#define FUSED_WP 64
#include "pinn_fused_adj.inc"
