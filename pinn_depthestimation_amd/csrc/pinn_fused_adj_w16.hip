// pinn_fused_adj_w16.hip — external-adjoint instances of the fused tile kernel, padded hidden width 16 (see pinn_fused_adj.inc)
#define FUSED_WP 16
#include "pinn_fused_adj.inc"
