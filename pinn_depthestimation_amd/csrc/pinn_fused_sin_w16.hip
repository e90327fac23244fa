// pinn_fused_sin_w16.hip — sine-first-layer instances of the fused tile kernel, padded hidden width 16 (see pinn_fused_sin.inc)
#define FUSED_WP 16
#include "pinn_fused_sin.inc"
