// pinn_fused_sin_w32.hip — sine-first-layer instances of the fused tile kernel, padded hidden width 32 (see pinn_fused_sin.inc)
#define FUSED_WP 32
#include "pinn_fused_sin.inc"
