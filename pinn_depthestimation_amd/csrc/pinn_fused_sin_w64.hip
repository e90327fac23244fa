// pinn_fused_sin_w64.hip — sine-first-layer instances of the fused tile kernel, padded hidden width 64 (see pinn_fused_sin.inc)
#define FUSED_WP 64
#include "pinn_fused_sin.inc"
