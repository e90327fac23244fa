// pinn_fused_coef_w32.hip — runtime-coefficient instances of the fused tile kernel, padded hidden width 32 (see pinn_fused_coef.inc)
#define FUSED_WP 32
#include "pinn_fused_coef.inc"
