// pinn_fused_coef_w64.hip — runtime-coefficient instances of the fused tile kernel, padded hidden width 64 (see pinn_fused_coef.inc)
#define FUSED_WP 64
#include "pinn_fused_coef.inc"
