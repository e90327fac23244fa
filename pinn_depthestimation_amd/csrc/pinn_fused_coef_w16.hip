// pinn_fused_coef_w16.hip — runtime-coefficient instances of the fused tile kernel, padded hidden width 16 (see pinn_fused_coef.inc)
#define FUSED_WP 16
#include "pinn_fused_coef.inc"
