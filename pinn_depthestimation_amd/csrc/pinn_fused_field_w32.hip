// pinn_fused_field_w32.hip — field (pinn_residual_fields) instances of the fused tile kernel, padded hidden width 32 (see pinn_fused_field.inc)
#define FUSED_WP 32
#include "pinn_fused_field.inc"
