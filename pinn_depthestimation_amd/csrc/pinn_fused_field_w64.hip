// pinn_fused_field_w64.hip — field (pinn_residual_fields) instances of the fused tile kernel, padded hidden width 64 (see pinn_fused_field.inc)
#define FUSED_WP 64
#include "pinn_fused_field.inc"
