// pinn_fused_field_w16.hip — field (pinn_residual_fields) instances of the fused tile kernel, padded hidden width 16 (see pinn_fused_field.inc)
#define FUSED_WP 16
#include "pinn_fused_field.inc"
