// pinn_fused_w16.hip — fused tile kernel instances, padded hidden width 16 (see pinn_fused_launch.inc)
#define FUSED_WP 16
#include "pinn_fused_launch.inc"
