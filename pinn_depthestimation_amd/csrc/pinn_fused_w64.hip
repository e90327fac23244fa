// pinn_fused_w64.hip — fused tile kernel instances, padded hidden width 64 (see pinn_fused_launch.inc)
#define FUSED_WP 64
#include "pinn_fused_launch.inc"
