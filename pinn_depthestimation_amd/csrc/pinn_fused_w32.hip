// pinn_fused_w32.hip — fused tile kernel instances, padded hidden width 32 (see pinn_fused_launch.inc)
#define FUSED_WP 32
#include "pinn_fused_launch.inc"
