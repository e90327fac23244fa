// pinn_fused_wt_w32.hip — point-weighted instances of the fused tile kernel, padded hidden width 32 (see pinn_fused_wt.inc)
#define FUSED_WP 32
#include "pinn_fused_wt.inc"
