// pinn_fused_wt_w64.hip — point-weighted instances of the fused tile kernel, padded hidden width 64 (see pinn_fused_wt.inc)
#define FUSED_WP 64
#include "pinn_fused_wt.inc"
