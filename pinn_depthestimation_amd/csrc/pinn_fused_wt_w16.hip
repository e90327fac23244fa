// pinn_fused_wt_w16.hip — point-weighted instances of the fused tile kernel, padded hidden width 16 (see pinn_fused_wt.inc)
#define FUSED_WP 16
#include "pinn_fused_wt.inc"
