// pinn_fused_pec_w16.hip — corrected-radiation-stress instances of the fused tile kernel, padded hidden width 16 (see pinn_fused_pec.inc)
#define FUSED_WP 16
#include "pinn_fused_pec.inc"
