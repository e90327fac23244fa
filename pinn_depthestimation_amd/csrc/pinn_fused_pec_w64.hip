// pinn_fused_pec_w64.hip — corrected-radiation-stress instances of the fused tile kernel, padded hidden width 64 (see pinn_fused_pec.inc)
#define FUSED_WP 64
#include "pinn_fused_pec.inc"
