// pinn_fused_pec_w32.hip — corrected-radiation-stress instances of the fused tile kernel, padded hidden width 32 (see pinn_fused_pec.inc)
#define FUSED_WP 32
#include "pinn_fused_pec.inc"
