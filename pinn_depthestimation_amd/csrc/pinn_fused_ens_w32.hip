// the fused tile kernel's ensemble instances at padded width 32 (pinn_fused_ens.inc)
#define FUSED_WP 32
#include "pinn_fused_ens.inc"
