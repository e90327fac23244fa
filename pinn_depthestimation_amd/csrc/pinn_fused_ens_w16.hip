// the fused tile kernel's ensemble instances at padded width 16 (pinn_fused_ens.inc)
#define FUSED_WP 16
#include "pinn_fused_ens.inc"
