// the fused tile kernel's ensemble instances at padded width 64 (pinn_fused_ens.inc)
#define FUSED_WP 64
#include "pinn_fused_ens.inc"
