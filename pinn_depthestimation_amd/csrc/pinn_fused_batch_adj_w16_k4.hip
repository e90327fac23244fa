// pinn_fused_batch_adj_w16_k4.hip — batch kernel instances with the external-adjoint epilogue (pinn_jet_backward), padded
// hidden width 16, K1 = 4 (see pinn_fused_batch.inc)
#define BATCH_WP 16
#define BATCH_K1 4
#define BATCH_EPI EPI_ADJ
#include "pinn_fused_batch.inc"
