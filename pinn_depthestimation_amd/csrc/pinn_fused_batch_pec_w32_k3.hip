// pinn_fused_batch_pec_w32_k3.hip — batch kernel instances with the corrected-radiation-stress loss epilogue (EPI_PEC), padded
// hidden width 32, K1 = 3 (see pinn_fused_batch.inc)
#define BATCH_WP 32
#define BATCH_K1 3
#define BATCH_EPI EPI_PEC
#define BATCH_LAUNCH launch_fused_batch_pec_k
#define BATCH_WHAT "fused batch kernel (corrected residual)"
#include "pinn_fused_batch.inc"
