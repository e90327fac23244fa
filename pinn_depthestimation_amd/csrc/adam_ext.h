// adam_ext.h — pinn_adam_loop_ext (include/pinn_hip.h): device-enqueued Adam runs of the residual with runtime coefficients
// or with point weights.  What pinn_abi.hip (validation) hands pinn_fused.hip (passes + the finishing kernel).
#pragma once
#include "common.h"

namespace pinn {

struct AdamExtReq {
  LossReq res;          // the residual pass: kind 0 with coef (coefficients) or point_w (weights) set; sums = term_sums,
                        // grad = grad_flat (OVERWRITTEN by the finishing kernel), adam null
  LossReq fid;          // the fidelity pass: kind 1; read only when N_fid > 0
  const float* Xf; int64_t N_fid;
  AdamReq adam;         // params, m, v, packed_valid and the loss rows (c is not read: each iteration forms its own scalars)
  double beta1, beta2, eps; int64_t step;   // iteration i runs step + i
  int row_cols;         // the caller's n_cols (loss_rows' stride)
  float* col_sums;      // the caller's (row_cols): zeroed once when there is no fidelity pass
  // coefficients (res.coef set): updated in place unless coef_grad is null
  float* coef; float* coef_m; float* coef_v; float* coef_grad; const float* coef_mask; float* coef_log; int n_coef;
  // weights (res.point_w set): lam null = fixed
  float* point_w; int w_rows; float* lam; float* lam_m; float* lam_v; int sa_mask;
  int n_iters; const double* lr; const double* lr_coef; const double* lr_w;   // HOST arrays (n_iters)
};

// why the fused engine does not run the request as a device-enqueued run, or nullptr (pure host logic): the rule of the
// family's instances (fused_tile_refusal of TILE_COEF / TILE_WEIGHTED) and a K1 = 1 gradient pass for the fidelity points
const char* fused_adam_ext_refusal(const Net& n, int family);
int64_t fused_adam_ext_workspace_bytes(const Net& n, int64_t N_res, int64_t N_fid);
int fused_adam_ext(const Net& n, const AdamExtReq& q, const float* X, int64_t N_res, void* ws, int64_t ws_bytes, hipStream_t s);

}  // namespace pinn
