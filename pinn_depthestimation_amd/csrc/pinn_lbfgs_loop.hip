// pinn_lbfgs_loop.hip — the device-resident L-BFGS loop (include/pinn_hip.h, pinn_lbfgs_loop): the kernels around the
// loss + gradient pass of one SLOT.  The host enqueues the same launches for every slot; what a slot does is decided by the
// control block (pinn_lbfgs_ctrl, offset 0 of `state`) that these kernels read and write:
//
//   k_lbl_trial, (the pass: run_loss, pinn_abi.hip, params = x_trial), k_lbl_dots, k_lbl_control, k_lbl_accept1,
//   k_lbl_accept2, k_lbl_push, k_lbl_rowdots / k_lbl_solve_upper / k_lbl_combine / k_lbl_rowdots / k_lbl_solve_lower /
//   k_lbl_combine, k_lbl_gtd, k_lbl_arm
//
// Each is one line around its body in lbfgs_loop_bodies.h, which says what it does and is shared with the ensemble loop
// (pinn_lbfgs_ens.hip).
#include "lbfgs_loop_bodies.h"

namespace pinn {
namespace {

__global__ void k_lbl_init(pinn_lbfgs_ctrl* c, int64_t P, pinn_lbfgs_opts o) {
  if (threadIdx.x == 0 && blockIdx.x == 0) lbl_init_body(c, P, o);
}
__global__ void k_lbl_trial(LblPtrs p, int n_cols, int n_terms) { lbl_trial_body(p, n_cols, n_terms); }
__global__ void k_lbl_dots(LblPtrs p) { lbl_dots_body(p); }
__global__ void k_lbl_control(LblPtrs p, int nb, int n_cols, int n_terms, int n_loss_rows, const float* __restrict__ loss_rows,
                              int total_row, double* __restrict__ trace) {
  lbl_control_body(p, nb, n_cols, n_terms, n_loss_rows, loss_rows, total_row, trace);
}
__global__ void k_lbl_accept1(LblPtrs p) { lbl_accept1_body(p); }
__global__ void k_lbl_accept2(LblPtrs p, int nb, double* __restrict__ trace) { lbl_accept2_body(p, nb, trace); }
__global__ void k_lbl_push(LblPtrs p) { lbl_push_body(p); }
__global__ void k_lbl_rowdots(LblPtrs p, int which) { lbl_rowdots_body(p, which); }
__global__ void k_lbl_solve_upper(LblPtrs p) { lbl_solve_upper_body(p); }
__global__ void k_lbl_solve_lower(LblPtrs p) { lbl_solve_lower_body(p); }
__global__ void k_lbl_combine(LblPtrs p, int which) { lbl_combine_body(p, which); }
__global__ void k_lbl_gtd(LblPtrs p) { lbl_gtd_body(p); }
__global__ void k_lbl_arm(LblPtrs p, int nb, double* __restrict__ trace) { lbl_arm_body(p, nb, trace); }

}  // namespace

LblLayout lbl_layout(int64_t P, int m) {
  LblLayout L;
  int64_t off = align256((int64_t)sizeof(pinn_lbfgs_ctrl));
  const int64_t vec = align256(P * 4);
  L.d = off; off += vec;
  L.xt = off; off += vec;
  L.gnew = off; off += vec;
  L.pool = off; off += align256(PINN_LS_POOL_ROWS * P * 4);
  L.prevg = off; off += vec;
  L.sv = off; off += vec;
  L.yv = off; off += vec;
  L.q = off; off += vec;
  L.part = off; off += align256((int64_t)LBL_NB * LBL_PART * 8);
  L.sums = off; off += align256(LBL_MAX_SUMS * 4);
  L.losses = off; off += align256(8 * 4);
  L.tmp = off; off += align256(4 * LBL_MAX_M * 8);
  L.coef = off; off += align256(2 * LBL_MAX_M * 4);
  L.hist = off;
  off += 2 * align256((int64_t)m * P * 4) + align256((int64_t)m * m * 8);
  L.total = off;
  return L;
}

LblPtrs lbl_ptrs(void* state, float* params, int64_t P, int n_cols) {
  const LblLayout L = lbl_layout(P, 1);
  char* b = (char*)state;
  LblPtrs p;
  p.c = (pinn_lbfgs_ctrl*)b; p.params = params;
  p.d = (float*)(b + L.d); p.xt = (float*)(b + L.xt); p.gnew = (float*)(b + L.gnew); p.pool = (float*)(b + L.pool);
  p.prevg = (float*)(b + L.prevg); p.sv = (float*)(b + L.sv); p.yv = (float*)(b + L.yv); p.q = (float*)(b + L.q);
  p.part = (double*)(b + L.part); p.csums = (float*)(b + L.sums); p.tsums = p.csums + n_cols; p.losses = (float*)(b + L.losses);
  p.tmp = (double*)(b + L.tmp); p.coef = (float*)(b + L.coef); p.hist = b + L.hist; p.P = P; p.m = 0;
  return p;
}

int lbl_init(void* state, int64_t state_bytes, int64_t P, const pinn_lbfgs_opts& o, hipStream_t s) {
  const LblLayout L = lbl_layout(P, o.history_size);
  if (hipMemsetAsync(state, 0, (size_t)L.total, s) != hipSuccess) { set_error("pinn_lbfgs_loop_init: memset failed"); return PINN_ERR_LAUNCH; }
  hipLaunchKernelGGL(k_lbl_init, dim3(1), dim3(64), 0, s, (pinn_lbfgs_ctrl*)state, P, o);
  return check_launch("lbfgs loop init");
}

int lbl_before_pass(const LblPtrs& p, int n_cols, int n_terms, hipStream_t s) {
  hipLaunchKernelGGL(k_lbl_trial, dim3(lbl_grid(p.P)), dim3(LBL_T), 0, s, p, n_cols, n_terms);
  return check_launch("lbfgs loop trial");
}

int lbl_after_pass(const LblPtrs& p, int n_cols, int n_terms, int n_loss_rows, const float* loss_rows, int total_row,
                   double* trace_row, hipStream_t s) {
  const int nb = lbl_grid(p.P);
  const unsigned gp = (unsigned)((p.P + LB_T - 1) / LB_T);
  hipLaunchKernelGGL(k_lbl_dots, dim3(nb), dim3(LBL_T), 0, s, p);
  hipLaunchKernelGGL(k_lbl_control, dim3(1), dim3(LBL_T), 0, s, p, nb, n_cols, n_terms, n_loss_rows, loss_rows, total_row, trace_row);
  hipLaunchKernelGGL(k_lbl_accept1, dim3(nb), dim3(LBL_T), 0, s, p);
  hipLaunchKernelGGL(k_lbl_accept2, dim3(1), dim3(LBL_T), 0, s, p, nb, trace_row);
  hipLaunchKernelGGL(k_lbl_push, dim3(LBL_MAX_M + nb), dim3(LBL_T), 0, s, p);
  hipLaunchKernelGGL(k_lbl_rowdots, dim3(LBL_MAX_M), dim3(LB_T), 0, s, p, 0);
  hipLaunchKernelGGL(k_lbl_solve_upper, dim3(1), dim3(64), 0, s, p);
  hipLaunchKernelGGL(k_lbl_combine, dim3(gp), dim3(LB_T), 0, s, p, 0);
  hipLaunchKernelGGL(k_lbl_rowdots, dim3(LBL_MAX_M), dim3(LB_T), 0, s, p, 1);
  hipLaunchKernelGGL(k_lbl_solve_lower, dim3(1), dim3(64), 0, s, p);
  hipLaunchKernelGGL(k_lbl_combine, dim3(gp), dim3(LB_T), 0, s, p, 1);
  hipLaunchKernelGGL(k_lbl_gtd, dim3(nb), dim3(LBL_T), 0, s, p);
  hipLaunchKernelGGL(k_lbl_arm, dim3(1), dim3(LBL_T), 0, s, p, nb, trace_row);
  return check_launch("lbfgs loop slot");
}

}  // namespace pinn
