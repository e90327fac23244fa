// pinn_lbfgs_ens.hip — the device-resident L-BFGS loop of an ensemble (include/pinn_hip.h, pinn_ensemble_lbfgs_loop): M
// networks, each with its own strong-Wolfe search, ring and stopping tests, advanced by ONE schedule of launches per slot.
//
// The kernels k_lbe_* run on a 2-D grid: blockIdx.x is what it is in pinn_lbfgs_loop.hip, blockIdx.y the member (the axis
// k_fused_ens uses).  Each forms member blockIdx.y's LblPtrs from the base pointers and strides of LbePtrs and calls the
// body the single loop calls (lbfgs_loop_bodies.h): there is no second copy of the state machine.
//
// Per member: its control block, d, the gradient pool, prev_g, s, y, q, the partials, the recursion's scratch, S, Y, M.
// Shared, as whole matrices, because the ensemble pass (fused_ensemble_loss) takes them so: x_trial (M, P) — its `params`
// —, g_new (M, P) — its gradient, added into, so the trial kernel zeroes it —, the term sums (M, n_terms) and the column
// sums (M, n_cols).  A member that has stopped is inert from then on: its kernels return (the trial kernel still zeroes
// its gradient row and sums, the control kernel its trace row), its row of `params` is not touched, and its pass runs on
// its unchanged row of x_trial.  No atomics: a member's reductions are its own per-workgroup partials combined by one
// workgroup in a fixed order, so member j's numbers do not depend on who else is in the ensemble.
//
// The recursion kernels' grid.x is the history size the call names, not the LBL_MAX_M rows the single loop launches: with
// a member axis that would be 256 x M workgroups per launch, nearly all returning.  A member whose control block holds
// another m is off in every kernel (lbl_off), as one with another P is.
#include "lbfgs_loop_bodies.h"

namespace pinn {
namespace {

__device__ __forceinline__ LblPtrs lbe_member(const LbePtrs& e) {
  const int64_t j = blockIdx.y;
  char* b = e.state;
  char* mb = b + e.L.mem + j * e.L.mem_stride;
  LblPtrs p;
  p.c = (pinn_lbfgs_ctrl*)(b + j * e.L.ctrl_stride);
  p.params = e.params + j * e.P;
  p.d = (float*)(b + e.L.d) + j * e.P; p.xt = (float*)(b + e.L.xt) + j * e.P; p.gnew = (float*)(b + e.L.gnew) + j * e.P;
  p.csums = (float*)(b + e.L.csums) + j * e.n_cols; p.tsums = (float*)(b + e.L.tsums) + j * e.n_terms;
  p.pool = (float*)(mb + e.L.in.pool); p.prevg = (float*)(mb + e.L.in.prevg); p.sv = (float*)(mb + e.L.in.sv);
  p.yv = (float*)(mb + e.L.in.yv); p.q = (float*)(mb + e.L.in.q); p.part = (double*)(mb + e.L.in.part);
  p.losses = (float*)(mb + e.L.in.losses); p.tmp = (double*)(mb + e.L.in.tmp); p.coef = (float*)(mb + e.L.in.coef);
  p.hist = mb + e.L.in.hist; p.P = e.P; p.m = e.m;
  return p;
}
__device__ __forceinline__ double* lbe_trace(double* trace) {
  return trace ? trace + (int64_t)blockIdx.y * PINN_LBFGS_TRACE_COLS : nullptr;
}

__global__ void k_lbe_init(char* state, int64_t ctrl_stride, int M, int64_t P, pinn_lbfgs_opts o) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < M) lbl_init_body((pinn_lbfgs_ctrl*)(state + j * ctrl_stride), P, o);
}
__global__ void k_lbe_trial(LbePtrs e) { lbl_trial_body(lbe_member(e), e.n_cols, e.n_terms); }
__global__ void k_lbe_dots(LbePtrs e) { lbl_dots_body(lbe_member(e)); }
__global__ void k_lbe_control(LbePtrs e, int nb, int n_loss_rows, const float* __restrict__ loss_rows, int total_row,
                              double* __restrict__ trace) {
  lbl_control_body(lbe_member(e), nb, e.n_cols, e.n_terms, n_loss_rows, loss_rows, total_row, lbe_trace(trace));
}
__global__ void k_lbe_accept1(LbePtrs e) { lbl_accept1_body(lbe_member(e)); }
__global__ void k_lbe_accept2(LbePtrs e, int nb, double* __restrict__ trace) { lbl_accept2_body(lbe_member(e), nb, lbe_trace(trace)); }
__global__ void k_lbe_push(LbePtrs e) { lbl_push_body(lbe_member(e)); }
__global__ void k_lbe_rowdots(LbePtrs e, int which) { lbl_rowdots_body(lbe_member(e), which); }
__global__ void k_lbe_solve_upper(LbePtrs e) { lbl_solve_upper_body(lbe_member(e)); }
__global__ void k_lbe_solve_lower(LbePtrs e) { lbl_solve_lower_body(lbe_member(e)); }
__global__ void k_lbe_combine(LbePtrs e, int which) { lbl_combine_body(lbe_member(e), which); }
__global__ void k_lbe_gtd(LbePtrs e) { lbl_gtd_body(lbe_member(e)); }
__global__ void k_lbe_arm(LbePtrs e, int nb, double* __restrict__ trace) { lbl_arm_body(lbe_member(e), nb, lbe_trace(trace)); }

}  // namespace

LbeLayout lbe_layout(int M, int64_t P, int m) {
  LbeLayout L;
  LbeMember& in = L.in;
  const int64_t vec = align256(P * 4);
  int64_t off = 0;
  in.pool = off; off += align256(PINN_LS_POOL_ROWS * P * 4);
  in.prevg = off; off += vec;
  in.sv = off; off += vec;
  in.yv = off; off += vec;
  in.q = off; off += vec;
  in.part = off; off += align256((int64_t)LBL_NB * LBL_PART * 8);
  in.losses = off; off += align256(8 * 4);
  in.tmp = off; off += align256(4 * LBL_MAX_M * 8);
  in.coef = off; off += align256(2 * LBL_MAX_M * 4);
  in.hist = off;
  off += 2 * align256((int64_t)m * P * 4) + align256((int64_t)m * m * 8);
  in.total = off;
  const int64_t mat = align256((int64_t)M * P * 4), sums = align256((int64_t)M * PINN_MAX_ROLES * 4);
  L.ctrl_stride = align256((int64_t)sizeof(pinn_lbfgs_ctrl));
  off = (int64_t)M * L.ctrl_stride;
  L.d = off; off += mat;
  L.xt = off; off += mat;
  L.gnew = off; off += mat;
  L.csums = off; off += sums;
  L.tsums = off; off += sums;
  L.mem = off; L.mem_stride = in.total;
  L.total = off + (int64_t)M * in.total;
  return L;
}

LbePtrs lbe_ptrs(void* state, float* params, int M, int64_t P, int m, int n_cols, int n_terms) {
  LbePtrs e;
  e.state = (char*)state; e.params = params; e.P = P; e.M = M; e.m = m; e.n_cols = n_cols; e.n_terms = n_terms;
  e.L = lbe_layout(M, P, m);
  return e;
}

int lbe_init(void* state, int M, int64_t P, const pinn_lbfgs_opts& o, hipStream_t s) {
  const LbeLayout L = lbe_layout(M, P, o.history_size);
  if (hipMemsetAsync(state, 0, (size_t)L.total, s) != hipSuccess) { set_error("pinn_ensemble_lbfgs_loop_init: memset failed"); return PINN_ERR_LAUNCH; }
  hipLaunchKernelGGL(k_lbe_init, dim3((M + 63) / 64), dim3(64), 0, s, (char*)state, L.ctrl_stride, M, P, o);
  return check_launch("ensemble lbfgs loop init");
}

int lbe_before_pass(const LbePtrs& e, hipStream_t s) {
  hipLaunchKernelGGL(k_lbe_trial, dim3(lbl_grid(e.P), e.M), dim3(LBL_T), 0, s, e);
  return check_launch("ensemble lbfgs loop trial");
}

int lbe_after_pass(const LbePtrs& e, int n_loss_rows, const float* loss_rows, int total_row, double* trace_rows, hipStream_t s) {
  const unsigned nb = lbl_grid(e.P), M = e.M, m = e.m;
  const unsigned gp = (unsigned)((e.P + LB_T - 1) / LB_T);
  hipLaunchKernelGGL(k_lbe_dots, dim3(nb, M), dim3(LBL_T), 0, s, e);
  hipLaunchKernelGGL(k_lbe_control, dim3(1, M), dim3(LBL_T), 0, s, e, (int)nb, n_loss_rows, loss_rows, total_row, trace_rows);
  hipLaunchKernelGGL(k_lbe_accept1, dim3(nb, M), dim3(LBL_T), 0, s, e);
  hipLaunchKernelGGL(k_lbe_accept2, dim3(1, M), dim3(LBL_T), 0, s, e, (int)nb, trace_rows);
  hipLaunchKernelGGL(k_lbe_push, dim3(m + nb, M), dim3(LBL_T), 0, s, e);
  hipLaunchKernelGGL(k_lbe_rowdots, dim3(m, M), dim3(LB_T), 0, s, e, 0);
  hipLaunchKernelGGL(k_lbe_solve_upper, dim3(1, M), dim3(64), 0, s, e);
  hipLaunchKernelGGL(k_lbe_combine, dim3(gp, M), dim3(LB_T), 0, s, e, 0);
  hipLaunchKernelGGL(k_lbe_rowdots, dim3(m, M), dim3(LB_T), 0, s, e, 1);
  hipLaunchKernelGGL(k_lbe_solve_lower, dim3(1, M), dim3(64), 0, s, e);
  hipLaunchKernelGGL(k_lbe_combine, dim3(gp, M), dim3(LB_T), 0, s, e, 1);
  hipLaunchKernelGGL(k_lbe_gtd, dim3(nb, M), dim3(LBL_T), 0, s, e);
  hipLaunchKernelGGL(k_lbe_arm, dim3(1, M), dim3(LBL_T), 0, s, e, (int)nb, trace_rows);
  return check_launch("ensemble lbfgs loop slot");
}

}  // namespace pinn
