// pinn_lbfgs_loop.hip — the device-resident L-BFGS loop (include/pinn_hip.h, pinn_lbfgs_loop): the kernels around the
// loss + gradient pass of one SLOT.  The host enqueues the same launches for every slot; what a slot does is decided by the
// control block (pinn_lbfgs_ctrl, offset 0 of `state`) that these kernels read and write:
//
//   k_lbl_trial     x_trial = x + t d; zeroes the gradient buffer and the sums the pass adds into
//   (the pass)      run_loss, pinn_abi.hip, params = x_trial
//   k_lbl_dots      per-workgroup partial sums of g_new . d
//   k_lbl_control   one workgroup: fixed-order fp64 combine, the weighted losses, ls_step, the trace row
//   k_lbl_accept1   files g_new in its pool row; on ACCEPT: x += t* d, s, y, prev_g, partials of y.s, y.y, max|g|, max|s|
//   k_lbl_accept2   one workgroup: the stopping tests, the ring bookkeeping, H (first iteration: t = min(1, 1/|g|_1) lr)
//   k_lbl_push      rows and columns of M for the new pair, and its copy into S, Y
//   k_lbl_rowdots / k_lbl_solve_upper / k_lbl_combine / k_lbl_rowdots / k_lbl_solve_lower / k_lbl_combine
//                   the recursion of pinn_lbfgs.hip, bodies shared (lbfgs_recursion.h), head / k / H from the control block
//   k_lbl_gtd       partials of g . d and max|d|
//   k_lbl_arm       one workgroup: the g.d test, ls_init
//
// Every kernel returns at once when the done flag is up; every kernel from k_lbl_accept2's successors on returns unless the
// slot is an accept.  No atomics: reductions are per-workgroup partials (a fixed grid for a given P) combined by one
// workgroup in a fixed order, so the loop is reproducible wherever the pass is.  Sized for P up to 2^20 + 3 and beyond
// (grid-stride, 64-bit offsets) and m <= 256.
#include "lbfgs_loop.h"
#include "lbfgs_line_search.h"
#include "lbfgs_recursion.h"

namespace pinn {
namespace {

constexpr int LBL_T = 256;

__device__ __forceinline__ double blk_sum(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = LBL_T / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}
__device__ __forceinline__ double blk_max(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = LBL_T / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}
// torch's abs().max() propagates NaN; fmax drops it.  A NaN anywhere makes the sum of absolute values NaN, which the
// callers use to put it back.
__device__ __forceinline__ double nan_max(double mx, double l1) { return l1 != l1 ? l1 : mx; }

__device__ __forceinline__ bool lbl_off(const LblPtrs& p) { return p.c->done != 0 || p.c->P != p.P; }
__device__ __forceinline__ bool lbl_no_accept(const LblPtrs& p) { return lbl_off(p) || p.c->action < PINN_LBFGS_ACT_ACCEPT; }

__device__ __forceinline__ float* lbl_S(const LblPtrs& p) { return (float*)p.hist; }
__device__ __forceinline__ int64_t lbl_rowbytes(const LblPtrs& p) { return ((int64_t)p.c->m * p.P * 4 + 255) & ~(int64_t)255; }
__device__ __forceinline__ float* lbl_Y(const LblPtrs& p) { return (float*)(p.hist + lbl_rowbytes(p)); }
__device__ __forceinline__ double* lbl_M(const LblPtrs& p) { return (double*)(p.hist + 2 * lbl_rowbytes(p)); }

__global__ void k_lbl_init(pinn_lbfgs_ctrl* c, int64_t P, pinn_lbfgs_opts o) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  c->phase = 0; c->done = 0; c->reason = PINN_LBFGS_STOP_NONE; c->action = PINN_LBFGS_ACT_INERT;
  c->head = 0; c->k = 0; c->slot = 0; c->m = o.history_size;
  c->n_iter = 0; c->n_evals = 0; c->max_iter = o.max_iter; c->max_eval = o.max_eval;
  c->push = 0; c->file_row = 0; c->acc_row = 0; c->n_slots = 0;
  c->P = P;
  c->t = 0.0; c->f = 0.0; c->gtd = 0.0; c->d_norm = 0.0; c->H = 1.0; c->f_prev = 0.0; c->t_acc = 0.0; c->gmax = 0.0;
  c->lr = o.lr; c->tolerance_grad = o.tolerance_grad; c->tolerance_change = o.tolerance_change;
  ls_init(&c->ls, 0.0, 0.0, 0.0, 0.0, 0);
}

__global__ void k_lbl_trial(LblPtrs p, int n_sums) {
  const bool off = lbl_off(p);
  const bool first = p.c->phase == 0;
  const float tf = (float)p.c->t;
  if (blockIdx.x == 0 && (int)threadIdx.x < n_sums) p.sums[threadIdx.x] = 0.f;
  for (int64_t e = (int64_t)blockIdx.x * LBL_T + threadIdx.x; e < p.P; e += (int64_t)gridDim.x * LBL_T) {
    p.gnew[e] = 0.f;                  // (also in an inert slot: the pass still adds into it)
    if (!off) p.xt[e] = first ? p.params[e] : fmaf(tf, p.d[e], p.params[e]);
  }
}

__global__ void k_lbl_dots(LblPtrs p) {
  if (lbl_off(p)) return;
  __shared__ double red[LBL_T];
  double a = 0.0;
  if (p.c->phase != 0)
    for (int64_t e = (int64_t)blockIdx.x * LBL_T + threadIdx.x; e < p.P; e += (int64_t)gridDim.x * LBL_T)
      a += (double)p.gnew[e] * (double)p.d[e];
  a = blk_sum(a, red);
  if (threadIdx.x == 0) p.part[blockIdx.x * LBL_PART] = a;
}

__global__ void k_lbl_control(LblPtrs p, int nb, int n_cols, int n_terms, int n_loss_rows, const float* __restrict__ loss_rows,
                              int total_row, double* __restrict__ trace) {
#pragma clang fp contract(off)
  __shared__ double red[LBL_T];
  if (trace)
    for (int j = threadIdx.x; j < PINN_LBFGS_TRACE_COLS; j += LBL_T) trace[j] = 0.0;
  pinn_lbfgs_ctrl* c = p.c;
  if (lbl_off(p)) {
    if (threadIdx.x == 0 && c->P == p.P) c->action = PINN_LBFGS_ACT_INERT;
    return;
  }
  const double gtd_new = blk_sum((int)threadIdx.x < nb ? p.part[threadIdx.x * LBL_PART] : 0.0, red);
  // the weighted losses as k_finish_adam forms them: double accumulation over [col sums | term sums], one rounding
  if ((int)threadIdx.x < n_loss_rows) {
    double a = 0.0;
    for (int j = 0; j < n_cols + n_terms; ++j) a += (double)loss_rows[threadIdx.x * (n_cols + n_terms) + j] * (double)p.sums[j];
    p.losses[threadIdx.x] = (float)a;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double f_new = (double)p.losses[total_row];
  c->n_evals += 1;
  c->n_slots += 1;
  const double t_eval = c->phase == 0 ? 0.0 : c->t;
  int action;
  if (c->phase == 0) {
    action = PINN_LBFGS_ACT_INITIAL;
    c->file_row = 0; c->acc_row = 0; c->t_acc = 0.0; c->f = f_new;
  } else {
    c->file_row = c->ls.g_slot_for_new;
    if (ls_step(&c->ls, f_new, gtd_new) == PINN_LS_EVALUATE) {
      action = PINN_LBFGS_ACT_CONTINUE;
      c->t = c->ls.t;
    } else {
      action = PINN_LBFGS_ACT_ACCEPT;
      c->acc_row = c->ls.g_acc_slot; c->t_acc = c->ls.t_acc; c->f = c->ls.f_acc;
    }
  }
  c->action = action;
  c->push = 0;
  if (trace) {
    trace[0] = (double)c->n_evals; trace[1] = (double)c->n_iter; trace[2] = (double)action;
    trace[3] = t_eval; trace[4] = f_new; trace[5] = gtd_new;
    if (action >= PINN_LBFGS_ACT_ACCEPT) { trace[7] = c->t_acc; trace[8] = c->f; }
    for (int r = 0; r < n_loss_rows; ++r) trace[10 + r] = (double)p.losses[r];
  }
}

// partials: 0 y.s, 1 y.y, 2 max|g|, 3 max|s|, 4 |g|_1
__global__ void k_lbl_accept1(LblPtrs p) {
  if (lbl_off(p)) return;
  const int action = p.c->action;
  if (action == PINN_LBFGS_ACT_INERT) return;
  __shared__ double red[LBL_T];
  const int file_row = p.c->file_row, acc_row = p.c->acc_row;
  const bool accept = action == PINN_LBFGS_ACT_ACCEPT, fresh = action >= PINN_LBFGS_ACT_ACCEPT;
  const float tf = (float)p.c->t_acc;
  float* frow = p.pool + (int64_t)file_row * p.P;
  const float* arow = p.pool + (int64_t)acc_row * p.P;
  double ys = 0.0, yy = 0.0, gmax = 0.0, smax = 0.0, l1 = 0.0;
  for (int64_t e = (int64_t)blockIdx.x * LBL_T + threadIdx.x; e < p.P; e += (int64_t)gridDim.x * LBL_T) {
    const float gn = p.gnew[e];
    frow[e] = gn;
    if (!fresh) continue;
    const float ga = acc_row == file_row ? gn : arow[e];
    if (accept) {
      const float dd = p.d[e];
      const float sv = dd * tf;                      // d.mul(t)
      const float yv = ga - p.prevg[e];              // g.sub(prev_g)
      p.params[e] = fmaf(tf, dd, p.params[e]);       // the very expression of k_lbl_trial: the iterate IS the trial evaluated
      p.sv[e] = sv; p.yv[e] = yv;
      ys += (double)yv * (double)sv; yy += (double)yv * (double)yv;
      smax = fmax(smax, fabs((double)sv));
    }
    if (acc_row != 0) p.pool[e] = ga;                // row 0: the gradient of the iterate
    p.prevg[e] = ga;
    gmax = fmax(gmax, fabs((double)ga));
    l1 += fabs((double)ga);
  }
  ys = blk_sum(ys, red); yy = blk_sum(yy, red); l1 = blk_sum(l1, red);
  gmax = blk_max(gmax, red); smax = blk_max(smax, red);
  if (threadIdx.x == 0) {
    double* o = p.part + blockIdx.x * LBL_PART;
    o[0] = ys; o[1] = yy; o[2] = gmax; o[3] = smax; o[4] = l1;
  }
}

__device__ void lbl_stop(pinn_lbfgs_ctrl* c, int reason, double* trace) {
  c->done = 1; c->reason = reason; c->action = PINN_LBFGS_ACT_INERT;
  if (trace) trace[6] = (double)reason;
}

__global__ void k_lbl_accept2(LblPtrs p, int nb, double* __restrict__ trace) {
#pragma clang fp contract(off)
  if (lbl_no_accept(p)) return;
  __shared__ double red[LBL_T];
  const bool in = (int)threadIdx.x < nb;
  const double* o = p.part + threadIdx.x * LBL_PART;
  const double ys = blk_sum(in ? o[0] : 0.0, red), yy = blk_sum(in ? o[1] : 0.0, red), l1 = blk_sum(in ? o[4] : 0.0, red);
  const double gmax = nan_max(blk_max(in ? o[2] : 0.0, red), l1);
  const double smax = nan_max(blk_max(in ? o[3] : 0.0, red), ys);
  if (threadIdx.x != 0) return;
  pinn_lbfgs_ctrl* c = p.c;
  c->gmax = gmax;
  if (trace) { trace[9] = gmax; trace[1] = (double)c->n_iter; }
  if (c->action == PINN_LBFGS_ACT_INITIAL) {
    if (gmax <= c->tolerance_grad) return lbl_stop(c, PINN_LBFGS_STOP_GRADIENT, trace);
    if (!(c->n_iter < c->max_iter)) return lbl_stop(c, PINN_LBFGS_STOP_MAX_ITER, trace);
    c->n_iter += 1;
    c->H = 1.0;
    c->t = py_min(1.0, 1.0 / l1) * c->lr;
  } else {
    if (c->n_iter == c->max_iter) return lbl_stop(c, PINN_LBFGS_STOP_MAX_ITER, trace);
    if (c->n_evals >= c->max_eval) return lbl_stop(c, PINN_LBFGS_STOP_MAX_EVAL, trace);
    if (gmax <= c->tolerance_grad) return lbl_stop(c, PINN_LBFGS_STOP_GRADIENT, trace);
    if (smax <= c->tolerance_change) return lbl_stop(c, PINN_LBFGS_STOP_STEP, trace);
    if (fabs(c->f - c->f_prev) < c->tolerance_change) return lbl_stop(c, PINN_LBFGS_STOP_LOSS, trace);
    c->n_iter += 1;
    if (ys > 1e-10) {
      c->push = 1;
      if (c->k == c->m) { c->slot = c->head; c->head = (c->head + 1) % c->m; }      // overwrite the oldest pair
      else { c->slot = (c->head + c->k) % c->m; c->k += 1; }
      c->H = ys / yy;
    }
    c->t = c->lr;
  }
  c->f_prev = c->f;
  if (trace) trace[1] = (double)c->n_iter;
}

// workgroups 0 .. LBL_MAX_M-1: row / column `slot` of M (workgroup j: physical row j); the rest copy (s, y) into row `slot`.
// No workgroup reads row `slot` of S or Y here: workgroup `slot` takes s and y themselves, the same numbers.
__global__ void k_lbl_push(LblPtrs p) {
  if (lbl_no_accept(p) || !p.c->push) return;
  const int m = p.c->m, slot = p.c->slot;
  float* S = lbl_S(p); float* Y = lbl_Y(p);
  if ((int)blockIdx.x < LBL_MAX_M) {
    const int j = blockIdx.x;
    if (j >= m) return;
    lb_push_dots_body(j == slot ? p.sv : S + (int64_t)j * p.P, j == slot ? p.yv : Y + (int64_t)j * p.P, p.sv, p.yv, j, slot, m,
                      p.P, lbl_M(p));
    return;
  }
  float* Ss = S + (int64_t)slot * p.P; float* Ys = Y + (int64_t)slot * p.P;
  const int64_t nbc = gridDim.x - LBL_MAX_M;
  for (int64_t e = (int64_t)(blockIdx.x - LBL_MAX_M) * LBL_T + threadIdx.x; e < p.P; e += nbc * LBL_T) {
    Ss[e] = p.sv[e]; Ys[e] = p.yv[e];
  }
}

// which = 0: b = -(S g);  1: c = Y q     (tmp: b | al | c | w, m doubles each; coef: alf | wf)
__global__ void k_lbl_rowdots(LblPtrs p, int which) {
  if (lbl_no_accept(p)) return;
  const int m = p.c->m;
  if ((int)blockIdx.x >= m) return;
  const float* A = (which == 0 ? lbl_S(p) : lbl_Y(p)) + (int64_t)blockIdx.x * p.P;
  lb_rowdots_body(A, which == 0 ? p.pool : p.q, which == 0 ? -1.0 : 1.0, p.P, p.tmp + (which == 0 ? 0 : 2 * m) + blockIdx.x);
}
__global__ void k_lbl_solve_upper(LblPtrs p) {
  if (lbl_no_accept(p)) return;
  const int m = p.c->m;
  lb_solve_upper_body(lbl_M(p), p.tmp, p.c->head, p.c->k, m, p.tmp + m, p.coef);
}
__global__ void k_lbl_solve_lower(LblPtrs p) {
  if (lbl_no_accept(p)) return;
  const int m = p.c->m;
  lb_solve_lower_body(lbl_M(p), p.tmp + m, p.tmp + 2 * m, p.c->H, p.c->head, p.c->k, m, p.tmp + 3 * m, p.coef + m);
}
// which = 0: q = -g - Y^T al;  1: d = H q + S^T w
__global__ void k_lbl_combine(LblPtrs p, int which) {
  if (lbl_no_accept(p)) return;
  const int m = p.c->m;
  if (which == 0) lb_combine_body(p.pool, -1.f, lbl_Y(p), p.coef, -1.f, m, p.P, p.q);
  else lb_combine_body(p.q, (float)p.c->H, lbl_S(p), p.coef + m, 1.f, m, p.P, p.d);
}

// partials: 0 g . d, 1 max|d|, 2 |d|_1 (NaN carrier)
__global__ void k_lbl_gtd(LblPtrs p) {
  if (lbl_no_accept(p)) return;
  __shared__ double red[LBL_T];
  double a = 0.0, mx = 0.0, l1 = 0.0;
  for (int64_t e = (int64_t)blockIdx.x * LBL_T + threadIdx.x; e < p.P; e += (int64_t)gridDim.x * LBL_T) {
    const double dd = (double)p.d[e];
    a += (double)p.pool[e] * dd;
    mx = fmax(mx, fabs(dd)); l1 += fabs(dd);
  }
  a = blk_sum(a, red); l1 = blk_sum(l1, red); mx = blk_max(mx, red);
  if (threadIdx.x == 0) { double* o = p.part + blockIdx.x * LBL_PART; o[0] = a; o[1] = mx; o[2] = l1; }
}

__global__ void k_lbl_arm(LblPtrs p, int nb, double* __restrict__ trace) {
  if (lbl_no_accept(p)) return;
  __shared__ double red[LBL_T];
  const bool in = (int)threadIdx.x < nb;
  const double* o = p.part + threadIdx.x * LBL_PART;
  const double gtd = blk_sum(in ? o[0] : 0.0, red), l1 = blk_sum(in ? o[2] : 0.0, red);
  const double d_norm = nan_max(blk_max(in ? o[1] : 0.0, red), l1);
  if (threadIdx.x != 0) return;
  pinn_lbfgs_ctrl* c = p.c;
  c->gtd = gtd; c->d_norm = d_norm;
  if (gtd > -c->tolerance_change) return lbl_stop(c, PINN_LBFGS_STOP_DIRECTION, trace);
  ls_init(&c->ls, c->f, gtd, c->t, d_norm, c->max_eval - c->n_evals);
  c->phase = 1;
}

inline int lbl_grid(int64_t P) {
  const int64_t nb = (P + LBL_T - 1) / LBL_T;
  return (int)(nb < 1 ? 1 : nb > LBL_NB ? LBL_NB : nb);
}

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

LblPtrs lbl_ptrs(void* state, float* params, int64_t P) {
  const LblLayout L = lbl_layout(P, 1);
  char* b = (char*)state;
  LblPtrs p;
  p.c = (pinn_lbfgs_ctrl*)b; p.params = params;
  p.d = (float*)(b + L.d); p.xt = (float*)(b + L.xt); p.gnew = (float*)(b + L.gnew); p.pool = (float*)(b + L.pool);
  p.prevg = (float*)(b + L.prevg); p.sv = (float*)(b + L.sv); p.yv = (float*)(b + L.yv); p.q = (float*)(b + L.q);
  p.part = (double*)(b + L.part); p.sums = (float*)(b + L.sums); p.losses = (float*)(b + L.losses);
  p.tmp = (double*)(b + L.tmp); p.coef = (float*)(b + L.coef); p.hist = b + L.hist; p.P = P;
  return p;
}

int lbl_init(void* state, int64_t state_bytes, int64_t P, const pinn_lbfgs_opts& o, hipStream_t s) {
  const LblLayout L = lbl_layout(P, o.history_size);
  if (hipMemsetAsync(state, 0, (size_t)L.total, s) != hipSuccess) { set_error("pinn_lbfgs_loop_init: memset failed"); return PINN_ERR_LAUNCH; }
  hipLaunchKernelGGL(k_lbl_init, dim3(1), dim3(64), 0, s, (pinn_lbfgs_ctrl*)state, P, o);
  return check_launch("lbfgs loop init");
}

int lbl_before_pass(const LblPtrs& p, int n_sums, hipStream_t s) {
  hipLaunchKernelGGL(k_lbl_trial, dim3(lbl_grid(p.P)), dim3(LBL_T), 0, s, p, n_sums);
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
