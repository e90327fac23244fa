// lbfgs_loop_bodies.h — the bodies of the device L-BFGS loop's kernels as __device__ functions, shared by the single-network
// kernels of pinn_lbfgs_loop.hip (k_lbl_*: one LblPtrs as the launch argument) and by the ensemble kernels of
// pinn_lbfgs_ens.hip (k_lbe_*: member blockIdx.y's LblPtrs formed from base pointers and strides).  One body, two ways to be
// told where a network's state lives: the state machine, the stopping tests and the ring bookkeeping exist once.
//
//   lbl_trial_body     x_trial = x + t d; zeroes the gradient buffer and the sums the pass adds into
//   lbl_dots_body      per-workgroup partial sums of g_new . d
//   lbl_control_body   one workgroup: fixed-order fp64 combine, the weighted losses, ls_step, the trace row
//   lbl_accept1_body   files g_new in its pool row; on ACCEPT: x += t* d, s, y, prev_g, partials of y.s, y.y, max|g|, max|s|
//   lbl_accept2_body   one workgroup: the stopping tests, the ring bookkeeping, H (first iteration: t = min(1, 1/|g|_1) lr)
//   lbl_push_body      rows and columns of M for the new pair, and its copy into S, Y
//   lbl_rowdots_body / lbl_solve_upper_body / lbl_combine_body / lbl_solve_lower_body
//                      the recursion of pinn_lbfgs.hip (lbfgs_recursion.h), head / k / H from the control block
//   lbl_gtd_body       partials of g . d and max|d|
//   lbl_arm_body       one workgroup: the g.d test, ls_init
//
// Every body returns at once when the done flag is up; every body from lbl_accept2_body's successors on returns unless the
// slot is an accept.  No atomics: reductions are per-workgroup partials (a fixed grid for a given P) combined by one
// workgroup in a fixed order, so the loop is reproducible wherever the pass is.  Sized for P up to 2^20 + 3 and beyond
// (grid-stride, 64-bit offsets) and m <= 256.  blockIdx.x / gridDim.x are the network's own grid in both forms.
#ifndef PINN_LBFGS_LOOP_BODIES_H
#define PINN_LBFGS_LOOP_BODIES_H
#include "lbfgs_loop.h"
#include "lbfgs_line_search.h"
#include "lbfgs_recursion.h"

namespace pinn {

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

// (p.m: the history size the recursion grids were sized by, 0 where they serve LBL_MAX_M rows whatever m is)
__device__ __forceinline__ bool lbl_off(const LblPtrs& p) {
  return p.c->done != 0 || p.c->P != p.P || (p.m != 0 && p.c->m != p.m);
}
__device__ __forceinline__ bool lbl_no_accept(const LblPtrs& p) { return lbl_off(p) || p.c->action < PINN_LBFGS_ACT_ACCEPT; }
__device__ __forceinline__ int lbl_rows(const LblPtrs& p) { return p.m != 0 ? p.m : LBL_MAX_M; }

__device__ __forceinline__ float* lbl_S(const LblPtrs& p) { return (float*)p.hist; }
__device__ __forceinline__ int64_t lbl_rowbytes(const LblPtrs& p) { return ((int64_t)p.c->m * p.P * 4 + 255) & ~(int64_t)255; }
__device__ __forceinline__ float* lbl_Y(const LblPtrs& p) { return (float*)(p.hist + lbl_rowbytes(p)); }
__device__ __forceinline__ double* lbl_M(const LblPtrs& p) { return (double*)(p.hist + 2 * lbl_rowbytes(p)); }

// one thread
__device__ __forceinline__ void lbl_init_body(pinn_lbfgs_ctrl* c, int64_t P, const pinn_lbfgs_opts& o) {
  c->phase = 0; c->done = 0; c->reason = PINN_LBFGS_STOP_NONE; c->action = PINN_LBFGS_ACT_INERT;
  c->head = 0; c->k = 0; c->slot = 0; c->m = o.history_size;
  c->n_iter = 0; c->n_evals = 0; c->max_iter = o.max_iter; c->max_eval = o.max_eval;
  c->push = 0; c->file_row = 0; c->acc_row = 0; c->n_slots = 0;
  c->P = P;
  c->t = 0.0; c->f = 0.0; c->gtd = 0.0; c->d_norm = 0.0; c->H = 1.0; c->f_prev = 0.0; c->t_acc = 0.0; c->gmax = 0.0;
  c->lr = o.lr; c->tolerance_grad = o.tolerance_grad; c->tolerance_change = o.tolerance_change;
  ls_init(&c->ls, 0.0, 0.0, 0.0, 0.0, 0);
}

__device__ __forceinline__ void lbl_trial_body(const LblPtrs& p, int n_cols, int n_terms) {
  const bool off = lbl_off(p);
  const bool first = p.c->phase == 0;
  const float tf = (float)p.c->t;
  if (blockIdx.x == 0) {
    if ((int)threadIdx.x < n_cols) p.csums[threadIdx.x] = 0.f;
    if ((int)threadIdx.x < n_terms) p.tsums[threadIdx.x] = 0.f;
  }
  for (int64_t e = (int64_t)blockIdx.x * LBL_T + threadIdx.x; e < p.P; e += (int64_t)gridDim.x * LBL_T) {
    p.gnew[e] = 0.f;                  // (also in an inert slot: the pass still adds into it)
    if (!off) p.xt[e] = first ? p.params[e] : fmaf(tf, p.d[e], p.params[e]);
  }
}

__device__ __forceinline__ void lbl_dots_body(const LblPtrs& p) {
  if (lbl_off(p)) return;
  __shared__ double red[LBL_T];
  double a = 0.0;
  if (p.c->phase != 0)
    for (int64_t e = (int64_t)blockIdx.x * LBL_T + threadIdx.x; e < p.P; e += (int64_t)gridDim.x * LBL_T)
      a += (double)p.gnew[e] * (double)p.d[e];
  a = blk_sum(a, red);
  if (threadIdx.x == 0) p.part[blockIdx.x * LBL_PART] = a;
}

__device__ __forceinline__ void lbl_control_body(const LblPtrs& p, int nb, int n_cols, int n_terms, int n_loss_rows,
                                                 const float* __restrict__ loss_rows, int total_row, double* __restrict__ trace) {
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
    for (int j = 0; j < n_cols + n_terms; ++j)
      a += (double)loss_rows[threadIdx.x * (n_cols + n_terms) + j] * (double)(j < n_cols ? p.csums[j] : p.tsums[j - n_cols]);
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
__device__ __forceinline__ void lbl_accept1_body(const LblPtrs& p) {
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
      p.params[e] = fmaf(tf, dd, p.params[e]);       // the very expression of lbl_trial_body: the iterate IS the trial evaluated
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

__device__ __forceinline__ void lbl_stop(pinn_lbfgs_ctrl* c, int reason, double* trace) {
  c->done = 1; c->reason = reason; c->action = PINN_LBFGS_ACT_INERT;
  if (trace) trace[6] = (double)reason;
}

__device__ __forceinline__ void lbl_accept2_body(const LblPtrs& p, int nb, double* __restrict__ trace) {
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

// workgroups 0 .. lbl_rows-1: row / column `slot` of M (workgroup j: physical row j); the rest copy (s, y) into row `slot`.
// No workgroup reads row `slot` of S or Y here: workgroup `slot` takes s and y themselves, the same numbers.
__device__ __forceinline__ void lbl_push_body(const LblPtrs& p) {
  if (lbl_no_accept(p) || !p.c->push) return;
  const int m = p.c->m, slot = p.c->slot, rows = lbl_rows(p);
  float* S = lbl_S(p); float* Y = lbl_Y(p);
  if ((int)blockIdx.x < rows) {
    const int j = blockIdx.x;
    if (j >= m) return;
    lb_push_dots_body(j == slot ? p.sv : S + (int64_t)j * p.P, j == slot ? p.yv : Y + (int64_t)j * p.P, p.sv, p.yv, j, slot, m,
                      p.P, lbl_M(p));
    return;
  }
  float* Ss = S + (int64_t)slot * p.P; float* Ys = Y + (int64_t)slot * p.P;
  const int64_t nbc = gridDim.x - rows;
  for (int64_t e = (int64_t)(blockIdx.x - rows) * LBL_T + threadIdx.x; e < p.P; e += nbc * LBL_T) {
    Ss[e] = p.sv[e]; Ys[e] = p.yv[e];
  }
}

// which = 0: b = -(S g);  1: c = Y q     (tmp: b | al | c | w, m doubles each; coef: alf | wf)
__device__ __forceinline__ void lbl_rowdots_body(const LblPtrs& p, int which) {
  if (lbl_no_accept(p)) return;
  const int m = p.c->m;
  if ((int)blockIdx.x >= m) return;
  const float* A = (which == 0 ? lbl_S(p) : lbl_Y(p)) + (int64_t)blockIdx.x * p.P;
  lb_rowdots_body(A, which == 0 ? p.pool : p.q, which == 0 ? -1.0 : 1.0, p.P, p.tmp + (which == 0 ? 0 : 2 * m) + blockIdx.x);
}
__device__ __forceinline__ void lbl_solve_upper_body(const LblPtrs& p) {
  if (lbl_no_accept(p)) return;
  const int m = p.c->m;
  lb_solve_upper_body(lbl_M(p), p.tmp, p.c->head, p.c->k, m, p.tmp + m, p.coef);
}
__device__ __forceinline__ void lbl_solve_lower_body(const LblPtrs& p) {
  if (lbl_no_accept(p)) return;
  const int m = p.c->m;
  lb_solve_lower_body(lbl_M(p), p.tmp + m, p.tmp + 2 * m, p.c->H, p.c->head, p.c->k, m, p.tmp + 3 * m, p.coef + m);
}
// which = 0: q = -g - Y^T al;  1: d = H q + S^T w
__device__ __forceinline__ void lbl_combine_body(const LblPtrs& p, int which) {
  if (lbl_no_accept(p)) return;
  const int m = p.c->m;
  if (which == 0) lb_combine_body(p.pool, -1.f, lbl_Y(p), p.coef, -1.f, m, p.P, p.q);
  else lb_combine_body(p.q, (float)p.c->H, lbl_S(p), p.coef + m, 1.f, m, p.P, p.d);
}

// partials: 0 g . d, 1 max|d|, 2 |d|_1 (NaN carrier)
__device__ __forceinline__ void lbl_gtd_body(const LblPtrs& p) {
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

__device__ __forceinline__ void lbl_arm_body(const LblPtrs& p, int nb, double* __restrict__ trace) {
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

// workgroups of the element-wise / partial-sum kernels for P parameters
inline int lbl_grid(int64_t P) {
  const int64_t nb = (P + LBL_T - 1) / LBL_T;
  return (int)(nb < 1 ? 1 : nb > LBL_NB ? LBL_NB : nb);
}

}  // namespace pinn
#endif
