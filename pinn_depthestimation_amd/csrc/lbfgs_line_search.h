// lbfgs_line_search.h — torch's _strong_wolfe (torch/optim/lbfgs.py) as a resumable state machine, one source for the
// host entries (pinn_lbfgs_ls_init / _step, pinn_abi.hip) and for the controller kernel (pinn_lbfgs_loop.hip).
//
// torch's function calls obj_func from three places (the first trial, the bracketing loop, the zoom loop); here every
// such call is a return of PINN_LS_EVALUATE with the trial in st->t, and ls_step resumes right behind it with the two
// numbers the evaluation gave.  Branch for branch torch's code, comparisons written as torch writes them so that NaN and
// inf take the same branches; Python's min / max of two numbers are py_min / py_max below (the FIRST argument wins ties
// and unordered comparisons).  All scalars are double; c1 = 1e-4, c2 = 0.9, tolerance_change = 1e-9 as
// lbfgs.FlatLBFGS.step calls it.  The returned point is the LOW end of the bracket, not the last point evaluated.
//
// No vectors: the gradients torch clones into g_prev / bracket_g are ROWS of a pool the caller keeps.  Row 0 is the
// gradient at t = 0 and is never written; the gradient of the trial about to be evaluated goes to row g_slot_for_new,
// always one of rows 1..3 that neither the previous point nor a bracket end occupies.  Four rows suffice: during
// bracketing {0, prev, new}, during zoom {0, bracket[0], bracket[1], new} with row 0 possibly one of the bracket ends.
#ifndef PINN_LBFGS_LINE_SEARCH_H
#define PINN_LBFGS_LINE_SEARCH_H
#include <math.h>
#include "../../include/pinn_hip.h"

#if defined(__HIPCC__)
#define PINN_LS_HD __host__ __device__ inline
#else
#define PINN_LS_HD inline
#endif

namespace pinn {

constexpr double LS_C1 = 1e-4, LS_C2 = 0.9, LS_TOL_CHANGE = 1e-9;

// Python's max(a, b) / min(a, b): b replaces a only if b > a (b < a)
PINN_LS_HD double py_max(double a, double b) { return b > a ? b : a; }
PINN_LS_HD double py_min(double a, double b) { return b < a ? b : a; }

// _cubic_interpolate; has_bounds = 0: the bounds are the two points in order
PINN_LS_HD double ls_cubic(double x1, double f1, double g1, double x2, double f2, double g2, int has_bounds, double lo,
                           double hi) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double xmin_bound, xmax_bound;
  if (has_bounds) { xmin_bound = lo; xmax_bound = hi; }
  else if (x1 <= x2) { xmin_bound = x1; xmax_bound = x2; }
  else { xmin_bound = x2; xmax_bound = x1; }
  const double d1 = g1 + g2 - 3 * (f1 - f2) / (x1 - x2);
  const double d2_square = d1 * d1 - g1 * g2;
  if (d2_square >= 0) {
    const double d2 = sqrt(d2_square);
    double min_pos;
    if (x1 <= x2) min_pos = x2 - (x2 - x1) * ((g2 + d2 - d1) / (g2 - g1 + 2 * d2));
    else min_pos = x1 - (x1 - x2) * ((g1 + d2 - d1) / (g1 - g2 + 2 * d2));
    return py_min(py_max(min_pos, xmin_bound), xmax_bound);
  }
  return (xmin_bound + xmax_bound) / 2.0;
}

// a pool row in 1..3 other than a and b
PINN_LS_HD int ls_free_row(int a, int b) {
  for (int r = 1; r < PINN_LS_POOL_ROWS; ++r)
    if (r != a && r != b) return r;
  return 1;
}

PINN_LS_HD int ls_finish(pinn_ls_state* st) {
  st->t_acc = st->br_t[st->low_pos];
  st->f_acc = st->br_f[st->low_pos];
  st->g_acc_slot = st->br_slot[st->low_pos];
  st->phase = 2;
  return PINN_LS_DONE;
}

// the head of the zoom loop, up to its obj_func call
PINN_LS_HD int ls_zoom_next(pinn_ls_state* st, int done) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (done || !(st->ls_iter < st->max_ls)) return ls_finish(st);
  if (fabs(st->br_t[1] - st->br_t[0]) * st->d_norm < LS_TOL_CHANGE) return ls_finish(st);
  double t = ls_cubic(st->br_t[0], st->br_f[0], st->br_gtd[0], st->br_t[1], st->br_f[1], st->br_gtd[1], 0, 0.0, 0.0);
  const double bmax = py_max(st->br_t[0], st->br_t[1]), bmin = py_min(st->br_t[0], st->br_t[1]);
  const double eps = 0.1 * (bmax - bmin);
  if (py_min(bmax - t, t - bmin) < eps) {
    if (st->insuf_progress || t >= bmax || t <= bmin) {
      if (fabs(t - bmax) < fabs(t - bmin)) t = bmax - eps;
      else t = bmin + eps;
      st->insuf_progress = 0;
    } else {
      st->insuf_progress = 1;
    }
  } else {
    st->insuf_progress = 0;
  }
  st->t = t;
  st->g_slot_for_new = ls_free_row(st->br_slot[0], st->br_slot[1]);
  st->phase = 1;
  return PINN_LS_EVALUATE;
}

// arms a search from (f0, gtd0) at t = 0: the first trial is t0.  max_ls as torch.optim.LBFGS.step passes it.
PINN_LS_HD int ls_init(pinn_ls_state* st, double f0, double gtd0, double t0, double d_norm, int max_ls) {
  st->f0 = f0; st->gtd0 = gtd0; st->d_norm = d_norm;
  st->t = t0;
  st->t_prev = 0.0; st->f_prev = f0; st->gtd_prev = gtd0;
  st->br_t[0] = st->br_t[1] = 0.0; st->br_f[0] = st->br_f[1] = 0.0; st->br_gtd[0] = st->br_gtd[1] = 0.0;
  st->t_acc = 0.0; st->f_acc = f0;
  st->phase = 0; st->ls_iter = 0; st->max_ls = max_ls; st->n_evals = 0;
  st->low_pos = 0; st->high_pos = 1; st->insuf_progress = 0; st->br_n = 0;
  st->g_prev_slot = 0; st->br_slot[0] = st->br_slot[1] = 0;
  st->g_slot_for_new = 1; st->g_acc_slot = 0;
  return PINN_LS_EVALUATE;
}

// (f_new, gtd_new): loss and g.d at st->t, its gradient filed in row st->g_slot_for_new
PINN_LS_HD int ls_step(pinn_ls_state* st, double f_new, double gtd_new) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (st->phase == 2) return PINN_LS_DONE;
  const double f = st->f0, gtd = st->gtd0, t = st->t;
  const int new_slot = st->g_slot_for_new;
  st->n_evals += 1;
  if (st->phase == 0) {
    int done = 0, bracketed = 0;
    if (st->ls_iter < st->max_ls) {
      if (f_new > (f + LS_C1 * t * gtd) || (st->ls_iter > 1 && f_new >= st->f_prev)) {
        bracketed = 1;
      } else if (fabs(gtd_new) <= -LS_C2 * gtd) {
        st->br_t[0] = st->br_t[1] = t; st->br_f[0] = st->br_f[1] = f_new; st->br_gtd[0] = st->br_gtd[1] = gtd_new;
        st->br_slot[0] = st->br_slot[1] = new_slot; st->br_n = 1;
        done = 1;
      } else if (gtd_new >= 0) {
        bracketed = 1;
      } else {
        // interpolate: the next trial in [t + 0.01 (t - t_prev), 10 t]
        const double min_step = t + 0.01 * (t - st->t_prev), max_step = t * 10;
        st->t = ls_cubic(st->t_prev, st->f_prev, st->gtd_prev, t, f_new, gtd_new, 1, min_step, max_step);
        st->t_prev = t; st->f_prev = f_new; st->gtd_prev = gtd_new;
        st->g_prev_slot = new_slot;                           // (the row of the point before it is free again)
        st->g_slot_for_new = ls_free_row(new_slot, new_slot);
        st->ls_iter += 1;
        return PINN_LS_EVALUATE;
      }
      if (bracketed) {
        st->br_t[0] = st->t_prev; st->br_t[1] = t;
        st->br_f[0] = st->f_prev; st->br_f[1] = f_new;
        st->br_gtd[0] = st->gtd_prev; st->br_gtd[1] = gtd_new;
        st->br_slot[0] = st->g_prev_slot; st->br_slot[1] = new_slot; st->br_n = 2;
      }
    } else {
      // reached max number of iterations: the bracket [0, t] (bracket_gtd is not read again: the zoom loop cannot run)
      st->br_t[0] = 0.0; st->br_t[1] = t;
      st->br_f[0] = f; st->br_f[1] = f_new;
      st->br_gtd[0] = gtd; st->br_gtd[1] = gtd_new;
      st->br_slot[0] = 0; st->br_slot[1] = new_slot; st->br_n = 2;
    }
    st->insuf_progress = 0;
    if (st->br_f[0] <= st->br_f[1]) { st->low_pos = 0; st->high_pos = 1; } else { st->low_pos = 1; st->high_pos = 0; }
    return ls_zoom_next(st, done);
  }
  // zoom phase, behind its obj_func call
  st->ls_iter += 1;
  int done = 0;
  const int lo = st->low_pos, hi = st->high_pos;
  if (f_new > (f + LS_C1 * t * gtd) || f_new >= st->br_f[lo]) {
    st->br_t[hi] = t; st->br_f[hi] = f_new; st->br_gtd[hi] = gtd_new; st->br_slot[hi] = new_slot;
    if (st->br_f[0] <= st->br_f[1]) { st->low_pos = 0; st->high_pos = 1; } else { st->low_pos = 1; st->high_pos = 0; }
  } else {
    if (fabs(gtd_new) <= -LS_C2 * gtd) {
      done = 1;
    } else if (gtd_new * (st->br_t[hi] - st->br_t[lo]) >= 0) {
      st->br_t[hi] = st->br_t[lo]; st->br_f[hi] = st->br_f[lo]; st->br_gtd[hi] = st->br_gtd[lo];
      st->br_slot[hi] = st->br_slot[lo];
    }
    st->br_t[lo] = t; st->br_f[lo] = f_new; st->br_gtd[lo] = gtd_new; st->br_slot[lo] = new_slot;
  }
  return ls_zoom_next(st, done);
}

}  // namespace pinn
#endif
