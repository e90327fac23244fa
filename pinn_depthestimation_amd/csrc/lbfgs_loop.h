// lbfgs_loop.h — host interface of pinn_lbfgs_loop.hip and pinn_lbfgs_ens.hip: the layout of `state` and the launches around
// the pass of one slot, for one network and for an ensemble of M.
#ifndef PINN_LBFGS_LOOP_H
#define PINN_LBFGS_LOOP_H
#include "common.h"

namespace pinn {

constexpr int LBL_NB = 256;        // workgroups of the element-wise / partial-sum kernels at most
constexpr int LBL_PART = 8;        // doubles per workgroup in the partials
constexpr int LBL_MAX_M = 256;     // history rows the recursion kernels serve
constexpr int LBL_MAX_SUMS = 2 * PINN_MAX_ROLES;

// Byte offsets into `state`.  Everything up to `hist` does not depend on the history size: the host needs only P to find
// it.  S, Y and M follow at hist, hist + rowbytes, hist + 2 rowbytes with rowbytes = align256(m * P * 4): the kernels
// form those from the control block's m.
struct LblLayout {
  int64_t d, xt, gnew, pool, prevg, sv, yv, q, part, sums, losses, tmp, coef, hist, total;
};
LblLayout lbl_layout(int64_t P, int m);

// device pointers of one network (kernel arguments hold only pointers and sizes: every scalar lives in the control block).
// csums | tsums: the fidelity column sums and the residual term sums the pass writes (single loop: one vector, tsums =
// csums + n_cols; ensemble: member rows of two matrices).  m: the history size the recursion grids were sized by, which
// must then be the control block's, or 0 where they serve LBL_MAX_M rows (the single loop).
struct LblPtrs {
  pinn_lbfgs_ctrl* c;
  float *params, *d, *xt, *gnew, *pool, *prevg, *sv, *yv, *q;
  double* part;
  float *csums, *tsums, *losses;
  double* tmp;
  float* coef;
  char* hist;
  int64_t P;
  int m;
};
LblPtrs lbl_ptrs(void* state, float* params, int64_t P, int n_cols);

int lbl_init(void* state, int64_t state_bytes, int64_t P, const pinn_lbfgs_opts& o, hipStream_t s);
// before the pass: x_trial, zeroed gradient and sums.  After it: controller and the accept path.
int lbl_before_pass(const LblPtrs& p, int n_cols, int n_terms, hipStream_t s);
int lbl_after_pass(const LblPtrs& p, int n_cols, int n_terms, int n_loss_rows, const float* loss_rows, int total_row,
                   double* trace_row, hipStream_t s);

// ---- the ensemble loop (pinn_lbfgs_ens.hip): M networks, one schedule of launches ------------------------------------------
// Byte offsets into the ensemble state (include/pinn_hip.h states the formula).  Shared matrices first — the M control
// blocks at stride `ctrl_stride`, d, x_trial and g_new (M, P), the column sums and the term sums (M, PINN_MAX_ROLES floats
// reserved each; rows of the request's n_cols / n_terms) — then M member blocks of `mem_stride` bytes, each laid out by
// `in`: what only the member's own kernels touch.
struct LbeMember {
  int64_t pool, prevg, sv, yv, q, part, losses, tmp, coef, hist, total;
};
struct LbeLayout {
  int64_t ctrl_stride, d, xt, gnew, csums, tsums, mem, mem_stride, total;
  LbeMember in;
};
LbeLayout lbe_layout(int M, int64_t P, int m);

// what every k_lbe_* kernel gets: member blockIdx.y's LblPtrs are formed from it on the device
struct LbePtrs {
  char* state;
  float* params;         // (M, P)
  int64_t P;
  int M, m;              // m: history_size, by which grid.x of the recursion kernels is sized
  int n_cols, n_terms;   // row lengths of the column sums and the term sums
  LbeLayout L;
};
LbePtrs lbe_ptrs(void* state, float* params, int M, int64_t P, int m, int n_cols, int n_terms);
inline float* lbe_xt(const LbePtrs& e) { return (float*)(e.state + e.L.xt); }
inline float* lbe_gnew(const LbePtrs& e) { return (float*)(e.state + e.L.gnew); }
inline float* lbe_csums(const LbePtrs& e) { return (float*)(e.state + e.L.csums); }
inline float* lbe_tsums(const LbePtrs& e) { return (float*)(e.state + e.L.tsums); }

int lbe_init(void* state, int M, int64_t P, const pinn_lbfgs_opts& o, hipStream_t s);
int lbe_before_pass(const LbePtrs& e, hipStream_t s);
// trace_rows: this slot's (M, PINN_LBFGS_TRACE_COLS) doubles, or null
int lbe_after_pass(const LbePtrs& e, int n_loss_rows, const float* loss_rows, int total_row, double* trace_rows, hipStream_t s);

}  // namespace pinn
#endif
