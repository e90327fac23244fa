// lbfgs_loop.h — host interface of pinn_lbfgs_loop.hip: the layout of `state` and the launches around the pass of one slot.
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

// device pointers of one call (kernel arguments hold only pointers and sizes: every scalar lives in the control block)
struct LblPtrs {
  pinn_lbfgs_ctrl* c;
  float *params, *d, *xt, *gnew, *pool, *prevg, *sv, *yv, *q;
  double* part;
  float *sums, *losses;
  double* tmp;
  float* coef;
  char* hist;
  int64_t P;
};
LblPtrs lbl_ptrs(void* state, float* params, int64_t P);

int lbl_init(void* state, int64_t state_bytes, int64_t P, const pinn_lbfgs_opts& o, hipStream_t s);
// before the pass: x_trial, zeroed gradient and sums.  After it: controller and the accept path.
int lbl_before_pass(const LblPtrs& p, int n_sums, hipStream_t s);
int lbl_after_pass(const LblPtrs& p, int n_cols, int n_terms, int n_loss_rows, const float* loss_rows, int total_row,
                   double* trace_row, hipStream_t s);

}  // namespace pinn
#endif
