// balance.h — gradient-statistics loss balancing (include/pinn_hip.h: pinn_balance_weights_host, pinn_balance_update,
// pinn_adam_loop_balanced).  The update rule, once, for the host entry and for the kernels (the pattern of
// pinn_residual2_point / pinn_pe_corrected_point), the statistics' block and final reductions, and what pinn_abi.hip
// (validation) hands pinn_fused.hip (passes + statistics + the finishing kernel) for the device-enqueued runs.
#pragma once
#include <math.h>
#include "common.h"

namespace pinn {

// per group: A = max|g|, S = sum|g|, Q = sum g^2 (PINN_BALANCE_STATS doubles)
constexpr int BAL_A = 0, BAL_S = 1, BAL_Q = 2;

// max that keeps a NaN (fmax drops it): a NaN on either side is the result
__host__ __device__ inline double balance_nanmax(double a, double b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }

// lam_out[j] <- (float)((1 - alpha) lam_in[j] + alpha lam_hat[j]) where lam_hat[j] is a finite positive number, else
// lam_in[j] bit for bit.  MAX_MEAN: lam_hat[j] = A[ref] / (S[j] / P), j != ref (lam[ref] is left alone);
// NORM: lam_hat[j] = (sum_i sqrt(Q[i])) / sqrt(Q[j]), the sum in group order.  Everything in double, contraction off,
// one rounding to fp32.  The arguments were validated by the caller (mode, G, ref, alpha, P).
__host__ __device__ inline void balance_weights(int mode, int G, int ref, double alpha, int64_t P, const double* stats,
                                                const float* lam_in, float* lam_out) {
#pragma clang fp contract(off)
  double total = 0.0;
  if (mode == PINN_BALANCE_NORM)
    for (int i = 0; i < G; ++i) total = i == 0 ? sqrt(stats[i * PINN_BALANCE_STATS + BAL_Q]) : total + sqrt(stats[i * PINN_BALANCE_STATS + BAL_Q]);
  for (int j = 0; j < G; ++j) {
    const float cur = lam_in[j];
    float out = cur;
    if (mode == PINN_BALANCE_NORM || (mode == PINN_BALANCE_MAX_MEAN && j != ref)) {
      const double hat = mode == PINN_BALANCE_NORM
                             ? total / sqrt(stats[j * PINN_BALANCE_STATS + BAL_Q])
                             : stats[ref * PINN_BALANCE_STATS + BAL_A] / (stats[j * PINN_BALANCE_STATS + BAL_S] / (double)P);
      // finite and positive (a NaN fails both comparisons)
      if (hat > 0.0 && hat <= 1.7976931348623157e308) {
        const double keep = (1.0 - alpha) * (double)cur;
        const double move = alpha * hat;
        out = (float)(keep + move);
      }
    }
    lam_out[j] = out;
  }
}

// rows of per-block partial statistics a pass over P entries leaves per group (pinn_balance_update): fixed by P alone
inline int balance_blocks(int64_t P) {
  const int64_t nb = (P + 2047) / 2048;
  return (int)(nb < 1 ? 1 : (nb > 64 ? 64 : nb));
}

#ifdef __HIPCC__
// One block's statistics of the values its threads hold (a = |g| or 0, s = |g|, q = g^2, as doubles; threads without a
// value pass zeros): a 128 ... 1 tree in a fixed order.  Called by all 256 threads; thread 0 gets the result in a, s, q.
// A second call must be separated from the first by a __syncthreads().
__device__ __forceinline__ void balance_block_reduce(double& a, double& s, double& q) {
  __shared__ double red[PINN_BALANCE_STATS][256];
  red[BAL_A][threadIdx.x] = a; red[BAL_S][threadIdx.x] = s; red[BAL_Q][threadIdx.x] = q;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      red[BAL_A][threadIdx.x] = balance_nanmax(red[BAL_A][threadIdx.x], red[BAL_A][threadIdx.x + w]);
      red[BAL_S][threadIdx.x] += red[BAL_S][threadIdx.x + w];
      red[BAL_Q][threadIdx.x] += red[BAL_Q][threadIdx.x + w];
    }
    __syncthreads();
  }
  a = red[BAL_A][0]; s = red[BAL_S][0]; q = red[BAL_Q][0];
}

// The second stage: partials (nb, G, 3) -> stats (G, 3) in shared memory, one statistic at a time — thread t folds rows
// t, t + 256, ... in that order, then a 128 ... 1 tree: a fixed order for a given nb — then thread 0 applies the rule to lam
// in place and, if asked, copies the statistics out.  One block of 256 threads.  (A single thread per statistic walking all
// rows was measured first: 464 dependent double additions behind 464 loads cost 90 us on the 8x64 network.)
__device__ __forceinline__ void balance_finish(int mode, int G, int ref, double alpha, int64_t P,
                                               const double* __restrict__ partials, int nb, float* __restrict__ lam,
                                               double* __restrict__ stats_out) {
  __shared__ double st[PINN_BALANCE_MAX_GROUPS * PINN_BALANCE_STATS];
  __shared__ double red[256];
  const int t = threadIdx.x;
  for (int e = 0; e < G * PINN_BALANCE_STATS; ++e) {
    const bool is_max = e % PINN_BALANCE_STATS == BAL_A;
    double acc = 0.0;          // (the identity of both folds: every statistic is >= 0 or NaN)
    for (int b = t; b < nb; b += 256) {
      const double v = partials[(int64_t)b * G * PINN_BALANCE_STATS + e];
      acc = is_max ? balance_nanmax(acc, v) : acc + v;
    }
    red[t] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (t < w) red[t] = is_max ? balance_nanmax(red[t], red[t + w]) : red[t] + red[t + w];
      __syncthreads();
    }
    if (t == 0) st[e] = red[0];
    __syncthreads();
  }
  if (t == 0) {
    float in[PINN_BALANCE_MAX_GROUPS], out[PINN_BALANCE_MAX_GROUPS];
    for (int j = 0; j < G; ++j) in[j] = lam[j];
    balance_weights(mode, G, ref, alpha, P, st, in, out);
    for (int j = 0; j < G; ++j) lam[j] = out[j];
    if (stats_out) for (int j = 0; j < G * PINN_BALANCE_STATS; ++j) stats_out[j] = st[j];
  }
}
#endif

// pinn_adam_loop_balanced: what pinn_abi.hip hands pinn_fused.hip
struct AdamBalReq {
  LossReq res;          // the plain residual pass (kind 0); sums = term_sums, grad = grad_flat (OVERWRITTEN by the finishing kernel)
  LossReq fid;          // the fidelity pass (kind 1)
  const float* Xf; int64_t N_fid;
  AdamReq adam;         // params, m, v, packed_valid and the loss rows (c is not read)
  double beta1, beta2, eps; int64_t step;
  int row_cols; float* col_sums;
  int mode, every, ref; double alpha;
  float* lam; float* lam_log; double* stats_log; float* group_grads;
  int n_iters; const double* lr;   // HOST array (n_iters)
};

// why the fused engine does not run the balanced loop on this network, or nullptr (pure host logic)
const char* fused_adam_bal_refusal(const Net& n);
int64_t fused_adam_bal_workspace_bytes(const Net& n, int64_t N_res, int64_t N_fid);
int fused_adam_bal(const Net& n, const AdamBalReq& q, const float* X, int64_t N_res, void* ws, int64_t ws_bytes, hipStream_t s);

// pinn_balance_update's kernels (pinn_balance.hip); the arguments were validated by the entry
int64_t balance_workspace_bytes(int64_t P, int G);
int balance_update(int mode, int G, int ref, double alpha, const float* grads, int64_t P, int64_t ld, float* lam, double* stats,
                   float* grad_out, void* ws, hipStream_t s);

}  // namespace pinn
