// pinn_balance.hip — pinn_balance_update (include/pinn_hip.h): the statistics of G flat gradients, the weight update and the
// weighted combination, in at most three small launches.  Independent of engine and descriptor.
#include "balance.h"

namespace pinn {

// Stage 1, grid (nb, G): block (b, j) folds entries b * 256 + t, (b + nb) * 256 + t, ... of group j in that order per
// thread, then a fixed tree over the block: partials[b][j] = (max|g|, sum|g|, sum g^2) in double.  g^2 is exact in double
// (24 x 24 bits), so S and Q carry the rounding of the additions alone.
__global__ void k_balance_stats(const float* __restrict__ grads, int64_t P, int64_t ld, int G, double* __restrict__ partials) {
#pragma clang fp contract(off)
  const int j = blockIdx.y, nb = gridDim.x;
  const float* __restrict__ g = grads + (int64_t)j * ld;
  double a = 0.0, s = 0.0, q = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < P; i += (int64_t)nb * 256) {
    const double v = (double)g[i], av = fabs(v);
    a = balance_nanmax(a, av);
    s += av;
    q += v * v;
  }
  balance_block_reduce(a, s, q);
  if (threadIdx.x == 0) {
    double* out = partials + ((int64_t)blockIdx.x * G + j) * PINN_BALANCE_STATS;
    out[BAL_A] = a; out[BAL_S] = s; out[BAL_Q] = q;
  }
}

// Stage 2, one block of 256 threads
__global__ void k_balance_weights(int mode, int G, int ref, double alpha, int64_t P, const double* __restrict__ partials, int nb,
                                  float* __restrict__ lam, double* __restrict__ stats) {
  balance_finish(mode, G, ref, alpha, P, partials, nb, lam, stats);
}

// grad_out[i] = ((lam[0] g_0[i]) + (lam[1] g_1[i])) + ..., group order, no fused multiply-add
__global__ void k_balance_combine(const float* __restrict__ grads, int64_t P, int64_t ld, int G, const float* __restrict__ lam,
                                  float* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  float acc = lam[0] * grads[i];
  for (int j = 1; j < G; ++j) {
    const float t = lam[j] * grads[(int64_t)j * ld + i];
    acc = acc + t;
  }
  out[i] = acc;
}

int64_t balance_workspace_bytes(int64_t P, int G) {
  return align256((int64_t)balance_blocks(P) * G * PINN_BALANCE_STATS * (int64_t)sizeof(double));
}

int balance_update(int mode, int G, int ref, double alpha, const float* grads, int64_t P, int64_t ld, float* lam, double* stats,
                   float* grad_out, void* ws, hipStream_t s) {
  if (mode != PINN_BALANCE_NONE) {
    const int nb = balance_blocks(P);
    hipLaunchKernelGGL(k_balance_stats, dim3(nb, G), dim3(256), 0, s, grads, P, ld, G, (double*)ws);
    hipLaunchKernelGGL(k_balance_weights, dim3(1), dim3(256), 0, s, mode, G, ref, alpha, P, (const double*)ws, nb, lam, stats);
  }
  if (grad_out)
    hipLaunchKernelGGL(k_balance_combine, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, grads, P, ld, G, (const float*)lam,
                       grad_out);
  return check_launch("pinn_balance_update");
}

}  // namespace pinn
