// lbfgs_recursion.h — the bodies of the five recursion kernels of pinn_lbfgs.hip as __device__ functions, shared by the
// launch-argument entries there (head, k, slot, H come from the host) and by the device-argument forms of
// pinn_lbfgs_loop.hip (the same values read from the control block).  One body, two ways to be told the ring's state.
#ifndef PINN_LBFGS_RECURSION_H
#define PINN_LBFGS_RECURSION_H
#include "common.h"

namespace pinn {

constexpr int LB_T = 256;

// out[row] = sign * sum_e a[e] * x[e]   (one workgroup per row; fp64 combine)
__device__ __forceinline__ void lb_rowdots_body(const float* __restrict__ a, const float* __restrict__ x, double sign, int64_t P,
                                                double* __restrict__ out_row) {
  float acc = 0.f;
  for (int64_t e = threadIdx.x; e < P; e += LB_T) acc = fmaf(a[e], x[e], acc);
  __shared__ double red[LB_T];
  red[threadIdx.x] = (double)acc;
  __syncthreads();
  for (int s = LB_T / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out_row = sign * red[0];
}

// M[slot][j] = s . Yj ;  M[j][slot] = Sj . y   (Sj, Yj: physical row j, which for j == slot holds s, y)
__device__ __forceinline__ void lb_push_dots_body(const float* __restrict__ Sj, const float* __restrict__ Yj,
                                                  const float* __restrict__ s, const float* __restrict__ y, int j, int slot,
                                                  int m, int64_t P, double* __restrict__ M) {
  float a0 = 0.f, a1 = 0.f;
  for (int64_t e = threadIdx.x; e < P; e += LB_T) {
    a0 = fmaf(s[e], Yj[e], a0);
    a1 = fmaf(Sj[e], y[e], a1);
  }
  __shared__ double r0[LB_T], r1[LB_T];
  r0[threadIdx.x] = (double)a0; r1[threadIdx.x] = (double)a1;
  __syncthreads();
  for (int t = LB_T / 2; t > 0; t >>= 1) {
    if (threadIdx.x < t) { r0[threadIdx.x] += r0[threadIdx.x + t]; r1[threadIdx.x] += r1[threadIdx.x + t]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    M[(int64_t)slot * m + j] = r0[0];
    M[(int64_t)j * m + slot] = r1[0];
  }
}

__device__ inline double lb_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return __shfl(v, 0, 64);
}

// one wave: al (logical i = k-1 .. 0):  al_i = (b_i - sum_{j>i} al_j M[pi][pj]) / M[pi][pi]
__device__ __forceinline__ void lb_solve_upper_body(const double* __restrict__ M, const double* __restrict__ b, int head, int k,
                                                    int m, double* __restrict__ al, float* __restrict__ alf) {
  const int lane = threadIdx.x;
  for (int j = lane; j < m; j += 64) { al[j] = 0.0; alf[j] = 0.f; }
  __syncthreads();
  for (int i = k - 1; i >= 0; --i) {
    const int pi = (head + i) % m;
    double part = 0.0;
    for (int j = i + 1 + lane; j < k; j += 64) {
      const int pj = (head + j) % m;
      part += al[pj] * M[(int64_t)pi * m + pj];
    }
    const double s = lb_wave_sum(part);
    if (lane == 0) {
      const double v = (b[pi] - s) / M[(int64_t)pi * m + pi];
      al[pi] = v; alf[pi] = (float)v;
    }
    __syncthreads();
  }
}

// one wave: w (logical i = 0 .. k-1):  w_i = (M_ii al_i - H c_i - sum_{j<i} w_j M[pj][pi]) / M_ii
__device__ __forceinline__ void lb_solve_lower_body(const double* __restrict__ M, const double* __restrict__ al,
                                                    const double* __restrict__ c, double H, int head, int k, int m,
                                                    double* __restrict__ w, float* __restrict__ wf) {
  const int lane = threadIdx.x;
  for (int j = lane; j < m; j += 64) { w[j] = 0.0; wf[j] = 0.f; }
  __syncthreads();
  for (int i = 0; i < k; ++i) {
    const int pi = (head + i) % m;
    double part = 0.0;
    for (int j = lane; j < i; j += 64) {
      const int pj = (head + j) % m;
      part += w[pj] * M[(int64_t)pj * m + pi];
    }
    const double s = lb_wave_sum(part);
    if (lane == 0) {
      const double mii = M[(int64_t)pi * m + pi];
      const double v = (mii * al[pi] - H * c[pi] - s) / mii;
      w[pi] = v; wf[pi] = (float)v;
    }
    __syncthreads();
  }
}

// out[e] = alpha * base[e] + sign * sum_row coef[row] * A[row][e]    (rows with coef == 0 are unused slots)
__device__ __forceinline__ void lb_combine_body(const float* __restrict__ base, float alpha, const float* __restrict__ A,
                                                const float* __restrict__ coef, float sign, int m, int64_t P,
                                                float* __restrict__ out) {
  __shared__ float cf[256];
  for (int j = threadIdx.x; j < m; j += LB_T) cf[j] = coef[j];
  __syncthreads();
  const int64_t e = (int64_t)blockIdx.x * LB_T + threadIdx.x;
  if (e >= P) return;
  float acc = 0.f;
  for (int r = 0; r < m; ++r) acc = fmaf(cf[r], A[(int64_t)r * P + e], acc);
  out[e] = fmaf(alpha, base[e], sign * acc);
}

}  // namespace pinn
#endif
