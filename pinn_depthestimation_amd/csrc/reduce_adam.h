// reduce_adam.h — what follows a loss pass on every engine, once: the fixed-order column sum over per-workgroup rows of
// partial sums, and torch.optim.Adam's update.  The folded Adam iteration (k_finish_adam, pinn_fused.hip) equals the
// separate calls (k_reduce_sums, k_adam) bit for bit because both run the functions below.
#pragma once
#include <math.h>
#include "common.h"

namespace pinn {

// Sum of column t over n_rows rows of `stride` floats, in double and in a fixed order (thread j adds rows j, j + 256, ...;
// then a 128 ... 1 tree), so the result does not depend on scheduling.  Called by all 256 threads of a block; every
// thread gets the sum.  A second call must be separated from the readers of the first by a __syncthreads().
__device__ __forceinline__ double column_sum(const float* __restrict__ rows, int64_t n_rows, int stride, int t) {
  __shared__ double red[256];
  double v = 0.0;
  for (int64_t b = threadIdx.x; b < n_rows; b += 256) v += (double)rows[b * stride + t];
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

// launches k_reduce_sums (pinn_abi.hip): out[j] = column_sum of column col0 + j, j < n; one block per column
void reduce_sums(const float* rows, int64_t n_rows, int stride, int col0, int n, float* out, hipStream_t s);
// ... and its accumulating form (k_reduce_sums_add): out[j] += the same sum (pinn_residual_coef_loss_grad's coef_grad)
void reduce_sums_add(const float* rows, int64_t n_rows, int stride, int col0, int n, float* out, hipStream_t s);

// torch.optim.Adam, _single_tensor_adam (the path train.py:192 takes on CPU):
//   exp_avg.lerp_(grad, 1-b1); exp_avg_sq.mul_(b2).addcmul_(grad, grad, value=1-b2)
//   denom = (exp_avg_sq.sqrt() / sqrt(bc2)).add_(eps); param.addcdiv_(exp_avg, denom, value=-lr/bc1)
// Scalars are formed in double on the host exactly as Python does, then cast to
// fp32 once; contraction is off so every op rounds where torch's rounds.
inline AdamScalars adam_scalars(double lr, double beta1, double beta2, double eps, int64_t step) {
  const double bc1 = 1.0 - pow(beta1, (double)step);
  const double bc2 = 1.0 - pow(beta2, (double)step);
  return AdamScalars{(float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps, (float)(lr / bc1), (float)sqrt(bc2)};
}
// updates m and v in place and returns the new parameter
__device__ __forceinline__ float adam_update(float p, float gi, float& m, float& v, const AdamScalars& c) {
#pragma clang fp contract(off)
  const float mi = m + c.w1 * (gi - m);
  float vi = v * c.b2;
  vi = vi + (c.w2 * gi) * gi;
  m = mi; v = vi;
  const float denom = sqrtf(vi) / c.bc2_sqrt + c.eps;
  return p - c.step_size * (mi / denom);
}

}  // namespace pinn
