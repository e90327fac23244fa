// pinn_fields.hip — pinn_residual_fields for every request the fused tile kernel's field instances do not serve (hidden
// width above 64, the generic engine, dropout, bf16 operands): the descriptor's own forward jet is staged chunk by chunk
// (pinn_abi.hip) and this point-wise kernel turns each chunk into fields with the formulas of residuals.h — the same
// RES::fields the tile kernel's epilogue calls.  fp32 whatever the precision mode of the jet.
#include <type_traits>
#include "common.h"
#include "residuals.h"

namespace pinn {

namespace {

struct FieldsJetParams {
  const float* X; const float* Y; const float* dY;   // X: the chunk's rows (n, d_in); Y (n, d_out); dY (k, n, d_out)
  float* fields;                                     // (NF, N): this chunk writes columns [n0, n0 + n)
  int64_t n, n0, N;
  int d_in, d_out;
  int out_col[PINN_MAX_ROLES];
  int dir_of[PINN_MAX_DIRS];
  int anchor_on, xcol;
  float thr, anchor;
};

// The residual's closure (residuals.h) from the parameter block — the one place here that knows which residual takes what:
// continuity its anchor switch, point i's mask and the anchor value; the wave closure (omega, gamma) = spec.param[0..1],
// which arrive as (thr, anchor); the others nothing.
template <class RES>
__device__ inline typename RES::Closure residual_closure(const FieldsJetParams& P, int64_t i) {
  if constexpr (std::is_same<RES, ResContinuity>::value) {
    const bool masked = P.anchor_on && P.X[i * P.d_in + P.xcol] < P.thr;
    return {P.anchor_on != 0, masked, P.anchor};
  } else if constexpr (std::is_same<RES, ResPhysicsEquationWave>::value) {
    return {P.thr, P.anchor};
  } else {
    return {};
  }
}

// one thread per point: the roles' columns of the jet -> RES::fields -> fields[f * N + n0 + i]
template <class RES>
__global__ __launch_bounds__(256) void k_fields_from_jet(const FieldsJetParams P) {
  constexpr int NR = RES::NR, ND = RES::ND, NF = RES::NF;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P.n) return;
  float v[1 + ND][NR], f[NF];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int o = P.out_col[r];
    v[0][r] = P.Y[i * P.d_out + o];
#pragma unroll
    for (int d = 0; d < ND; ++d) v[1 + d][r] = P.dY[((int64_t)P.dir_of[d] * P.n + i) * P.d_out + o];
  }
  RES::fields(v, residual_closure<RES>(P, i), f);
#pragma unroll
  for (int t = 0; t < NF; ++t) P.fields[(int64_t)t * P.N + P.n0 + i] = f[t];
}

}  // namespace

int fields_from_jet(const Net& net, const pinn_residual_spec& spec, const float* X, const float* Y, const float* dY,
                    int64_t n, int64_t n0, int64_t N, float* fields, hipStream_t s) {
  FieldsJetParams P;
  P.X = X; P.Y = Y; P.dY = dY; P.fields = fields;
  P.n = n; P.n0 = n0; P.N = N;
  P.d_in = net.d_in; P.d_out = net.d_out;
  for (int r = 0; r < PINN_MAX_ROLES; ++r) P.out_col[r] = spec.out_col[r];
  for (int d = 0; d < PINN_MAX_DIRS; ++d) P.dir_of[d] = spec.dir_of[d];
  P.anchor_on = spec.residual_id == PINN_RES_CONTINUITY_ONLY ? 1 : 0;
  P.xcol = net.dir_col[spec.dir_of[0]];
  P.thr = spec.param[0]; P.anchor = spec.param[1];
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  switch (spec.residual_id) {
    case PINN_RES_NAVIER_STOKES: hipLaunchKernelGGL(k_fields_from_jet<ResNavierStokes>, grid, block, 0, s, P); break;
    case PINN_RES_PHYSICS_EQUATION: hipLaunchKernelGGL(k_fields_from_jet<ResPhysicsEquation>, grid, block, 0, s, P); break;
    case RES_PE_CORRECTED: hipLaunchKernelGGL(k_fields_from_jet<ResPhysicsEquationCorrected>, grid, block, 0, s, P); break;
    case RES_PE_WAVE: hipLaunchKernelGGL(k_fields_from_jet<ResPhysicsEquationWave>, grid, block, 0, s, P); break;
    default: hipLaunchKernelGGL(k_fields_from_jet<ResContinuity>, grid, block, 0, s, P); break;
  }
  return check_launch("fields from jet");
}

}  // namespace pinn
