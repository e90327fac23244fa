// common.h — shared host/device declarations for libpinn_hip.so
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdarg.h>
#include <stdio.h>
#include "../../include/pinn_hip.h"

namespace pinn {

void set_error(const char* fmt, ...);

inline int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }   // workspace regions start on 256-byte boundaries

// layer geometry helpers: layers = [d_in] + [width]*n_hidden + [d_out] (train.py:56)
constexpr int FUSED_KERNEL_AUTO = 0, FUSED_KERNEL_TILE = 1, FUSED_KERNEL_COOP = 2, FUSED_KERNEL_BATCH = 3;
struct Net {
  int d_in, d_out, L /*hidden layers*/, W, k, K1, act, prec;
  int fused_kernel;  // FUSED_KERNEL_*: which fused kernel desc.engine asked for (PINN_ENGINE_FUSED_TILE / _COOP / _BATCH)
  float drop_p;      // nn.Dropout rate in training mode (dnn.py:38), 0 = off
  uint32_t drop_seed, drop_thresh;   // keep unit iff dropout_bits(...) >= drop_thresh (= p * 2^32)
  int dir_col[PINN_MAX_DIRS];
  int n_lin;  // L + 1 linear layers
  __host__ __device__ int in_dim(int l) const { return l == 0 ? d_in : W; }
  __host__ __device__ int out_dim(int l) const { return l == L ? d_out : W; }
  __host__ __device__ int64_t w_off(int l) const {  // offset of W_l in the flat parameter vector (O(1): 100-layer nets)
    if (l == 0) return 0;
    const int64_t hid = (int64_t)d_in * W + W + (int64_t)((l <= L ? l : L) - 1) * ((int64_t)W * W + W);   // layer 0 + hidden blocks
    return l <= L ? hid : hid + (int64_t)W * d_out + d_out;                                        // l == L + 1: the total
  }
  __host__ __device__ int layer_of(int64_t i) const {   // which layer's block holds flat parameter index i
    const int64_t s0 = (int64_t)d_in * W + W, per = (int64_t)W * W + W;
    if (i < s0) return 0;
    const int64_t l = 1 + (i - s0) / per;
    return l < L ? (int)l : L;
  }
  __host__ __device__ int64_t b_off(int l) const { return w_off(l) + (int64_t)in_dim(l) * out_dim(l); }
  __host__ __device__ int64_t n_params() const { return w_off(L + 1); }
};

int make_net(const pinn_desc* d, Net* n);  // validates, returns PINN_OK or error

// Counter-based dropout mask (two rounds of the murmur3 finaliser over (seed, point) then (layer, feature)):
// 32 uniform bits per (seed, hidden layer, unit, point); the unit is kept iff bits >= p * 2^32.  Stateless, so
// the reverse sweep re-derives the forward's mask from the same seed (no mask storage, any launch geometry).
__host__ __device__ inline uint32_t dropout_fmix(uint32_t x) {
  x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
  return x;
}
__host__ __device__ inline uint32_t dropout_bits(uint32_t seed, uint32_t layer, uint32_t feature, uint64_t point) {
  uint32_t x = dropout_fmix(seed ^ ((uint32_t)point * 0x9E3779B1u));
  x ^= (layer * 0x01000193u + feature) * 0x9E3779B1u + (uint32_t)(point >> 32);
  return dropout_fmix(x);
}
__host__ __device__ inline uint32_t dropout_threshold(float p) {
  const double t = (double)p * 4294967296.0;
  return t >= 4294967295.0 ? 4294967295u : (uint32_t)t;
}

// torch.optim.Adam's scalars, formed in double as Python forms them and cast to fp32 once (adam_scalars, reduce_adam.h)
struct AdamScalars { float w1, b2, w2, eps, step_size, bc2_sqrt; };   // 1 - b1, b2, 1 - b2, eps, lr / bc1, sqrt(bc2)

// pinn_residual_spec.flags bit 0 on PINN_RES_PHYSICS_EQUATION (the corrected radiation stress, residuals.h:
// ResPhysicsEquationCorrected) travels inside the library as a residual id of its own: check_spec (pinn_abi.hip) writes it
// into the NORMALISED spec, no caller can pass it and pinn_hip.h does not know it.
constexpr int RES_PE_CORRECTED = 5;
// ... and bits 0 and 1 together (the corrected residual closed by the dispersion relation and the wave-energy balance,
// residuals.h: ResPhysicsEquationWave; param[0] = omega, param[1] = gamma) the same way
constexpr int RES_PE_WAVE = 6;
// the fused engine's partial-sum rows keep the fifth term's sum in the slot of the eighth fidelity column (fused_kernel.h, term_slot)
constexpr int WAVE_MAX_COLS = PINN_MAX_ROLES - 1;
// either of the two: what the engines serve alike (the engine rule, the split request at every width, no cooperative kernel)
inline bool is_pe_closure(int residual_id) { return residual_id == RES_PE_CORRECTED || residual_id == RES_PE_WAVE; }
// how a refusal names the request's closure (flags: the caller's spec.flags)
inline const char* pe_closure_name(bool wave) {
  return wave ? "the wave closure (spec.flags bits 0 and 1: corrected radiation stress, dispersion and wave-energy terms)"
              : "the corrected radiation stress (spec.flags bit 0)";
}

// what a loss call asks the engines for
// torch.optim.Adam's update folded into the kernel that finishes a loss + gradient pass (pinn_loss_grad_adam_step)
struct AdamReq {
  float* params;        // updated in place (the pass itself read the PACKED copy of them in the workspace)
  float* m; float* v;
  AdamScalars c;        // the scalars pinn_adam_step hands k_adam
  bool packed_valid;    // the workspace's packed weights already equal params (left there by the previous call)
  int n_loss_rows; const float* loss_rows; float* losses;   // optional weighted loss values (see pinn_adam_state)
};

struct LossReq {
  int kind;  // 0 = residual, 1 = mse, 2 = residual + mse in one pass
  int64_t n_split;  // kind 2: < 0 both terms on every point; >= 0 residual on points [0, n_split), mse on [n_split, N)
  pinn_residual_spec spec;
  const float* scale;   // residual: device term_scale (may be null when !want_grad)
  float* sums;          // residual: device term_sums
  int n_terms;          // residual: number of terms
  // mse
  const float* T; int n_cols; int out_col[PINN_MAX_ROLES];
  const float* mse_scale;   // device col_scale
  float* mse_sums;          // device col_sums
  float* grad;          // device flat grad (+=) or null
  const AdamReq* adam;  // fused engine only: grad is OVERWRITTEN with this pass's gradient and the update applied
  // pinn_residual_coef_loss_grad only (kind 0, no adam; null everywhere else): the residual's closure coefficients, a device
  // array of n_coef floats, and where their gradient goes (n_coef floats, +=; null = not wanted)
  const float* coef; float* coef_grad; int n_coef;
  // pinn_residual_weighted_loss_grad only (kind 0, no adam; null everywhere else): the point weights, a device array
  // (w_rows, N) with row stride w_stride (0: one row for every term, N: a row per weighted term); n_weighted = the
  // residual's weighted terms; fields_out: null or the (n_fields, N) array of the unweighted signed fields (overwritten)
  const float* point_w; int64_t w_stride; int n_weighted; float* fields_out;
};

// generic engine (pinn_generic.hip)
int64_t generic_workspace_bytes(const Net& n, int64_t N);
int generic_forward(const Net& n, const float* params, const float* X, int64_t N, float* Y, float* dY,
                    void* ws, int64_t ws_bytes, hipStream_t s);
int generic_jet_backward(const Net& n, const float* params, const float* X, int64_t N, const float* gY,
                         const float* gdY, float* grad, void* ws, int64_t ws_bytes, hipStream_t s);
int generic_loss(const Net& n, const LossReq& rq, const float* params, const float* X, int64_t N,
                 void* ws, int64_t ws_bytes, hipStream_t s);

// second-order jets (pinn_jet2.hip): generic VALU layer kernels, or MFMA layer kernels (mfma = true) where
// jet2_mfma_supports(); one workspace layout serves both
int64_t jet2_workspace_bytes(const Net& n, int64_t N);
bool jet2_mfma_supports(const Net& n);
int jet2_forward(const Net& n, bool mfma, const float* params, const float* X, int64_t N, float* Y, float* dY,
                 float* d2Y, void* ws, int64_t ws_bytes, hipStream_t s);
int jet2_backward(const Net& n, bool mfma, const float* params, const float* X, int64_t N, const float* gY,
                  const float* gdY, const float* gd2Y, float* grad, void* ws, int64_t ws_bytes, hipStream_t s);

// pinn_residual2_loss_grad (pinn_jet2.hip): the residual with the lateral-mixing term nu * lap(U) on the second-order jets,
// forward chunk -> k2_residual -> backward chunk; mfma = the MFMA layer kernels and k2m_wgrad, else the VALU kernels and
// k2_wgrad.  spec is normalised (check_spec) and names a residual with a momentum equation; fields and grad may be null.
int64_t residual2_workspace_bytes(const Net& n, int64_t N);
int residual2_loss_grad(const Net& n, bool mfma, const pinn_residual_spec& spec, float nu, const float* scale,
                        const float* params, const float* X, int64_t N, float* sums, float* fields, float* grad,
                        void* ws, int64_t ws_bytes, hipStream_t s);

// fused MFMA engine (pinn_fused.hip)
bool fused_supports(const Net& n, bool want_grad);
bool fused_supports_adam(const Net& n, const LossReq& rq, int64_t N);   // one-pass requests only
int64_t fused_workspace_bytes(const Net& n, int64_t N);
int fused_forward(const Net& n, const float* params, const float* X, int64_t N, float* Y, float* dY,
                  void* ws, int64_t ws_bytes, hipStream_t s);
int fused_loss(const Net& n, const LossReq& rq, const float* params, const float* X, int64_t N,
               void* ws, int64_t ws_bytes, hipStream_t s);
// Ensembles (pinn_ensemble_*): M networks of one shape through the tile kernel's ensemble instances (fused_kernel.h,
// k_fused_ens), one launch for all members.  rq (and rq.adam) hold the BASE pointers of the (M, .) arrays: params, grad, m, v
// (M, P); sums (M, n_terms); mse_sums (M, n_cols); losses (M, n_loss_rows).  flags: PINN_ENSEMBLE_OWN_X / _OWN_T.
// fused_ensemble_refusal: why the request has no ensemble kernel, or nullptr (pure host logic): the descriptor's part is
// fused_tile_refusal(TILE_ENSEMBLE, n), the request's the corrected radiation stress and the split request at width 33..64.
const char* fused_ensemble_refusal(const Net& n, const LossReq& rq);
// the per-member grid gx, whether a workgroup's gradient copy lives in LDS, and the workspace of M members on N points
void fused_ensemble_plan(const Net& n, int M, int64_t N, int* gx, int* copy_in_lds, int64_t* ws_bytes);
int fused_ensemble_loss(const Net& n, const LossReq& rq, int M, int flags, const float* params, const float* X, int64_t N,
                        void* ws, int64_t ws_bytes, hipStream_t s);
// The tile kernel's families of instances beside the plain forward / loss ones: external adjoint (pinn_jet_backward, EPI_ADJ),
// per-point fields (EPI_FIELD), runtime coefficients (EPI_COEF), point weights (EPI_WEIGHTED), ensembles (k_fused_ens).
// fused_tile_refusal: why the descriptor has no instance in the family, or nullptr = served (pure host logic; the text
// lives in a per-thread buffer until the next call).  One rule, pinn_fused.hip; "supports" is !refusal.
// (TILE_BALANCE: no instances of its own — the plain gradient instances, as pinn_adam_loop_balanced serves them)
enum { TILE_ADJ, TILE_FIELD, TILE_COEF, TILE_WEIGHTED, TILE_ENSEMBLE, TILE_BALANCE };
const char* fused_tile_refusal(int family, const Net& n);
// which fused kernel a served pinn_jet_backward request runs: PINN_ENGINE_FUSED_TILE or PINN_ENGINE_FUSED_BATCH (pure host
// logic: the decision run() itself takes)
int fused_jet_backward_kernel(const Net& n, int64_t N);
// pinn_jet_backward on the tile kernel (fused_kernel.h, EPI_ADJ): grad += d/dtheta [sum(gY * Y) + sum(gdY * dY)]
int fused_jet_backward(const Net& n, const float* params, const float* X, int64_t N, const float* gY,
                       const float* gdY, float* grad, void* ws, int64_t ws_bytes, hipStream_t s);

// whether the fused engine serves a corrected-radiation-stress loss or field request (RES_PE_CORRECTED); if not, why not
const char* fused_corrected_refusal(const Net& n);
// pinn_residual_fields on the tile kernel (fused_kernel.h, EPI_FIELD): fields (NF, N) of the residual in `spec`
int64_t fused_fields_workspace_bytes(const Net& n);
int fused_residual_fields(const Net& n, const pinn_residual_spec& spec, const float* params, const float* X, int64_t N,
                          float* fields, void* ws, int64_t ws_bytes, hipStream_t s);
// ... and from a staged jet (pinn_fields.hip): Y (n, d_out), dY (k, n, d_out) of points [n0, n0 + n) -> fields[f * N + n0 + i]
int fields_from_jet(const Net& net, const pinn_residual_spec& spec, const float* X, const float* Y, const float* dY,
                    int64_t n, int64_t n0, int64_t N, float* fields, hipStream_t s);

// pinn_residual_coef_loss_grad / pinn_residual_weighted_loss_grad on the tile kernel's coefficient / weighted instances
// (family TILE_COEF: rq.coef set; TILE_WEIGHTED: rq.point_w set): the workspace of a served call (-1: not served), the call
int64_t fused_tile_workspace_bytes(int family, const Net& n, int64_t N);
int fused_tile_loss(int family, const Net& n, const LossReq& rq, const float* params, const float* X, int64_t N, void* ws,
                    int64_t ws_bytes, hipStream_t s);

// wide MFMA engine, 64 < W <= 256 (pinn_wide.hip)
bool wide_supports(const Net& n);
int64_t wide_workspace_bytes(const Net& n, int64_t N);
int wide_forward(const Net& n, const float* params, const float* X, int64_t N, float* Y, float* dY,
                 void* ws, int64_t ws_bytes, hipStream_t s);
int wide_loss(const Net& n, const LossReq& rq, const float* params, const float* X, int64_t N,
              void* ws, int64_t ws_bytes, hipStream_t s);

// compute units of the CURRENT device (cached per device ordinal: one process may drive several GPUs)
int device_cu_count();
// raise a kernel's dynamic-LDS limit above 64 KB, once per (kernel, device) instead of on every launch
int ensure_dynamic_lds(const void* kernel, size_t lds_bytes);

// the caller's workspace must hold `need` bytes: every engine's check before its first launch, and the message's one place
inline int check_workspace(const void* ws, int64_t ws_bytes, int64_t need) {
  if (ws && ws_bytes >= need) return PINN_OK;
  set_error("workspace too small: need %lld bytes, got %lld", (long long)need, (long long)ws_bytes);
  return PINN_ERR_WORKSPACE;
}

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: launch failed: %s", what, hipGetErrorString(e));
    return PINN_ERR_LAUNCH;
  }
  return PINN_OK;
}

}  // namespace pinn
