// pinn_fused.hip — host side of the fused MFMA engine: weight packing, workspace carve,
// launch geometry, cross-workgroup reductions.  Kernel: fused_kernel.h.
#include <algorithm>
#include <type_traits>
#include "fused_launch.h"
#include "fused_coop_kernel.h"
#include "fused_batch_kernel.h"
#include "reduce_adam.h"
#include "adam_ext.h"
#include "balance.h"

namespace pinn {

int launch_fused_plain(int WP, const FusedParams& P, int cus, hipStream_t s);                      // pinn_fused_plain.hip
int64_t fused_plain_min_tiles(int WP, int cus);

namespace {

// a loss request with the corrected radiation stress (common.h, RES_PE_CORRECTED): its own kernel instances (EPI_PEC), on
// the tile and on the batch kernel, never on the cooperative one
// (also true for the wave closure, RES_PE_WAVE, which follows the corrected residual's rules wherever is_pec decides them:
// the split request in one pass at every width, never the cooperative kernel, no ensemble)
bool is_pec(const LossReq* rq) { return rq && rq->kind != 1 && is_pe_closure(rq->spec.residual_id); }
// ... the wave closure itself: its own instances of the tile kernel (EPI_WAVE), never the batch kernel either
bool is_wave(const LossReq* rq) { return rq && rq->kind != 1 && rq->spec.residual_id == RES_PE_WAVE; }
// a residual request with runtime closure coefficients (pinn_residual_coef_loss_grad): its own instances of the tile kernel
// (EPI_COEF), never the batch or the cooperative kernel, natural unit order
bool is_coef(const LossReq* rq) { return rq && rq->coef != nullptr; }
// a residual request with point weights (pinn_residual_weighted_loss_grad): its own instances of the tile kernel too
// (EPI_WEIGHTED), with the coefficient requests' kernel choice and grid rule
bool is_weighted(const LossReq* rq) { return rq && rq->point_w != nullptr; }

int padded_width(int W) { return W <= 16 ? 16 : (W <= 32 ? 32 : 64); }

struct Geo {
  int WP, NTH, PW, PB, PP;
  int64_t slot_floats_k4;   // per spilled layer at K1 = 4
};
Geo geo_of(const Net& n) {
  Geo g;
  g.WP = padded_width(n.W); g.NTH = g.WP / 16;
  g.PW = g.WP * 16 + (n.L - 1) * g.WP * g.WP + 16 * g.WP;
  g.PB = n.L * g.WP + 16;
  g.PP = g.PW + g.PB;
  g.slot_floats_k4 = (int64_t)4 * g.NTH * 256;
  return g;
}

int cu_count() { return device_cu_count(); }   // of the CURRENT device (common.h: cached per device)
// every launch grid of this file: `want` workgroups, at least one, at most per_cu on each compute unit
int capped_grid(int64_t want, int per_cu) {
  const int64_t cap = (int64_t)cu_count() * per_cu;
  return (int)(want < 1 ? 1 : (want < cap ? want : cap));
}
// workgroups per CU of the tile kernel where LDS allows: the width-16 instances are compiled for FUSED_W16_WAVES waves per SIMD
int tile_wgs_per_cu(int WP) { return WP == 16 ? FUSED_W16_WAVES : 2; }

constexpr int64_t LDS_LIMIT = 160 * 1024;

int64_t lds_fixed_bytes() { return (int64_t)(MAX_LOCKS + FUSED_WAVES * TB_PER_WAVE * TB_FLOATS + FUSED_WAVES * MAX_SUMS) * 4; }
bool fits_lds(const Geo& g) { return (int64_t)g.PP * 4 + lds_fixed_bytes() <= LDS_LIMIT; }

// cooperative (four waves per tile) kernel for small point sets (fused_coop_kernel.h): one workgroup
// per CU runs a tile in ~45 us against ~110 us for k_fused's one-wave tile, so it wins while there is
// at most one tile per CU (measured: loss+grad 127 -> 69 us at N = 243, 137 -> 93 us at N = 4096,
// break-even at N = 8192).  desc.engine = PINN_ENGINE_FUSED_TILE / _COOP forces one of the two (Net::fused_kernel).
int64_t coop_lds_bytes(const Net& n, const Geo& g, bool grad) {
  return ((int64_t)(grad ? g.PP : 0) + 2 * (int64_t)n.K1 * 4 * TB_FLOATS + MAX_SUMS) * 4;
}
bool use_coop(const Net& n, const Geo& g, bool grad, int64_t N) {
  const int forced = n.fused_kernel == FUSED_KERNEL_COOP ? 1 : (n.fused_kernel == FUSED_KERNEL_TILE ? 0 : -1);
  if (forced == 0 || g.WP != 64 || n.drop_p > 0.f) return false;
  if (n.act == PINN_ACT_SIN_TANH) return false;   // the sine first layer: tile-kernel instances only
  if (coop_lds_bytes(n, g, grad) > LDS_LIMIT) return false;
  if (forced == 1) return true;
  return (N + 15) / 16 <= (int64_t)cu_count();
}

// Batch kernel (fused_batch_kernel.h): narrow networks, gradient passes, enough tiles that every wave of the chip
// gets at least one full batch of FUSED_BATCH_T tiles.  desc.engine = PINN_ENGINE_FUSED_BATCH forces it at any N
// (ragged batches are handled: tiles past the end are computed on a clamped point and contribute nothing).
bool batch_supported(const Net& n, const Geo& g) {
  return n.drop_p == 0.f && g.WP <= 32 && n.L >= 1 && n.L + 1 <= MAX_LOCKS && fused_batch_has_kernel(g.WP, n.W, n.d_in, n.K1, n.act);
}
constexpr int64_t BATCH_MIN_TILES = 256;   // AUTO: below this many tiles (4096 points) the tile kernel keeps the request
// pinn_jet_backward switches at a tile count of its own (pinn_hip.h; measured: DESIGN.md 2.4b)
constexpr int64_t ADJ_BATCH_MIN_TILES = PINN_JET_BACKWARD_BATCH_MIN_TILES;
// (min_points: the loss calls count a ragged last tile, (N + 15) / 16 >= BATCH_MIN_TILES)
bool use_batch(const Net& n, const Geo& g, bool grad, int64_t N, int64_t min_points = 16 * BATCH_MIN_TILES - 15) {
  if (!grad || !batch_supported(n, g)) return false;
  if (n.fused_kernel == FUSED_KERNEL_BATCH) return true;
  if (n.fused_kernel != FUSED_KERNEL_AUTO) return false;
  return N >= min_points;
}
// ... for an external-adjoint pass: the same rule as a gradient request (the batch kernel's EPI_ADJ instances cover the
// loss instances' grid), so LeakyReLU, k = 0, d_in > 8 and width 33..64 stay on the tile kernel under every engine value
// (full tiles: N >= 16 x PINN_JET_BACKWARD_BATCH_MIN_TILES)
bool use_batch_adj(const Net& n, const Geo& g, int64_t N) { return use_batch(n, g, true, N, 16 * ADJ_BATCH_MIN_TILES); }
// tiles per wave and batch: the full batch once every wave of the chip gets one, else ONE tile per wave (the latency of
// a layer step scales with the batch, and a small point set wants its tiles spread over as many waves as there are)
int batch_T_for(const Geo& g, int K1, int64_t n_tiles) {
  const int T = batch_tiles(g.WP, K1);
  return n_tiles >= (int64_t)cu_count() * BATCH_WAVES * batch_occ(g.WP, K1) * T ? T : 1;
}
int64_t batch_lds_fixed_bytes(int WP, int K1) { return (int64_t)(BATCH_WAVES * batch_pads(WP, K1) * TB_FLOATS + BATCH_WAVES * MAX_SUMS) * 4; }
int64_t batch_lds_comb_bytes(int WP) { return (int64_t)batch_comb_floats(WP) * 4; }   // T = 1 + atomic sink: bwgrad_flush_wg's two buffers
int batch_ks(const Net& n) { return n.W <= 12 ? 3 : (n.W <= 16 ? 4 : (n.W <= 20 ? 5 : 8)); }   // k-steps of the kernel instance
int batch_grid(int64_t n_tiles, int T, int occ) {
  const int64_t nb = (n_tiles + T - 1) / T;
  return capped_grid((nb + BATCH_WAVES - 1) / BATCH_WAVES, occ);
}

int grid_for(int64_t n_tiles, bool one_per_cu, int per_cu = 2) {
  return capped_grid((n_tiles + FUSED_WAVES - 1) / FUSED_WAVES, one_per_cu ? 1 : per_cu);
}
// External-adjoint pass (pinn_jet_backward): one workgroup per TILE up to the same cap.  With the kernel's workgroup-major
// wave numbering (fused_kernel.h, EPI_ADJ) a single wave per workgroup has work while n_tiles <= grid, so every gradient
// copy is added to in program order and the call is bit-reproducible for N <= 16 x grid.
int adj_grid_for(int64_t n_tiles, bool one_per_cu, int per_cu = 2) { return capped_grid(n_tiles, one_per_cu ? 1 : per_cu); }
// the cooperative kernel: one workgroup per tile, at most one per CU for a gradient pass (it fills the LDS), else two
int coop_grid_for(int64_t n_tiles, bool grad) { return capped_grid(n_tiles, grad ? 1 : 2); }

struct WsLayout {
  int64_t wp, wtp, bp, scratch, wg_sums, wg_grads, total;
  int max_grid;
};

// lean (pinn_residual_fields: a forward-only pass that spills nothing, sums nothing and has no gradient copies): the
// packed weights only — the answer no longer depends on N.
WsLayout ws_layout(const Net& n, const Geo& g, int64_t N, bool lean = false) {
  WsLayout w;
  const int64_t n_tiles = (N + 15) / 16;
  // the largest grid any pass launches: the tile kernel's; the cooperative kernel's, one workgroup per tile (up to 2 per CU);
  // the external-adjoint pass's, also one per tile, up to the tile kernel's own cap
  const int per_cu = tile_wgs_per_cu(g.WP);
  w.max_grid = std::max({grid_for(n_tiles, false, per_cu), coop_grid_for(n_tiles, false), adj_grid_for(n_tiles, false, per_cu)});
  int64_t off = 0;
  w.wp = off; off += align256((int64_t)g.PW * 4);
  w.wtp = off; off += align256((int64_t)g.PW * 4);
  w.bp = off; off += align256((int64_t)g.PB * 4);
  int64_t scratch_bytes = (int64_t)w.max_grid * FUSED_WAVES * n.L * g.slot_floats_k4 * 4;
  if (batch_supported(n, g)) {   // the batch kernel's slots: T tiles x (L - 1) layers x K1 <= 4 x KS x 64 floats per wave
    int64_t b = 0;      // (one workspace serves the K1 = 3 and K1 = 4 instances: the larger of the two)
    for (int k1 = 3; k1 <= 4; ++k1) {
      const int T = batch_T_for(g, k1, n_tiles);
      const int64_t bk = (int64_t)batch_grid(n_tiles, T, batch_occ(g.WP, k1)) * BATCH_WAVES * T * (n.L > 1 ? n.L - 1 : 1) * k1 * batch_ks(n) * 64 * 4;
      if (bk > b) b = bk;
    }
    if (b > scratch_bytes) scratch_bytes = b;
  }
  if (lean) scratch_bytes = 0;
  w.scratch = off; off += align256(scratch_bytes);
  w.wg_sums = off; off += align256(lean ? 0 : (int64_t)w.max_grid * MAX_SUMS * 4);
  const int64_t copies = lean ? 0 : w.max_grid;   // one (padded) gradient copy per workgroup, in LDS or — too large for it — here
  w.wg_grads = off; off += align256(copies * g.PP * 4);
  w.total = off;
  return w;
}

// Which real unit sits at padded index j.  perm = 0: j itself.  perm = 1 (k_fused_batch, fused_batch_kernel.h): hidden
// units and network inputs in k-step-major order, j <-> 16*(j/16) + perm16(j%16) (an involution, so the same formula
// maps a real unit to its padded index); network outputs always stay in natural order.
__host__ __device__ inline int unit_at(int j, bool permuted) { return permuted ? (j & ~15) + perm16(j & 15) : j; }
// packing flags: PACK_PERM = the batch kernel's order (hidden units and inputs permuted, outputs natural); PACK_RMAJOR =
// register-major gradient blocks (reduction kernels only); PACK_IN / PACK_OUT = ONLY the network inputs / outputs
// permuted (k_fused<..., KRO > 0>: one k-step for the first layer, ceil(d_out / 4) for the output layer's reverse GEMM)
constexpr int PACK_PERM = 1, PACK_RMAJOR = 2, PACK_IN = 4, PACK_OUT = 8;
__host__ __device__ inline bool row_permuted(int flags, int l, int L) { return l < L ? (flags & PACK_PERM) != 0 : (flags & PACK_OUT) != 0; }
__host__ __device__ inline bool col_permuted(int flags, int l) { return (flags & PACK_PERM) != 0 || (l == 0 && (flags & PACK_IN) != 0); }

// flat torch-layout parameters -> padded row-major W, padded transposed W, padded bias: entry i of each
__device__ __forceinline__ void pack_entry(const Net& n, int WP, const float* __restrict__ params, float* __restrict__ Wp,
                                           float* __restrict__ WTp, float* __restrict__ Bp, int PW, int PB, int flags, int i) {
  if (i < PW) {
    // which layer block does padded index i fall in?
    int l, rem;
    if (i < WP * 16) { l = 0; rem = i; }
    else {
      const int j = i - WP * 16;
      l = 1 + j / (WP * WP); rem = j % (WP * WP);
      if (l > n.L) { l = n.L; rem = i - (WP * 16 + (n.L - 1) * WP * WP); }
    }
    const int inP = (l == 0) ? 16 : WP, outP = (l == n.L) ? 16 : WP;
    const int in_d = n.in_dim(l), out_d = n.out_dim(l);
    const int base = i - rem;
    {  // row-major [out][in]
      const int o = unit_at(rem / inP, row_permuted(flags, l, n.L)), c = unit_at(rem % inP, col_permuted(flags, l));
      Wp[i] = (o < out_d && c < in_d) ? params[n.w_off(l) + (int64_t)o * in_d + c] : 0.f;
    }
    {  // transposed [in][out]
      const int c = unit_at(rem / outP, col_permuted(flags, l)), o = unit_at(rem % outP, row_permuted(flags, l, n.L));
      WTp[base + rem] = (o < out_d && c < in_d) ? params[n.w_off(l) + (int64_t)o * in_d + c] : 0.f;
    }
  }
  if (i < PB) {
    int l = i / WP, o = i % WP;
    if (l >= n.L) { l = n.L; o = i - n.L * WP; }
    o = unit_at(o, row_permuted(flags, l, n.L));
    Bp[i] = (o < n.out_dim(l)) ? params[n.b_off(l) + o] : 0.f;
  }
}
__global__ void k_pack(Net n, int WP, const float* __restrict__ params, float* __restrict__ Wp,
                       float* __restrict__ WTp, float* __restrict__ Bp, int PW, int PB, int flags) {
  pack_entry(n, WP, params, Wp, WTp, Bp, PW, PB, flags, blockIdx.x * blockDim.x + threadIdx.x);
}
// ... of every member of an ensemble (grid.y = M): params (M, P), the packed arrays M x PW / PW / PB floats
__global__ void k_pack_ens(Net n, int WP, const float* __restrict__ params, float* __restrict__ Wp,
                           float* __restrict__ WTp, float* __restrict__ Bp, int PW, int PB, int flags) {
  const int64_t mem = blockIdx.y;
  pack_entry(n, WP, params + mem * n.n_params(), Wp + mem * PW, WTp + mem * PW, Bp + mem * PB, PW, PB, flags,
             blockIdx.x * blockDim.x + threadIdx.x);
}

// k_reduce_grads: grad_flat[real index] += sum over copies of the padded per-workgroup gradients.  64 parameters x
// 4 copy groups per block; each thread adds its group's copies in index order and the 4 partial sums
// are combined in a fixed order, so the result does not depend on scheduling.
// sum_copies: a thread's share of the copies, added in index order; the loads of eight copies are issued together (one memory
// round trip per eight instead of per copy: 59 -> 12 us on the 768 copies of the 10x10 net) — the ORDER of the
// additions, and with it the result, is unchanged
__device__ __forceinline__ float sum_copies(const float* __restrict__ wg, int64_t PP, int pidx, int c0, int c1) {
  float s = 0.f;
  int c = c0;
  for (; c + 8 <= c1; c += 8) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = wg[(int64_t)(c + j) * PP + pidx];
#pragma unroll
    for (int j = 0; j < 8; ++j) s += v[j];
  }
  for (; c < c1; ++c) s += wg[(int64_t)c * PP + pidx];
  return s;
}

// Where flat parameter i lives in the padded arrays: its layer l, PADDED row / col (bias: row only), the layer's offset wo
// into the padded weights, and its index pidx into a padded, fragment-native gradient copy (fused_kernel.h, GradSink).
struct ParamSlot { int64_t i; int l, row, col, wo, pidx; bool is_w; };
__device__ __forceinline__ ParamSlot param_slot(const Net& n, int WP, int PW, int flags, int64_t i) {
  const int rmajor = (flags & PACK_RMAJOR) != 0;   // [r][lane] inside a 16x16 block (bwgrad_flush, BSINK_ATOMIC)
  ParamSlot p;
  p.i = i; p.l = n.layer_of(i);
  const int64_t r = i - n.w_off(p.l);
  const int in_d = n.in_dim(p.l), out_d = n.out_dim(p.l);
  p.wo = (p.l == 0) ? 0 : WP * 16 + (p.l - 1) * WP * WP;
  p.is_w = r < (int64_t)in_d * out_d;
  if (p.is_w) {
    p.row = unit_at((int)(r / in_d), row_permuted(flags, p.l, n.L)); p.col = unit_at((int)(r % in_d), col_permuted(flags, p.l));
    const int ntn = ((p.l == 0) ? 16 : WP) / 16;
    const int blk = (p.row >> 4) * ntn + (p.col >> 4), ln = ((p.row & 15) >> 2) * 16 + (p.col & 15);
    p.pidx = rmajor ? p.wo + (blk * 4 + (p.row & 3)) * 64 + ln : p.wo + (blk * 64 + ln) * 4 + (p.row & 3);
  } else {
    p.row = unit_at((int)(r - (int64_t)in_d * out_d), row_permuted(flags, p.l, n.L)); p.col = 0;
    p.pidx = PW + p.l * WP + p.row;
  }
  return p;
}
// This pass's gradient of flat parameter blockIdx.x * 64 + (threadIdx.x & 63), summed over the copies: each of the four
// 64-thread groups adds its share of the copies, the four partial sums are combined in a fixed order.  Called by all 256
// threads of a block; `owner` is true in the one thread per parameter (first group, i < n_params) that holds the result:
// only there are g (the gradient) and at (where the parameter lives) meaningful.
struct ParamGrad { bool owner; float g; ParamSlot at; };
__device__ __forceinline__ ParamGrad grad_of_param(const Net& n, int WP, const float* __restrict__ wg, int copies, int PP, int PW,
                                                   int flags) {
  __shared__ float part[4][64];
  const int lane_p = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * 64 + lane_p;
  ParamGrad r = {};
  float s = 0.f;
  if (i < n.n_params()) {
    r.at = param_slot(n, WP, PW, flags, i);
    const int per = (copies + 3) / 4;
    const int c0 = grp * per, c1 = (c0 + per < copies) ? c0 + per : copies;
    s = sum_copies(wg, PP, r.at.pidx, c0, c1);
  }
  part[grp][lane_p] = s;
  __syncthreads();
  r.owner = grp == 0 && i < n.n_params();
  if (r.owner) r.g = (part[0][lane_p] + part[1][lane_p]) + (part[2][lane_p] + part[3][lane_p]);
  return r;
}

__global__ void k_reduce_grads(Net n, int WP, const float* __restrict__ wg, int copies, int PP, int PW,
                               float* __restrict__ grad, int flags) {
  const ParamGrad r = grad_of_param(n, WP, wg, copies, PP, PW, flags);
  if (r.owner) grad[r.at.i] += r.g;
}

// The two parts of k_finish_adam (below), shared with the ensemble's finishing kernels:
// the loss sums' block: term_sums / col_sums <- the fixed-order column sums of the workgroups' partial sums and, optionally,
// the weighted losses.  Called by all 256 threads of ONE block.
// (finish_sums2: the term sums and the column sums from the partial sums of two different passes — pinn_adam_loop_ext runs
// the residual and the fidelity points as a pass each; finish_sums below: both from one pass)
// TAIL_TERMS = false: the caller's requests have at most MSE_SUM0 terms, all in their own slots (pinn_adam_loop_ext and
// pinn_adam_loop_balanced refuse the wave closure): term_slot is then the identity and is left out, so that their finishing
// kernels stay as they were compiled before the rule existed.
template <bool TAIL_TERMS = true>
__device__ __forceinline__ void finish_sums2(const float* __restrict__ wg_sums, int grid, const float* __restrict__ wg_sums_c, int grid_c,
                                             int n_terms, float* __restrict__ term_sums,
                                             int n_cols, float* __restrict__ col_sums, int n_loss_rows,
                                             const float* __restrict__ loss_rows, float* __restrict__ losses, int row_cols) {
#pragma clang fp contract(off)
  // [col sums (row_cols of them) | term sums], for the optional weighted losses.  row_cols is the CALLER's column
  // count — the stride of loss_rows (pinn_hip.h) — also when this pass carried no fidelity columns (n_cols = 0:
  // a residual-only request with n_res == N): their sums are then zeros, not a shifted layout.
  __shared__ double ssum[2 * PINN_MAX_ROLES + 8];
  if (threadIdx.x < 2 * PINN_MAX_ROLES + 8) ssum[threadIdx.x] = 0.0;
  __syncthreads();
  for (int j = 0; j < n_terms + n_cols; ++j) {
    const float sum = (float)column_sum(j < n_terms ? wg_sums : wg_sums_c, j < n_terms ? grid : grid_c, MAX_SUMS,
                                        j < n_terms ? (TAIL_TERMS ? term_slot(j) : j) : MSE_SUM0 + (j - n_terms));
    if (threadIdx.x == 0) {
      if (j < n_terms) { term_sums[j] = sum; ssum[row_cols + j] = (double)sum; }
      else { col_sums[j - n_terms] = sum; ssum[j - n_terms] = (double)sum; }
    }
    __syncthreads();
  }
  if ((int)threadIdx.x < n_loss_rows) {
    double a = 0.0;
    for (int j = 0; j < row_cols + n_terms; ++j) a += (double)loss_rows[threadIdx.x * (row_cols + n_terms) + j] * ssum[j];
    losses[threadIdx.x] = (float)a;
  }
}
__device__ __forceinline__ void finish_sums(const float* __restrict__ wg_sums, int grid, int n_terms, float* __restrict__ term_sums,
                                            int n_cols, float* __restrict__ col_sums, int n_loss_rows,
                                            const float* __restrict__ loss_rows, float* __restrict__ losses, int row_cols) {
  finish_sums2(wg_sums, grid, wg_sums, grid, n_terms, term_sums, n_cols, col_sums, n_loss_rows, loss_rows, losses, row_cols);
}
// a parameter block, once its gradient is summed (r, grad_of_param): Adam's update on the block's 64 parameters and the
// refreshed packed entries
__device__ __forceinline__ void finish_adam_apply(const Net& n, int WP, const ParamGrad& r,
                                                  float* __restrict__ grad, float* __restrict__ params, float* __restrict__ m,
                                                  float* __restrict__ v, float* __restrict__ Wp, float* __restrict__ WTp,
                                                  float* __restrict__ Bp, const AdamScalars& c) {
  if (r.owner) {
    const ParamSlot& p = r.at;
    const int64_t i = p.i;
    grad[i] = r.g;
    const float pn = adam_update(params[i], r.g, m[i], v[i], c);
    params[i] = pn;
    if (p.is_w) {
      const int inP = (p.l == 0) ? 16 : WP, outP = (p.l == n.L) ? 16 : WP;
      Wp[p.wo + p.row * inP + p.col] = pn;
      WTp[p.wo + p.col * outP + p.row] = pn;
    } else Bp[p.l * WP + p.row] = pn;
  }
}
// a parameter block: the gradient of the block's 64 parameters, Adam's update on them, the refreshed packed entries
__device__ __forceinline__ void finish_adam_params(const Net& n, int WP, const float* __restrict__ wg, int copies, int PP, int PW,
                                                   float* __restrict__ grad, float* __restrict__ params, float* __restrict__ m,
                                                   float* __restrict__ v, float* __restrict__ Wp, float* __restrict__ WTp,
                                                   float* __restrict__ Bp, const AdamScalars& c, int flags) {
  const ParamGrad r = grad_of_param(n, WP, wg, copies, PP, PW, flags);
  finish_adam_apply(n, WP, r, grad, params, m, v, Wp, WTp, Bp, c);
}
// One kernel for everything that follows the fused pass in an Adam iteration (pinn_loss_grad_adam_step): the
// gradient reduction of k_reduce_grads (grad_of_param), torch.optim.Adam's update (k_adam's adam_update, reduce_adam.h) on
// the parameter it just summed, the refreshed entries of the packed W / W^T / b the next pass reads (k_pack's mapping,
// inverted: padding entries stay zero), and — last block — the loss sums of k_reduce_sums (column_sum).  Five launches of
// ~4.7 us each become one at the reference's own problem sizes (N_res = 243).
__global__ void k_finish_adam(Net n, int WP, const float* __restrict__ wg, int copies, int PP, int PW,
                              const float* __restrict__ wg_sums, int grid, int n_terms, float* __restrict__ term_sums,
                              int n_cols, float* __restrict__ col_sums, float* __restrict__ grad,
                              float* __restrict__ params, float* __restrict__ m, float* __restrict__ v,
                              float* __restrict__ Wp, float* __restrict__ WTp, float* __restrict__ Bp, AdamScalars c,
                              int n_loss_rows, const float* __restrict__ loss_rows, float* __restrict__ losses,
                              int row_cols, int flags) {
  if (blockIdx.x == gridDim.x - 1) {          // loss sums
    finish_sums(wg_sums, grid, n_terms, term_sums, n_cols, col_sums, n_loss_rows, loss_rows, losses, row_cols);
    return;
  }
  finish_adam_params(n, WP, wg, copies, PP, PW, grad, params, m, v, Wp, WTp, Bp, c, flags);
}

// ---- pinn_adam_loop_ext: everything that follows the residual pass and the fidelity pass of one iteration --------------------
// The residual pass (EPI_COEF / EPI_WEIGHTED instance) and the fidelity pass (K1 = 1) each leave a row of partial sums per
// workgroup and their own gradient copies.  Grid: [parameter blocks | one sums block | multiplier blocks].
struct ExtFinish {
  const float* wg_r; int copies_r; const float* sums_r; int grid_r;   // the residual pass
  const float* wg_f; int copies_f; const float* sums_f; int grid_f;   // the fidelity pass (copies_f == 0: there was none)
  int param_blocks;
  int n_terms, n_cols, row_cols;      // n_cols: of the fidelity pass (0 without one); row_cols: the caller's
  float* term_sums; float* col_sums; float* grad;
  float* params; float* m; float* v; float* Wp; float* WTp; float* Bp;
  AdamScalars c;
  int n_loss_rows; const float* loss_rows; float* losses;
  // coefficients (n_coef == 0: none)
  int n_coef; float* coef; float* coef_m; float* coef_v; float* coef_grad; const float* coef_mask; float* coef_log;
  AdamScalars cc;
  // self-adaptive multipliers (lam == nullptr: none): lam, lam_m, lam_v, point_w (rows, N); fields (n_fields, N)
  int rows, n_w, sa_mask; int64_t N;
  const float* scale; const float* fields; float* lam; float* lam_m; float* lam_v; float* point_w;
  AdamScalars cw;
};
// the self-adaptive weights w = m(lambda) (trainer.sa_weights): lambda^2 (sa_mask 0) or lambda (1)
__device__ __forceinline__ float sa_weight_of(float lam, int sa_mask) {
#pragma clang fp contract(off)
  return sa_mask == 0 ? lam * lam : lam;
}
// One multiplier, element e = t * N + n of lam: trainer.sa_weight_grad's arithmetic in its order, contraction off —
// sf = (s_t f) f, summed over the weighted terms in term order for a shared row; g = -((2 lam) sf) or -sf — then Adam's
// update along g and the weight of the next pass.
__device__ __forceinline__ void finish_multiplier(const ExtFinish& f, int64_t e) {
#pragma clang fp contract(off)
  const int64_t t = e / f.N, nn = e - t * f.N;
  float sf;
  if (f.rows == 1) {
    sf = 0.f;
    for (int tt = 0; tt < f.n_w; ++tt) {
      const float fv = f.fields[(int64_t)tt * f.N + nn];
      const float st = (f.scale[tt] * fv) * fv;
      sf = tt == 0 ? st : sf + st;
    }
  } else {
    const float fv = f.fields[e];
    sf = (f.scale[t] * fv) * fv;
  }
  const float lam = f.lam[e];
  const float gi = f.sa_mask == 0 ? -((2.0f * lam) * sf) : -sf;
  const float ln = adam_update(lam, gi, f.lam_m[e], f.lam_v[e], f.cw);
  f.lam[e] = ln;
  f.point_w[e] = sa_weight_of(ln, f.sa_mask);
}
__global__ void k_finish_adam_ext(Net n, int WP, int PP, int PW, ExtFinish f) {
  const int b = blockIdx.x;
  if (b < f.param_blocks) {        // gradient = fidelity pass's + residual pass's, Adam, packed entries (natural unit order)
    ParamGrad r = grad_of_param(n, WP, f.wg_r, f.copies_r, PP, PW, 0);
    if (f.copies_f > 0) {
      __syncthreads();             // (grad_of_param's partial sums are read before they are written again)
      const ParamGrad q = grad_of_param(n, WP, f.wg_f, f.copies_f, PP, PW, 0);
      if (r.owner) r.g = q.g + r.g;
    }
    finish_adam_apply(n, WP, r, f.grad, f.params, f.m, f.v, f.Wp, f.WTp, f.Bp, f.c);
    return;
  }
  if (b == f.param_blocks) {       // loss sums, weighted losses, coefficients
    finish_sums2<false>(f.sums_r, f.grid_r, f.sums_f, f.grid_f, f.n_terms, f.term_sums, f.n_cols, f.col_sums, f.n_loss_rows,
                 f.loss_rows, f.losses, f.row_cols);
    for (int c = 0; c < f.n_coef; ++c) {
      // (the coefficient gradient rode in the free term slot of the residual pass's partial sums: fused_kernel.h, COEF_SUM)
      const float cg = (float)column_sum(f.sums_r, f.grid_r, MAX_SUMS, COEF_SUM + c);
      if (threadIdx.x == 0) {
        const float cur = f.coef[c];
        if (f.coef_log) f.coef_log[c] = cur;          // the value this iteration ran with
        if (f.coef_grad) {
          float gi = 0.f + cg;                         // what reduce_sums_add adds to a zeroed array
          if (f.coef_mask) gi = gi * f.coef_mask[c];
          f.coef_grad[c] = gi;
          f.coef[c] = adam_update(cur, gi, f.coef_m[c], f.coef_v[c], f.cc);
        }
      }
      __syncthreads();
    }
    return;
  }
  const int64_t e = (int64_t)(b - f.param_blocks - 1) * 256 + threadIdx.x;
  if (f.lam && e < (int64_t)f.rows * f.N) finish_multiplier(f, e);
}
// before the first pass of a pinn_adam_loop_ext call with multipliers: point_w = m(lambda)
__global__ void k_sa_weights(const float* __restrict__ lam, float* __restrict__ w, int64_t count, int sa_mask) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < count) w[e] = sa_weight_of(lam[e], sa_mask);
}

// ---- pinn_adam_loop_balanced: the plain residual pass and the fidelity pass, their gradients combined with device weights -----
// Both kernels sum a group's gradient over its pass's copies with grad_of_param, residual first, so the statistics are
// taken on the very floats the finishing kernel combines.
struct BalFinish {
  const float* wg_r; int copies_r; const float* sums_r; int grid_r;   // the residual pass
  const float* wg_f; int copies_f; const float* sums_f; int grid_f;   // the fidelity pass
  int param_blocks;
  int n_terms, n_cols, row_cols;
  float* term_sums; float* col_sums; float* grad;
  float* params; float* m; float* v; float* Wp; float* WTp; float* Bp;
  AdamScalars c;
  int n_loss_rows; const float* loss_rows; float* losses;
  const float* lam; float* lam_log; float* group_grads;   // (2) [residual, fidelity]; null or this iteration's row (2); null or (2, P)
};
// update iterations only, one block per 64 parameters: partials[b] = the block's (max|g|, sum|g|, sum g^2) of the residual
// gradient, then of the fidelity gradient
__global__ void k_bal_stats(Net n, int WP, int PP, int PW, const float* __restrict__ wg_r, int copies_r,
                            const float* __restrict__ wg_f, int copies_f, double* __restrict__ partials) {
#pragma clang fp contract(off)
  const ParamGrad r = grad_of_param(n, WP, wg_r, copies_r, PP, PW, 0);
  __syncthreads();                 // (grad_of_param's partial sums are read before they are written again)
  const ParamGrad q = grad_of_param(n, WP, wg_f, copies_f, PP, PW, 0);
  for (int j = 0; j < 2; ++j) {
    const double gv = r.owner ? (double)(j == 0 ? r.g : q.g) : 0.0;
    double a = fabs(gv), s = a, sq = gv * gv;
    if (j) __syncthreads();
    balance_block_reduce(a, s, sq);
    if (threadIdx.x == 0) {
      double* out = partials + ((int64_t)blockIdx.x * 2 + j) * PINN_BALANCE_STATS;
      out[BAL_A] = a; out[BAL_S] = s; out[BAL_Q] = sq;
    }
  }
}
// ... one block of 256 threads: the partials folded in a fixed order, the rule on lam, the statistics' log row
__global__ void k_bal_weights(int mode, int ref, double alpha, int64_t P, const double* __restrict__ partials, int nb,
                              float* __restrict__ lam, double* __restrict__ stats_row) {
  balance_finish(mode, 2, ref, alpha, P, partials, nb, lam, stats_row);
}
__global__ void k_finish_adam_bal(Net n, int WP, int PP, int PW, BalFinish f) {
#pragma clang fp contract(off)
  const int b = blockIdx.x;
  if (b < f.param_blocks) {        // g = (lam[0] g_res) + (lam[1] g_fid), Adam, packed entries (natural unit order)
    ParamGrad r = grad_of_param(n, WP, f.wg_r, f.copies_r, PP, PW, 0);
    __syncthreads();
    const ParamGrad q = grad_of_param(n, WP, f.wg_f, f.copies_f, PP, PW, 0);
    if (r.owner) {
      if (f.group_grads) { f.group_grads[r.at.i] = r.g; f.group_grads[n.n_params() + r.at.i] = q.g; }
      const float wr = f.lam[0] * r.g, wf = f.lam[1] * q.g;
      r.g = wr + wf;
    }
    finish_adam_apply(n, WP, r, f.grad, f.params, f.m, f.v, f.Wp, f.WTp, f.Bp, f.c);
    return;
  }
  finish_sums2<false>(f.sums_r, f.grid_r, f.sums_f, f.grid_f, f.n_terms, f.term_sums, f.n_cols, f.col_sums, f.n_loss_rows,
               f.loss_rows, f.losses, f.row_cols);
  if (f.lam_log && threadIdx.x < 2) f.lam_log[threadIdx.x] = f.lam[threadIdx.x];   // the weights this iteration stepped with
}

// The ensemble's finishing kernels, grid (parameter blocks + 1, M): member blockIdx.y's share of every array, then the
// single-network functions.  gx is the per-member grid of the pass (a gradient copy and a row of partial sums per workgroup); terms_stride / row_cols are
// the caller's n_terms / n_cols: the row lengths of term_sums / col_sums, also when this pass carried no fidelity columns.
struct EnsFinish {
  const float* wg; const float* wg_sums;    // M x gx x PP, M x gx x MAX_SUMS
  float* term_sums; float* col_sums;        // (M, n_terms), (M, row_cols)
  float* grad;                              // (M, P)
};
__device__ __forceinline__ EnsFinish ens_finish_member(EnsFinish f, const Net& n, int gx, int PP, int n_terms_stride, int row_cols) {
  const int64_t mem = blockIdx.y;
  f.wg += mem * gx * PP; f.wg_sums += mem * gx * MAX_SUMS;
  f.term_sums += mem * n_terms_stride; f.col_sums += mem * row_cols;
  f.grad += mem * n.n_params();
  return f;
}
// plain (no Adam): sums as k_reduce_sums writes them, grad (M, P) += as k_reduce_grads adds
__global__ void k_finish_ens(Net n, int WP, EnsFinish f0, int gx, int PP, int PW, int n_terms, int n_cols, int terms_stride,
                             int row_cols, int flags) {
  const EnsFinish f = ens_finish_member(f0, n, gx, PP, terms_stride, row_cols);
  if (blockIdx.x == gridDim.x - 1) {
    finish_sums(f.wg_sums, gx, n_terms, f.term_sums, n_cols, f.col_sums, 0, nullptr, nullptr, row_cols);
    return;
  }
  const ParamGrad r = grad_of_param(n, WP, f.wg, gx, PP, PW, flags);
  if (r.owner) f.grad[r.at.i] += r.g;
}
__global__ void k_finish_adam_ens(Net n, int WP, EnsFinish f0, int gx, int PP, int PW, int n_terms, int n_cols, int terms_stride,
                                  int row_cols, float* __restrict__ params, float* __restrict__ m, float* __restrict__ v,
                                  float* __restrict__ Wp, float* __restrict__ WTp, float* __restrict__ Bp, AdamScalars c,
                                  int n_loss_rows, const float* __restrict__ loss_rows, float* __restrict__ losses, int flags) {
  const EnsFinish f = ens_finish_member(f0, n, gx, PP, terms_stride, row_cols);
  const int64_t mem = blockIdx.y, np = n.n_params();
  if (blockIdx.x == gridDim.x - 1) {
    finish_sums(f.wg_sums, gx, n_terms, f.term_sums, n_cols, f.col_sums, n_loss_rows, loss_rows, losses + mem * n_loss_rows, row_cols);
    return;
  }
  finish_adam_params(n, WP, f.wg, gx, PP, PW, f.grad, params + mem * np, m + mem * np, v + mem * np, Wp + mem * PW,
                     WTp + mem * PW, Bp + mem * (PP - PW), c, flags);
}

// what pinn_jet_backward hands the tile kernel instead of a loss: the caller's output adjoints, and where the gradient goes
struct AdjReq {
  const float* gY; const float* gdY;   // either may be null
  float* grad;                         // device flat grad (+=)
};

// what pinn_residual_fields hands the tile kernel instead of a loss: the residual and where its fields go, (NF, N)
struct FieldReq {
  pinn_residual_spec spec;   // normalised (pinn_abi.hip, check_spec)
  float* fields;
};

// The family of kernel instances a request takes (fused_launch.h, TileFamily), in the order of precedence: what the call
// asks for (fields, an external adjoint), then what the network needs (dropout, the sine first layer), then the request's
// epilogue.  run() refuses the combinations without instances; the batch kernel has the adjoint, corrected and loss families.
TileFamily tile_family(const Net& n, const LossReq* rq, const AdjReq* adj, const FieldReq* fld) {
  if (fld) return fld->spec.residual_id == RES_PE_WAVE ? TF_FIELD_WAVE : fld->spec.residual_id == RES_PE_CORRECTED ? TF_FIELD_PEC : TF_FIELD;
  if (adj) return TF_ADJ;
  if (n.drop_p > 0.f) return TF_DROP;
  if (n.act == PINN_ACT_SIN_TANH) return TF_SIN;
  if (is_weighted(rq)) return TF_WEIGHTED;
  if (is_coef(rq)) return TF_COEF;
  return is_wave(rq) ? TF_WAVE : is_pec(rq) ? TF_PEC : TF_LOSS;
}

// One pass of pinn_adam_loop_ext: run() launches the gradient pass ALONE — no reduction, no finishing kernel, the packing
// kernel only if asked — with its scratch, partial sums and gradient copies at the byte offsets the caller names (the
// caller has checked the workspace against its own layout, fused_adam_ext), and reports what the finishing kernel needs.
struct PassOnly {
  int64_t scratch, wg_sums, wg_grads;   // in
  bool pack;                            // in: the packed weights are not valid yet
  int grid, n_copies;                   // out: rows of partial sums, gradient copies
  bool natural = false;                 // in: keep the pass in natural unit order — neither the batch kernel (PACK_PERM) nor the
                                        // width-64 KRO > 0 instances (PACK_IN | PACK_OUT), which a PLAIN residual request may
                                        // otherwise choose (pinn_adam_loop_balanced); the tile kernel with io1 = 0 serves instead
};

int run(const Net& n, bool grad, const LossReq* rq, const float* params, const float* X, int64_t N, float* Y,
        float* dY, void* ws, int64_t ws_bytes, hipStream_t s, const AdjReq* adj = nullptr, const FieldReq* fld = nullptr,
        PassOnly* po = nullptr) {
  const Geo g = geo_of(n);
  WsLayout w = ws_layout(n, g, N, fld != nullptr);
  if (po) { w.scratch = po->scratch; w.wg_sums = po->wg_sums; w.wg_grads = po->wg_grads; }
  if (!po) { if (int rc = check_workspace(ws, ws_bytes, w.total)) return rc; }
  char* base = (char*)ws;
  FusedParams P;
  memset(&P, 0, sizeof(P));
  P.d_in = n.d_in; P.d_out = n.d_out; P.L = n.L; P.act = n.act;
  for (int j = 0; j < PINN_MAX_DIRS; ++j) P.dir_col[j] = n.dir_col[j];
  P.N = N; P.n_tiles = (N + 15) / 16;
  P.n_split = -1;
  P.X = X;
  P.Wp = (const float*)(base + w.wp); P.WTp = (const float*)(base + w.wtp); P.Bp = (const float*)(base + w.bp);
  P.scratch = (float*)(base + w.scratch);
  P.scratch_per_wave = (int64_t)n.L * n.K1 * g.NTH * 256;
  P.Y = Y; P.dY = dY;
  P.wg_sums = (float*)(base + w.wg_sums);
  P.wg_grads = (float*)(base + w.wg_grads);
  P.PW = g.PW; P.PB = g.PB;
  P.acc_lds = (grad && fits_lds(g)) ? 1 : 0;
  P.lds_acc_floats = P.acc_lds ? g.PP : 0;
  if (rq) set_loss(P, n, *rq);
  if (adj) { P.gY = adj->gY; P.gdY = adj->gdY; }
  const bool wtq = is_weighted(rq);
  const bool coefq = is_coef(rq) || wtq;   // (everything below that holds for a coefficient request holds for a weighted one)
  if (coefq) P.gY = rq->coef;   // (fused_kernel.h, FusedParams: the coefficient instances' array)
  if (wtq) {   // (fused_kernel.h, FusedParams: the weighted instances' weights, their row stride and the optional fields array)
    P.gY = rq->point_w; P.n_split = rq->w_stride;
    P.Y = rq->fields_out; P.dY = nullptr;
  }
  if (fld) {   // the residual's roles as a residual loss sets them; nothing else of a loss request
    P.Y = fld->fields; P.dY = nullptr;   // (fused_kernel.h, FusedParams: the field instances' output array)
    set_residual_roles(P, n, fld->spec);
  }
  // (the field epilogue exists in the tile kernel only: every kernel choice of desc.engine lands there; the external-adjoint
  // one in the tile and in the batch kernel)
  const bool pec = is_pec(rq), fpec = fld && is_pe_closure(fld->spec.residual_id), wave = is_wave(rq);
  if (n.act == PINN_ACT_SIN_TANH && (adj || fld || n.drop_p > 0.f)) {   // (refused upstream: never a tanh kernel on a sine network)
    set_error("fused engine: no kernel for the sine first layer (activation 2) on this request"); return PINN_ERR_UNSUPPORTED;
  }
  if ((pec || fpec) && fused_corrected_refusal(n)) {
    set_error("fused engine: %s %s", pe_closure_name(wave || (fld && fld->spec.residual_id == RES_PE_WAVE)), fused_corrected_refusal(n));
    return PINN_ERR_UNSUPPORTED;
  }
  if (wave && (n.fused_kernel == FUSED_KERNEL_BATCH || n.fused_kernel == FUSED_KERNEL_COOP || (P.loss_kind & 2 && rq->n_cols > WAVE_MAX_COLS))) {
    // (refused upstream, pinn_abi.hip corrected_engine: tile-kernel instances only, and the fifth term's sum owns the last column's slot)
    set_error("fused engine: %s has no kernel for this request", pe_closure_name(true)); return PINN_ERR_UNSUPPORTED;
  }
  const bool natural = po && po->natural;
  const bool batch = !natural && !fld && !coefq && !wave && (adj ? use_batch_adj(n, g, N) : use_batch(n, g, grad, N));
  const bool coop = !adj && !fld && !batch && !pec && !coefq && use_coop(n, g, grad, N);   // (FUSED_COOP with it: the tile kernel)
  if (coop) {
    P.acc_lds = grad ? 1 : 0;
    P.lds_acc_floats = grad ? g.PP : 0;
  }
  if (batch) {   // the batch kernel carves its own pads (batch_pads per wave); the gradient copy stays in LDS if it still fits
    // a gradient copy per wave in LDS if four of them fit, else atomics into BATCH_ATOMIC_COPIES shared copies (bwgrad_flush)
    P.acc_lds = ((int64_t)BATCH_WAVES * g.PP * 4 + batch_lds_fixed_bytes(g.WP, n.K1)) * batch_occ(g.WP, n.K1) <= LDS_LIMIT ? 1 : 0;
    P.lds_acc_floats = P.acc_lds ? BATCH_WAVES * g.PP : 0;
  }
  const size_t lds = batch ? (size_t)P.lds_acc_floats * 4 + (size_t)batch_lds_fixed_bytes(g.WP, n.K1) +
                                 (size_t)(!P.acc_lds && batch_T_for(g, n.K1, P.n_tiles) == 1 ? batch_lds_comb_bytes(g.WP) : 0)
                   : coop ? (size_t)coop_lds_bytes(n, g, grad) : (size_t)P.lds_acc_floats * 4 + (size_t)lds_fixed_bytes();
  // 8x64 gradient kernels fill the register file and most of LDS (1 workgroup per CU); the narrow
  // networks' kernels fit 2 waves per SIMD, which hides their per-layer latencies
  // (a forward-only coefficient request takes the GRID of its gradient call — the geometry that call's LDS gives — so that its
  // per-workgroup partial sums, and with them term_sums, are the gradient call's bit for bit: include/pinn_hip.h)
  const bool as_grad = grad || coefq;
  const int64_t lds_geo = coefq && !grad ? (int64_t)(fits_lds(g) ? g.PP : 0) * 4 + lds_fixed_bytes() : (int64_t)lds;
  const bool one_per_cu = as_grad && (coefq ? fits_lds(g) : P.acc_lds != 0) && !(g.WP <= 32 && 2 * lds_geo <= LDS_LIMIT);
  const int per_cu = tile_wgs_per_cu(g.WP) * lds_geo <= LDS_LIMIT ? tile_wgs_per_cu(g.WP) : 2;
  int grid = adj && !batch ? adj_grid_for(P.n_tiles, one_per_cu, per_cu) : grid_for(P.n_tiles, one_per_cu, per_cu);
  if (coop) grid = coop_grid_for(P.n_tiles, grad);

  if (batch) {   // one workgroup per CU, one wave per SIMD; slots of T tiles x (L - 1) layers per wave
    const int T = batch_T_for(g, n.K1, P.n_tiles);
    P.batch_T = T;
    grid = batch_grid(P.n_tiles, T, batch_occ(g.WP, n.K1));
    P.scratch_per_wave = (int64_t)T * (n.L > 1 ? n.L - 1 : 1) * n.K1 * batch_ks(n) * 64;
  }
  // k_fused<64, ..., KRO > 0>: the specialised-epilogue kernels take inputs / outputs in k-step-major order
  if (!natural && !batch && !coop && !coefq && n.drop_p == 0.f && g.WP == 64 && grad && P.acc_lds && n.act == PINN_ACT_TANH && P.loss_kind == 1 && !Y && P.n_split < 0 &&
      n.d_in <= 4) {
    const int rid = P.residual_id;
    P.io1 = (n.K1 == 4 && rid == PINN_RES_NAVIER_STOKES && n.d_out <= 4) ||
            (n.K1 == 3 && rid == PINN_RES_PHYSICS_EQUATION && n.d_out <= 8) ||
            (n.K1 == 3 && (rid == PINN_RES_CONTINUITY_ONLY || rid == PINN_RES_CONTINUITY_FTEMP) && n.d_out <= 4);
    if (P.io1) {   // the epilogue addresses the output tile / the input jet by PADDED index
      for (int j = 0; j < PINN_MAX_ROLES; ++j) if (P.out_col[j] >= 0) P.out_col[j] = perm16(P.out_col[j]);
      for (int j = 0; j < PINN_MAX_DIRS; ++j) if (P.dir_col[j] >= 0) P.dir_col[j] = perm16(P.dir_col[j]);
    }
  }
  const int perm = (batch ? PACK_PERM : 0) | (P.io1 ? PACK_IN | PACK_OUT : 0);   // unit order the pass expects

  const AdamReq* adam = rq ? rq->adam : nullptr;
  const int packN = g.PW > g.PB ? g.PW : g.PB;
  // pinn_adam_loop_ext / pinn_adam_loop_balanced: one packed copy serves its two passes and its finishing kernel, so both must take natural unit order.
  // An INTERNAL INVARIANT, not a refusal a caller can meet: a coefficient / weighted request never takes the batch kernel or
  // the KRO > 0 order (coefq above), and a K1 = 1 pass has neither (fused_batch_has_kernel wants K1 = 3 or 4, io1 a residual),
  // so perm is 0 for both passes by construction.  Should a later kernel choice break that, the call stops here with what it
  // has enqueued so far instead of finishing an iteration on weights packed in the wrong order.
  if (po && perm) { set_error("fused engine: a pass of a device-enqueued Adam run would run in permuted unit order"); return PINN_ERR_UNSUPPORTED; }
  if (po ? po->pack : !(adam && adam->packed_valid))
    hipLaunchKernelGGL(k_pack, dim3((packN + 255) / 256), dim3(256), 0, s, n, g.WP, params, (float*)(base + w.wp),
                       (float*)(base + w.wtp), (float*)(base + w.bp), g.PW, g.PB, perm);
  // gradient copies the reduction reads: one per workgroup, or the batch kernel's shared atomic copies (register-major)
  const int rmajor = batch && !P.acc_lds ? 1 : 0;
  const int n_copies = rmajor ? (grid < BATCH_ATOMIC_COPIES ? grid : BATCH_ATOMIC_COPIES) : grid;
  if (grad && !P.acc_lds) {   // global gradient copies start from zero
    if (hipMemsetAsync(P.wg_grads, 0, (size_t)n_copies * g.PP * 4, s) != hipSuccess) {
      set_error("hipMemsetAsync failed"); return PINN_ERR_LAUNCH;
    }
  }
  // One launch: the family of instances the request takes (tile_family), on the kernel chosen above.  The field families:
  // forward-only grid (grid_for above, grad == false), natural unit order (perm == 0), no reductions, and no dynamic LDS —
  // these instances touch neither the pads nor the gradient copy.
  const TileFamily fam = tile_family(n, rq, adj, fld);
  const TileLaunch tile{n.K1, grad, P, dim3(grid), fld ? 0 : lds, s};
  const BatchLaunch bat{n.W, n.d_in, P, grid, lds, s};
  if (fam == TF_ADJ && n.drop_p > 0.f) { set_error("fused engine: no dropout instance of the external-adjoint kernel"); return PINN_ERR_UNSUPPORTED; }
  if (fam == TF_DROP) {     // training-mode dropout: its own instances of the tile kernel
    P.drop_seed = n.drop_seed; P.drop_thresh = n.drop_thresh; P.drop_scale = 1.f / (1.f - n.drop_p); P.drop_keep = 1.f - n.drop_p;
    if (!(grad && g.WP == 64 && P.acc_lds && n.act == PINN_ACT_TANH)) { set_error("fused engine: no dropout kernel for this request"); return PINN_ERR_UNSUPPORTED; }
  }
  int rc;
  if ((fam == TF_LOSS || fam == TF_SIN) && !rq && !grad && !coop && !batch && n.K1 == 1 && Y && !dY && n.fused_kernel == FUSED_KERNEL_AUTO &&
      P.n_tiles >= fused_plain_min_tiles(g.WP, cu_count())) {
    // pinn_forward on enough points to give every wave the chip holds a pass of four tiles: the plain forward's own
    // kernel, one weight fetch per 64 points (pinn_fused_plain.hip)
    rc = launch_fused_plain(g.WP, P, cu_count(), s);
  }
  else if (fam == TF_SIN && (wtq || coefq || pec || batch || coop)) {   // the sine first layer: the tile kernel's generic epilogue only
    set_error("fused engine: no kernel for the sine first layer (activation 2) on this request"); return PINN_ERR_UNSUPPORTED;
  }
  // (a field, dropout, coefficient or weighted request never has batch or coop set: above)
  else if (batch) rc = launch_batch(fam == TF_ADJ ? BF_ADJ : fam == TF_PEC ? BF_PEC : BF_LOSS, g.WP, n.K1, bat);
  else if (coop) rc = launch_fused_coop(n.K1, grad, P, grid, lds, s);
  else rc = launch_tile(fam, g.WP, tile);
  if (rc || fld) return rc;
  if (adj) {
    // (no loss sums after an adjoint pass: wg_sums is not read)
    const int64_t np = n.n_params();
    hipLaunchKernelGGL(k_reduce_grads, dim3((unsigned)((np + 63) / 64)), dim3(256), 0, s, n, g.WP,
                       (const float*)P.wg_grads, n_copies, g.PP, g.PW, adj->grad, perm | (rmajor ? PACK_RMAJOR : 0));
    return check_launch("fused reductions");
  }
  if (po) { po->grid = grid; po->n_copies = n_copies; return check_launch("fused pass"); }
  if (adam) {
    const int64_t np = n.n_params();
    hipLaunchKernelGGL(k_finish_adam, dim3((unsigned)((np + 63) / 64) + 1), dim3(256), 0, s, n, g.WP,
                       (const float*)P.wg_grads, n_copies, g.PP, g.PW, (const float*)P.wg_sums, grid,
                       (P.loss_kind & 1) ? rq->n_terms : 0, rq->sums, (P.loss_kind & 2) ? rq->n_cols : 0, rq->mse_sums,
                       rq->grad, adam->params, adam->m, adam->v, (float*)(base + w.wp), (float*)(base + w.wtp),
                       (float*)(base + w.bp), adam->c, adam->n_loss_rows, adam->loss_rows, adam->losses, rq->n_cols, perm | (rmajor ? PACK_RMAJOR : 0));
    return check_launch("fused finish + adam");
  }
  if (rq) {
    if (P.loss_kind & 1) {   // (terms beyond the first MSE_SUM0 sit behind the columns: fused_kernel.h, term_slot)
      reduce_sums(P.wg_sums, grid, MAX_SUMS, 0, std::min(rq->n_terms, MSE_SUM0), rq->sums, s);
      for (int t = MSE_SUM0; t < rq->n_terms; ++t) reduce_sums(P.wg_sums, grid, MAX_SUMS, term_slot(t), 1, rq->sums + t, s);
    }
    if (coefq && !wtq && grad && rq->coef_grad)   // the coefficient gradient rode in the free term slot (fused_kernel.h, COEF_SUM)
      reduce_sums_add(P.wg_sums, grid, MAX_SUMS, COEF_SUM, rq->n_coef, rq->coef_grad, s);
    if (P.loss_kind & 2)
      reduce_sums(P.wg_sums, grid, MAX_SUMS, MSE_SUM0, rq->n_cols, rq->mse_sums, s);
    if (grad) {
      const int copies = n_copies;
      const int64_t np = n.n_params();
      hipLaunchKernelGGL(k_reduce_grads, dim3((unsigned)((np + 63) / 64)), dim3(256), 0, s, n, g.WP,
                         (const float*)P.wg_grads, copies, g.PP, g.PW, rq->grad, perm | (rmajor ? PACK_RMAJOR : 0));
    }
  }
  return check_launch("fused reductions");
}

}  // namespace

// ---- the entry points of fused_launch.h: one table of units per kernel -------------------------------------------------------
#define TILE_ROW(F) {tile_unit<F, 16>, tile_unit<F, 32>, tile_unit<F, 64>}
int launch_tile(TileFamily f, int WP, const TileLaunch& a) {
  static int (*const unit[TF_COUNT][3])(const TileLaunch&) = {   // (in TileFamily's order)
      TILE_ROW(TF_LOSS), TILE_ROW(TF_ADJ), TILE_ROW(TF_FIELD), TILE_ROW(TF_PEC), TILE_ROW(TF_FIELD_PEC), TILE_ROW(TF_COEF),
      TILE_ROW(TF_WEIGHTED), TILE_ROW(TF_SIN), {nullptr, nullptr, tile_unit<TF_DROP, 64>}, TILE_ROW(TF_ENS), TILE_ROW(TF_WAVE),
      TILE_ROW(TF_FIELD_WAVE)};
  const auto fn = unit[f][WP == 16 ? 0 : WP == 32 ? 1 : 2];
  if (!fn) { set_error("fused engine: no kernel of family %d at padded width %d", (int)f, WP); return PINN_ERR_UNSUPPORTED; }
  return fn(a);
}
// (K1 = 3, else the K1 = 4 unit; the corrected radiation stress has K1 = 3 units only)
#define BATCH_ROW(F, K4) {{batch_unit<F, 16, 3>, batch_unit<F, 16, K4>}, {batch_unit<F, 32, 3>, batch_unit<F, 32, K4>}}
int launch_batch(BatchFamily f, int WP, int K1, const BatchLaunch& a) {
  static int (*const unit[BF_COUNT][2][2])(const BatchLaunch&) = {BATCH_ROW(BF_LOSS, 4), BATCH_ROW(BF_ADJ, 4), BATCH_ROW(BF_PEC, 3)};
  return unit[f][WP == 16 ? 0 : 1][K1 == 3 ? 0 : 1](a);
}
bool fused_batch_has_kernel(int WP, int W, int d_in, int K1, int act) {
  return (WP == 16 || WP == 32) && W >= 1 && d_in <= 8 && (K1 == 3 || K1 == 4) && act == PINN_ACT_TANH;
}

bool fused_supports(const Net& n, bool want_grad) {
  if (n.L + 1 > MAX_LOCKS) return false;
  // the sine first layer: exactly where a k_fused<.., PINN_ACT_SIN_TANH, EPI_GENERIC> instance exists (pinn_fused_tile.hip, TF_SIN) —
  // K1 in {1, 3, 4}, no dropout, the tile kernel (never the cooperative or the batch kernel: use_coop, fused_batch_has_kernel)
  if (n.act == PINN_ACT_SIN_TANH &&
      (n.drop_p > 0.f || n.prec != PINN_PREC_F32 || n.fused_kernel == FUSED_KERNEL_COOP || n.fused_kernel == FUSED_KERNEL_BATCH ||
       !(n.K1 == 1 || n.K1 == 3 || n.K1 == 4)))
    return false;
  if (n.drop_p > 0.f) {   // dropout: gradient passes of tanh networks of padded width 64 whose gradient copy fits LDS
    if (!(want_grad && padded_width(n.W) == 64 && n.act == PINN_ACT_TANH && fits_lds(geo_of(n)) && n.fused_kernel != FUSED_KERNEL_COOP &&
          (n.K1 == 1 || n.K1 == 3 || n.K1 == 4)))
      return false;
  }
  if (want_grad && n.K1 == 2) return false;   // no k = 1 gradient kernels (no residual of the reference has one direction)
  if (n.fused_kernel == FUSED_KERNEL_COOP && padded_width(n.W) != 64) return false;
  return n.W <= 64 && n.d_in <= 16 && n.d_out <= 16 && n.L >= 1 && n.K1 >= 1 && n.K1 <= 4;
}

// ---- the serving rule of the tile kernel's families of instances (common.h: TILE_*) ---------------------------------------
// Every family is the tile kernel's shape class (fp32, width <= 64, d_in and d_out <= 16, a lock per layer) without dropout
// and without the sine first layer, narrowed by what its instances exist for.  Each condition is written once, with the
// reason a refusal gives; a family is its name in those reasons and the conditions that apply to it, in the order in which
// its entry's table names them (with two causes at once the first is reported, and callers match on the text).
namespace {
enum TileCond {
  T_FORCED,    // desc.engine forces the cooperative or the batch kernel.  Not a condition of the external-adjoint and field
               // families: there the kernel choice does not matter for WHETHER the call is served (a request the batch kernel
               // has no instance for runs on the tile kernel; run() always takes the tile kernel for fields)
  T_PREC, T_WIDTH, T_SINE,
  T_LEAKY,     // (the external-adjoint and field instances exist for LeakyReLU)
  T_DROPOUT,
  T_K23,       // k is a residual's number of directions: K1 = 3 or 4
  T_K1,        // the gradient kernels' rule: no K1 = 2 (no residual of the reference has one direction); K1 = 1 is served
  T_IO, T_DEPTH, T_END
};
const TileCond ADJ_CONDS[] = {T_SINE, T_DROPOUT, T_PREC, T_K1, T_WIDTH, T_IO, T_DEPTH, T_END};
const TileCond FIELD_CONDS[] = {T_SINE, T_DROPOUT, T_PREC, T_K23, T_WIDTH, T_IO, T_DEPTH, T_END};
const TileCond LOSS_CONDS[] = {T_FORCED, T_PREC, T_WIDTH, T_SINE, T_LEAKY, T_DROPOUT, T_K23, T_IO, T_DEPTH, T_END};
struct TileRule { const char* noun; const char* kernel; const TileCond* conds; };
const TileRule TILE_RULES[] = {   // indexed by TILE_*
    {"external-adjoint", "external-adjoint kernel", ADJ_CONDS},
    {"field", "field kernel", FIELD_CONDS},
    {"coefficient", "coefficient kernel on the fused engine", LOSS_CONDS},
    {"weighted", "weighted kernel on the fused engine", LOSS_CONDS},
    {"ensemble", "ensemble kernel", LOSS_CONDS},
    {"balanced", "balanced loop on the fused engine", LOSS_CONDS},
};
// the reason of one condition, or nullptr where the network meets it (%s: the family's noun in T_FORCED, else its kernel)
const char* tile_cond_reason(TileCond c, const Net& n) {
  switch (c) {
    case T_FORCED:
      return n.fused_kernel == FUSED_KERNEL_COOP || n.fused_kernel == FUSED_KERNEL_BATCH
                 ? "the %s instances are the tile kernel's: engine FUSED_COOP / FUSED_BATCH has none (use AUTO, FUSED or FUSED_TILE)" : nullptr;
    case T_PREC: return n.prec != PINN_PREC_F32 ? "bf16 precision exists on the wide engine only, which has no %s" : nullptr;
    case T_WIDTH: return n.W > 64 ? "hidden width above 64 has no %s" : nullptr;
    case T_SINE: return n.act == PINN_ACT_SIN_TANH ? "the sine first layer (activation 2) has no %s" : nullptr;
    case T_LEAKY: return n.act == PINN_ACT_LEAKY_RELU ? "LeakyReLU has no %s" : nullptr;
    case T_DROPOUT: return n.drop_p > 0.f ? "dropout_p > 0 has no %s" : nullptr;
    case T_K23: return n.K1 != 3 && n.K1 != 4 ? "k must be 2 or 3" : nullptr;
    case T_K1: return n.K1 == 2 ? "k = 1 (one differentiated input) with gdY has no gradient kernel" : nullptr;
    case T_IO: return n.d_in > 16 || n.d_out > 16 ? "d_in or d_out above 16" : nullptr;
    case T_DEPTH: return n.L + 1 > MAX_LOCKS ? "network too deep for the per-layer locks" : nullptr;
    default: return nullptr;
  }
}
}  // namespace

const char* fused_tile_refusal(int family, const Net& n) {
  static thread_local char why[192];
  const TileRule& f = TILE_RULES[family];
  for (const TileCond* c = f.conds; *c != T_END; ++c)
    if (const char* fmt = tile_cond_reason(*c, n)) {
      snprintf(why, sizeof(why), fmt, *c == T_FORCED ? f.noun : f.kernel);
      return why;
    }
  return nullptr;
}

// (which of the two kernels with external-adjoint instances serves a request that fused_tile_refusal(TILE_ADJ) passes)
int fused_jet_backward_kernel(const Net& n, int64_t N) {
  return use_batch_adj(n, geo_of(n), N) ? PINN_ENGINE_FUSED_BATCH : PINN_ENGINE_FUSED_TILE;
}

// The corrected radiation stress (EPI_PEC / EPI_FIELD_PEC instances): tanh, k = 2, no dropout.  nullptr = served.
const char* fused_corrected_refusal(const Net& n) {
  if (n.act == PINN_ACT_SIN_TANH) return "has no instance for the sine first layer (activation 2) on the fused engine: use engine AUTO or GENERIC";
  if (n.act != PINN_ACT_TANH) return "has no LeakyReLU instance on the fused engine: use engine GENERIC";
  if (n.K1 != 3) return "has fused instances for k = 2 networks only: use engine GENERIC";
  if (n.drop_p > 0.f) return "has no dropout instance on the fused engine: use engine AUTO or GENERIC";
  return nullptr;
}

// Runtime coefficients (EPI_COEF instances, TILE_COEF) and point weights (EPI_WEIGHTED, TILE_WEIGHTED): one rule — the tile
// kernel only, fp32, tanh, k = 2 or 3, no dropout — one workspace, one way to the kernel.
int64_t fused_tile_workspace_bytes(int family, const Net& n, int64_t N) {
  if (fused_tile_refusal(family, n)) return -1;
  return ws_layout(n, geo_of(n), N > 0 ? N : 1).total;
}
int fused_tile_loss(int family, const Net& n, const LossReq& rq, const float* params, const float* X, int64_t N, void* ws,
                    int64_t ws_bytes, hipStream_t s) {
  if (const char* why = fused_tile_refusal(family, n)) { set_error("fused engine: %s", why); return PINN_ERR_UNSUPPORTED; }
  return run(n, rq.grad != nullptr, &rq, params, X, N, nullptr, nullptr, ws, ws_bytes, s);
}

// ---- pinn_adam_loop_ext ---------------------------------------------------------------------------------------------------
const char* fused_adam_ext_refusal(const Net& n, int family) {
  if (const char* why = fused_tile_refusal(family, n)) return why;
  Net n1 = n; n1.k = 0; n1.K1 = 1;
  if (!fused_supports(n1, true)) return "the fidelity pass has no fused gradient kernel for this network";
  return nullptr;
}
namespace {
// The workspace of pinn_adam_loop_ext: the single entries' layout for the larger of the two point sets (packed weights,
// scratch, and the RESIDUAL pass's partial sums and gradient copies), then the fidelity pass's partial sums and gradient
// copies.  Every region holds the largest grid any pass on that many points launches (ws_layout).
struct ExtLayout { WsLayout w; int64_t sums_f, grads_f, total; };
ExtLayout ext_layout(const Net& n, const Geo& g, int64_t N_res, int64_t N_fid) {
  ExtLayout e;
  const int64_t nmax = std::max<int64_t>(std::max(N_res, N_fid), 1);
  e.w = ws_layout(n, g, nmax);
  int64_t off = e.w.total;
  e.sums_f = off; off += align256((int64_t)e.w.max_grid * MAX_SUMS * 4);
  e.grads_f = off; off += align256((int64_t)e.w.max_grid * g.PP * 4);
  e.total = off;
  return e;
}
}  // namespace
int64_t fused_adam_ext_workspace_bytes(const Net& n, int64_t N_res, int64_t N_fid) {
  return ext_layout(n, geo_of(n), N_res, N_fid).total;
}
int fused_adam_ext(const Net& n, const AdamExtReq& q, const float* X, int64_t N_res, void* ws, int64_t ws_bytes, hipStream_t s) {
  if (const char* why = fused_adam_ext_refusal(n, q.res.coef ? TILE_COEF : TILE_WEIGHTED)) {
    set_error("fused engine, pinn_adam_loop_ext: %s", why); return PINN_ERR_UNSUPPORTED;
  }
  const Geo g = geo_of(n);
  const ExtLayout L = ext_layout(n, g, N_res, q.N_fid);
  if (int rc = check_workspace(ws, ws_bytes, L.total)) return rc;
  char* base = (char*)ws;
  Net n1 = n; n1.k = 0; n1.K1 = 1;   // the fidelity term needs no input derivatives (pinn_mse_loss_grad)
  const int64_t np = n.n_params();
  const int64_t n_lam = q.lam ? (int64_t)q.w_rows * N_res : 0;
  if (q.lam)   // w = m(lambda) of the first pass
    hipLaunchKernelGGL(k_sa_weights, dim3((unsigned)((n_lam + 255) / 256)), dim3(256), 0, s, (const float*)q.lam, q.point_w,
                       n_lam, q.sa_mask);
  if (q.N_fid == 0 && q.row_cols > 0 && q.col_sums) (void)hipMemsetAsync(q.col_sums, 0, q.row_cols * sizeof(float), s);
  ExtFinish f;
  memset(&f, 0, sizeof(f));
  f.param_blocks = (int)((np + 63) / 64);
  f.n_terms = q.res.n_terms; f.n_cols = q.N_fid > 0 ? q.fid.n_cols : 0; f.row_cols = q.row_cols;
  f.term_sums = q.res.sums; f.col_sums = q.col_sums; f.grad = q.res.grad;
  f.params = q.adam.params; f.m = q.adam.m; f.v = q.adam.v;
  f.Wp = (float*)(base + L.w.wp); f.WTp = (float*)(base + L.w.wtp); f.Bp = (float*)(base + L.w.bp);
  f.n_loss_rows = q.adam.n_loss_rows; f.loss_rows = q.adam.loss_rows;
  f.n_coef = q.res.coef ? q.n_coef : 0;
  f.coef = q.coef; f.coef_m = q.coef_m; f.coef_v = q.coef_v; f.coef_grad = q.coef_grad; f.coef_mask = q.coef_mask;
  f.rows = q.w_rows; f.n_w = q.res.n_weighted; f.sa_mask = q.sa_mask; f.N = N_res;
  f.scale = q.res.scale; f.fields = q.res.fields_out; f.lam = q.lam; f.lam_m = q.lam_m; f.lam_v = q.lam_v; f.point_w = q.point_w;
  const unsigned blocks = (unsigned)f.param_blocks + 1 + (unsigned)((n_lam + 255) / 256);
  for (int i = 0; i < q.n_iters; ++i) {
    PassOnly pr = {L.w.scratch, L.w.wg_sums, L.w.wg_grads, i == 0 && !q.adam.packed_valid, 0, 0};
    int rc = run(n, true, &q.res, q.adam.params, X, N_res, nullptr, nullptr, ws, ws_bytes, s, nullptr, nullptr, &pr);
    if (rc) return rc;
    // (on whichever kernel pinn_mse_loss_grad would take for these points: the cooperative one at padded width 64 while there
    // is at most one tile per CU, else the tile kernel — both natural order, one gradient copy and one sums row per workgroup)
    PassOnly pf = {L.w.scratch, L.sums_f, L.grads_f, false, 0, 0};
    if (q.N_fid > 0) {
      rc = run(n1, true, &q.fid, q.adam.params, q.Xf, q.N_fid, nullptr, nullptr, ws, ws_bytes, s, nullptr, nullptr, &pf);
      if (rc) return rc;
    }
    f.wg_r = (const float*)(base + L.w.wg_grads); f.copies_r = pr.n_copies; f.sums_r = (const float*)(base + L.w.wg_sums); f.grid_r = pr.grid;
    f.wg_f = (const float*)(base + L.grads_f); f.copies_f = pf.n_copies; f.sums_f = (const float*)(base + L.sums_f); f.grid_f = pf.grid;
    f.c = adam_scalars(q.lr[i], q.beta1, q.beta2, q.eps, q.step + i);
    if (f.n_coef && q.coef_grad) f.cc = adam_scalars(q.lr_coef[i], q.beta1, q.beta2, q.eps, q.step + i);
    if (q.lam) f.cw = adam_scalars(q.lr_w[i], q.beta1, q.beta2, q.eps, q.step + i);
    f.losses = q.adam.n_loss_rows > 0 ? q.adam.losses + (int64_t)i * q.adam.n_loss_rows : nullptr;
    f.coef_log = q.coef_log ? q.coef_log + (int64_t)i * f.n_coef : nullptr;
    hipLaunchKernelGGL(k_finish_adam_ext, dim3(blocks), dim3(256), 0, s, n, g.WP, g.PP, g.PW, f);
    rc = check_launch("fused finish + adam (ext)");
    if (rc) return rc;
  }
  return PINN_OK;
}

// ---- pinn_adam_loop_balanced ----------------------------------------------------------------------------------------------
// The residual pass is the PLAIN gradient request held to natural unit order (PassOnly::natural): the cooperative kernel
// where run() would take it anyway, else the tile kernel with io1 = 0 — never the batch kernel, never a KRO > 0 instance.
const char* fused_adam_bal_refusal(const Net& n) {
  if (n.fused_kernel == FUSED_KERNEL_BATCH)
    return "engine FUSED_BATCH: the batch kernel runs in permuted unit order, the balanced loop needs natural order (use AUTO, "
           "FUSED, FUSED_TILE or FUSED_COOP)";
  Net t = n; t.fused_kernel = FUSED_KERNEL_AUTO;   // (the forced-kernel condition of the family: handled above and below)
  if (const char* why = fused_tile_refusal(TILE_BALANCE, t)) return why;
  if (!fused_supports(n, true)) return "engine FUSED_COOP serves padded hidden width 64 (width 33..64) only";
  Net n1 = n; n1.k = 0; n1.K1 = 1;
  if (!fused_supports(n1, true)) return "the fidelity pass has no fused gradient kernel for this network";
  return nullptr;
}
namespace {
struct BalLayout { ExtLayout e; int64_t partials, total; };
BalLayout bal_layout(const Net& n, const Geo& g, int64_t N_res, int64_t N_fid) {
  BalLayout b;
  b.e = ext_layout(n, g, N_res, N_fid);
  b.partials = b.e.total;
  b.total = b.partials + align256(((n.n_params() + 63) / 64) * 2 * PINN_BALANCE_STATS * (int64_t)sizeof(double));
  return b;
}
}  // namespace
int64_t fused_adam_bal_workspace_bytes(const Net& n, int64_t N_res, int64_t N_fid) {
  return bal_layout(n, geo_of(n), N_res, N_fid).total;
}
int fused_adam_bal(const Net& n, const AdamBalReq& q, const float* X, int64_t N_res, void* ws, int64_t ws_bytes, hipStream_t s) {
  if (const char* why = fused_adam_bal_refusal(n)) {
    set_error("fused engine, pinn_adam_loop_balanced: %s", why); return PINN_ERR_UNSUPPORTED;
  }
  const Geo g = geo_of(n);
  const BalLayout B = bal_layout(n, g, N_res, q.N_fid);
  const ExtLayout& L = B.e;
  if (int rc = check_workspace(ws, ws_bytes, B.total)) return rc;
  char* base = (char*)ws;
  Net n1 = n; n1.k = 0; n1.K1 = 1;
  const int64_t np = n.n_params();
  BalFinish f;
  memset(&f, 0, sizeof(f));
  f.param_blocks = (int)((np + 63) / 64);
  f.n_terms = q.res.n_terms; f.n_cols = q.fid.n_cols; f.row_cols = q.row_cols;
  f.term_sums = q.res.sums; f.col_sums = q.col_sums; f.grad = q.res.grad;
  f.params = q.adam.params; f.m = q.adam.m; f.v = q.adam.v;
  f.Wp = (float*)(base + L.w.wp); f.WTp = (float*)(base + L.w.wtp); f.Bp = (float*)(base + L.w.bp);
  f.n_loss_rows = q.adam.n_loss_rows; f.loss_rows = q.adam.loss_rows;
  f.lam = q.lam; f.group_grads = q.group_grads;
  double* partials = (double*)(base + B.partials);
  for (int i = 0; i < q.n_iters; ++i) {
    PassOnly pr = {L.w.scratch, L.w.wg_sums, L.w.wg_grads, i == 0 && !q.adam.packed_valid, 0, 0, true};
    int rc = run(n, true, &q.res, q.adam.params, X, N_res, nullptr, nullptr, ws, ws_bytes, s, nullptr, nullptr, &pr);
    if (rc) return rc;
    PassOnly pf = {L.w.scratch, L.sums_f, L.grads_f, false, 0, 0, true};
    rc = run(n1, true, &q.fid, q.adam.params, q.Xf, q.N_fid, nullptr, nullptr, ws, ws_bytes, s, nullptr, nullptr, &pf);
    if (rc) return rc;
    f.wg_r = (const float*)(base + L.w.wg_grads); f.copies_r = pr.n_copies; f.sums_r = (const float*)(base + L.w.wg_sums); f.grid_r = pr.grid;
    f.wg_f = (const float*)(base + L.grads_f); f.copies_f = pf.n_copies; f.sums_f = (const float*)(base + L.sums_f); f.grid_f = pf.grid;
    if ((q.step + i - 1) % q.every == 0) {   // statistics of the two gradients, the rule on lam
      hipLaunchKernelGGL(k_bal_stats, dim3((unsigned)f.param_blocks), dim3(256), 0, s, n, g.WP, g.PP, g.PW, f.wg_r, f.copies_r,
                         f.wg_f, f.copies_f, partials);
      hipLaunchKernelGGL(k_bal_weights, dim3(1), dim3(256), 0, s, q.mode, q.ref, q.alpha, np, (const double*)partials,
                         f.param_blocks, q.lam, q.stats_log ? q.stats_log + (int64_t)i * 2 * PINN_BALANCE_STATS : nullptr);
    }
    f.c = adam_scalars(q.lr[i], q.beta1, q.beta2, q.eps, q.step + i);
    f.losses = q.adam.n_loss_rows > 0 ? q.adam.losses + (int64_t)i * q.adam.n_loss_rows : nullptr;
    f.lam_log = q.lam_log ? q.lam_log + (int64_t)i * 2 : nullptr;
    hipLaunchKernelGGL(k_finish_adam_bal, dim3((unsigned)f.param_blocks + 1), dim3(256), 0, s, n, g.WP, g.PP, g.PW, f);
    rc = check_launch("fused finish + adam (balanced)");
    if (rc) return rc;
  }
  return PINN_OK;
}

int64_t fused_fields_workspace_bytes(const Net& n) {
  if (fused_tile_refusal(TILE_FIELD, n)) return -1;
  return ws_layout(n, geo_of(n), 1, true).total;
}

int fused_residual_fields(const Net& n, const pinn_residual_spec& spec, const float* params, const float* X, int64_t N,
                          float* fields, void* ws, int64_t ws_bytes, hipStream_t s) {
  if (const char* why = fused_tile_refusal(TILE_FIELD, n)) { set_error("fused engine: %s", why); return PINN_ERR_UNSUPPORTED; }
  const FieldReq fld{spec, fields};
  return run(n, false, nullptr, params, X, N, nullptr, nullptr, ws, ws_bytes, s, nullptr, &fld);
}

// The folded update needs the whole request in ONE pass (the split request on the width-64 tile kernel runs as two).
bool fused_supports_adam(const Net& n, const LossReq& rq, int64_t N) {
  if (!rq.grad || !fused_supports(n, true)) return false;
  if (rq.kind == 2 && rq.n_split >= 0) {
    const Geo g = geo_of(n);
    if (g.WP == 64 && !is_pec(&rq) && !use_coop(n, g, true, N)) return false;   // (EPI_PEC carries the split code at every width)
  }
  return true;
}

int64_t fused_workspace_bytes(const Net& n, int64_t N) {
  if (!fused_supports(n, false) && !fused_supports(n, true)) return -1;   // (dropout: gradient passes only)
  return ws_layout(n, geo_of(n), N > 0 ? N : 1).total;
}

int fused_forward(const Net& n, const float* params, const float* X, int64_t N, float* Y, float* dY, void* ws,
                  int64_t ws_bytes, hipStream_t s) {
  return run(n, false, nullptr, params, X, N, Y, dY, ws, ws_bytes, s);
}

int fused_jet_backward(const Net& n, const float* params, const float* X, int64_t N, const float* gY, const float* gdY,
                       float* grad, void* ws, int64_t ws_bytes, hipStream_t s) {
  if (const char* why = fused_tile_refusal(TILE_ADJ, n)) { set_error("fused engine: %s", why); return PINN_ERR_UNSUPPORTED; }
  const AdjReq adj{gY, gdY, grad};
  return run(n, true, nullptr, params, X, N, nullptr, nullptr, ws, ws_bytes, s, &adj);
}

int fused_loss(const Net& n, const LossReq& rq, const float* params, const float* X, int64_t N, void* ws,
               int64_t ws_bytes, hipStream_t s) {
  const bool grad = rq.grad != nullptr;
  if (rq.kind == 2 && rq.n_split >= 0) {
    // Split mode lives in the cooperative kernel and the narrow (WP < 64) tile kernels only.  A
    // request that would run on the width-64 tile kernel (large N, where a second launch is noise)
    // is served as two passes on the same stream: residual on the collocation points, then the
    // fidelity columns on the rest with the k = 0 network.
    // (the corrected residual's width-64 instances carry the split code: they are not the register-starved generic ones)
    const Geo g = geo_of(n);
    if (g.WP == 64 && !is_pec(&rq) && !use_coop(n, g, grad, N)) {
      LossReq r0 = rq; r0.kind = 0; r0.n_split = -1;
      int rc = PINN_OK;
      if (rq.n_split > 0) rc = fused_loss(n, r0, params, X, rq.n_split, ws, ws_bytes, s);
      else (void)hipMemsetAsync(rq.sums, 0, rq.n_terms * sizeof(float), s);
      if (rc) return rc;
      LossReq r1 = rq; r1.kind = 1; r1.n_split = -1;
      Net n1 = n; n1.k = 0; n1.K1 = 1;
      return fused_loss(n1, r1, params, X + rq.n_split * n.d_in, N - rq.n_split, ws, ws_bytes, s);
    }
  }
  if (!fused_supports(n, grad)) { set_error("fused engine: no kernel for this request (k = %d, gradient %d)", n.k, (int)grad); return PINN_ERR_UNSUPPORTED; }
  return run(n, grad, &rq, params, X, N, nullptr, nullptr, ws, ws_bytes, s);
}

// ---- ensembles: M members through one launch of the tile kernel's ensemble instances (fused_kernel.h, k_fused_ens) ------
namespace {

// The launch geometry of a member is the single-network gradient pass's (run() above: LDS, workgroups per CU), with the
// grid clamped so that the M members together stay within the tile kernel's workgroup cap for the shape.
struct EnsPlan {
  int gx; bool acc_lds; size_t lds;
  int64_t wp, wtp, bp, scratch, wg_sums, wg_grads, total;   // workspace layout: M members' shares of each region, back to back
};
EnsPlan ens_plan(const Net& n, const Geo& g, int M, int64_t N) {
  EnsPlan e;
  e.acc_lds = fits_lds(g);
  e.lds = (size_t)(e.acc_lds ? g.PP : 0) * 4 + (size_t)lds_fixed_bytes();
  const bool one_per_cu = e.acc_lds && !(g.WP <= 32 && 2 * (int64_t)e.lds <= LDS_LIMIT);
  // (workgroups per CU: the single-network rule, with the ensemble instances' own waves per SIMD at width 16 — two, so the
  // else-branch's 2 is what every narrow shape gets; kept in the rule's form so that the two stay comparable)
  const int wgs = g.WP == 16 ? FUSED_ENS_W16_WAVES : tile_wgs_per_cu(g.WP);
  const int per_cu = wgs * (int64_t)e.lds <= LDS_LIMIT ? wgs : 2;
  const int64_t cap = (int64_t)cu_count() * (one_per_cu ? 1 : per_cu);
  const int64_t most = cap / M > 1 ? cap / M : 1;
  const int want = grid_for((N + 15) / 16, one_per_cu, per_cu);
  e.gx = (int)(want < most ? want : most);
  int64_t off = 0;
  e.wp = off; off += align256((int64_t)M * g.PW * 4);
  e.wtp = off; off += align256((int64_t)M * g.PW * 4);
  e.bp = off; off += align256((int64_t)M * g.PB * 4);
  e.scratch = off; off += align256((int64_t)M * e.gx * FUSED_WAVES * n.L * n.K1 * g.NTH * 256 * 4);
  e.wg_sums = off; off += align256((int64_t)M * e.gx * MAX_SUMS * 4);
  e.wg_grads = off; off += align256((int64_t)M * e.gx * g.PP * 4);
  e.total = off;
  return e;
}

}  // namespace

const char* fused_ensemble_refusal(const Net& n, const LossReq& rq) {
  // (the descriptor's rule first: the entries decide it before they have a request, pinn_abi.hip ensemble_net)
  if (const char* why = fused_tile_refusal(TILE_ENSEMBLE, n)) return why;
  if (is_wave(&rq)) return "the wave closure (spec.flags bits 0 and 1) has no ensemble kernel";
  if (is_pec(&rq)) return "the corrected radiation stress (spec.flags bit 0) has no ensemble kernel";
  if (rq.kind == 2 && rq.n_split >= 0 && padded_width(n.W) == 64)
    return "the split request (0 <= n_res < N) at hidden width 33..64: the tile kernel carries no split code there";
  return nullptr;
}

void fused_ensemble_plan(const Net& n, int M, int64_t N, int* gx, int* copy_in_lds, int64_t* ws_bytes) {
  const EnsPlan e = ens_plan(n, geo_of(n), M, N);
  if (gx) *gx = e.gx;
  if (copy_in_lds) *copy_in_lds = e.acc_lds ? 1 : 0;
  if (ws_bytes) *ws_bytes = e.total;
}

int fused_ensemble_loss(const Net& n, const LossReq& rq, int M, int flags, const float* params, const float* X, int64_t N,
                        void* ws, int64_t ws_bytes, hipStream_t s) {
  if (const char* why = fused_ensemble_refusal(n, rq)) { set_error("fused engine, ensemble: %s", why); return PINN_ERR_UNSUPPORTED; }
  const Geo g = geo_of(n);
  const EnsPlan e = ens_plan(n, g, M, N);
  if (int rc = check_workspace(ws, ws_bytes, e.total)) return rc;
  char* base = (char*)ws;
  FusedParams P;
  memset(&P, 0, sizeof(P));
  P.d_in = n.d_in; P.d_out = n.d_out; P.L = n.L; P.act = n.act;
  for (int j = 0; j < PINN_MAX_DIRS; ++j) P.dir_col[j] = n.dir_col[j];
  P.N = N; P.n_tiles = (N + 15) / 16;
  P.X = X;
  P.Wp = (const float*)(base + e.wp); P.WTp = (const float*)(base + e.wtp); P.Bp = (const float*)(base + e.bp);
  P.scratch = (float*)(base + e.scratch);
  P.scratch_per_wave = (int64_t)n.L * n.K1 * g.NTH * 256;
  P.wg_sums = (float*)(base + e.wg_sums);
  P.wg_grads = (float*)(base + e.wg_grads);
  P.PW = g.PW; P.PB = g.PB;
  P.acc_lds = e.acc_lds ? 1 : 0;
  P.lds_acc_floats = e.acc_lds ? g.PP : 0;
  set_loss(P, n, rq);
  // the members' X / T strides: two flag bits in a field the tile kernel does not read (fused_kernel.h, ens_member)
  P.batch_T = ((flags & PINN_ENSEMBLE_OWN_X) ? ENS_OWN_X : 0) | ((flags & PINN_ENSEMBLE_OWN_T) && (P.loss_kind & 2) ? ENS_OWN_T : 0);

  const AdamReq* adam = rq.adam;
  const int packN = g.PW > g.PB ? g.PW : g.PB;
  if (!(adam && adam->packed_valid))
    hipLaunchKernelGGL(k_pack_ens, dim3((packN + 255) / 256, M), dim3(256), 0, s, n, g.WP, params, (float*)(base + e.wp),
                       (float*)(base + e.wtp), (float*)(base + e.bp), g.PW, g.PB, 0);
  if (!e.acc_lds) {   // global gradient copies start from zero
    if (hipMemsetAsync(P.wg_grads, 0, (size_t)M * e.gx * g.PP * 4, s) != hipSuccess) {
      set_error("hipMemsetAsync failed"); return PINN_ERR_LAUNCH;
    }
  }
  if (int rc = launch_tile(TF_ENS, g.WP, TileLaunch{n.K1, true, P, dim3(e.gx, M), e.lds, s})) return rc;
  const int64_t np = n.n_params();
  const int n_terms = (P.loss_kind & 1) ? rq.n_terms : 0, n_cols = (P.loss_kind & 2) ? rq.n_cols : 0;
  const EnsFinish f{(const float*)P.wg_grads, (const float*)P.wg_sums, rq.sums, rq.mse_sums, rq.grad};
  const dim3 fgrid((unsigned)((np + 63) / 64) + 1, M);
  if (adam) {
    hipLaunchKernelGGL(k_finish_adam_ens, fgrid, dim3(256), 0, s, n, g.WP, f, e.gx, g.PP, g.PW, n_terms, n_cols, rq.n_terms,
                       rq.n_cols, adam->params, adam->m, adam->v, (float*)(base + e.wp), (float*)(base + e.wtp),
                       (float*)(base + e.bp), adam->c, adam->n_loss_rows, adam->loss_rows, adam->losses, 0);
    return check_launch("fused ensemble finish + adam");
  }
  hipLaunchKernelGGL(k_finish_ens, fgrid, dim3(256), 0, s, n, g.WP, f, e.gx, g.PP, g.PW, n_terms, n_cols, rq.n_terms, rq.n_cols, 0);
  return check_launch("fused ensemble finish");
}

}  // namespace pinn
