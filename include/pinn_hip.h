/*
 * pinn_hip.h — C-ABI of libpinn_hip.so, the MI355X (gfx950) engine for the
 * PINN depth-inversion hot path: tanh-MLP forward + first- and second-order input
 * derivatives ("jets") + PDE residual loss + parameter gradient.
 *
 * The reference (rezasalatin/PINN_depthEstimation) has no FFI; its boundary is
 * the Python call surface.  Every entry point below names the reference code it
 * replaces (file:line under /root/reference):
 *
 *   pinn_forward            dnn.py:54-55          DNN.forward (nn.Sequential of Linear/Tanh)
 *   pinn_forward_jet        dnn.py:54-55 + physics.py:6-15   forward plus every
 *                           compute_gradient(out_c, in_j) column in one pass
 *   pinn_jet_backward       the double-backward torch runs under loss.backward()
 *                           (train.py:191) for a generic consumer of the jet
 *   pinn_forward_jet2       physics.py:6-15 applied twice: every second derivative
 *                           compute_gradient(compute_gradient(out_c, in_i), in_j)
 *   pinn_jet2_backward      loss.backward() (train.py:191) through those second derivatives
 *   pinn_residual_loss[_grad] physics.py:18-33,37-47,50-88,91-120 (continuity_only,
 *                           continuity_ftemp, Navier_Stokes, physics_equation)
 *                           fused with loss.backward() (train.py:154,191)
 *   pinn_residual_fields    the same four residuals' signed per-point fields (physics.py:81-83, 113-115, 20-23, 27-28),
 *                           before they are squared and averaged: residual maps, adaptive resampling
 *   pinn_residual2_loss_grad  Navier_Stokes / physics_equation with the lateral-mixing term nu * lap(U) in the momentum
 *                           equations (nested compute_gradient, physics.py:6-15) fused with loss.backward()
 *   pinn_residual_coef_loss_grad  Navier_Stokes / physics_equation with gamma_b (physics.py:76) / Cd (physics.py:99) read from a
 *                           device array, and the gradient with respect to them: the closures as trainable unknowns
 *   pinn_residual_weighted_loss_grad  the four residuals with one weight per collocation point (and term) on the squares:
 *                           masks, confidence maps, importance weights, self-adaptive weights; optionally the signed
 *                           per-point fields out of the same pass
 *   pinn_mse_loss_grad      train.py:131-141 (weighted fidelity MSE) + backward
 *   pinn_residual_mse_loss_grad  train_newmethod.py:122-159 (both on one forward) + backward
 *   pinn_residual_mse_split_loss_grad  train.py:131-157 (fidelity set + collocation set, one launch)
 *   pinn_lbfgs_push / pinn_lbfgs_direction  torch.optim.LBFGS's two-loop recursion (train.py:116-125,200)
 *   pinn_lbfgs_loop         torch.optim.LBFGS.step(closure) with the strong-Wolfe line search (train.py:116-125,195-200): runs of
 *                           evaluations enqueued by one call, every decision taken on the device
 *   pinn_adam_step          torch.optim.Adam.step as called at train.py:192
 *   pinn_loss_grad_adam_step  train.py:189-193 (loss_func + backward + Adam.step) in two launches
 *   pinn_adam_loop          train.py:188-193, n iterations of the above enqueued by one call
 *   pinn_adam_loop_ext      the same for the residual with runtime coefficients or point weights (fixed or self-adaptive):
 *                           three launches per iteration, the coefficients' / multipliers' Adam step on the device
 *   pinn_balance_update     the weights of the loss terms, which the reference sets by hand (train.py:94-95,157: weight_fid,
 *                           weight_res), set from the terms' own gradients instead: statistics, update, weighted combination
 *   pinn_adam_loop_balanced train.py:188-193 with the residual and the fidelity gradient balanced that way on the device
 *
 * Conventions
 *   - plain C, no exceptions; every function returns 0 on success, <0 on error;
 *     pinn_last_error() returns a thread-local message for the last failure.
 *   - every pointer named params/X/Y/dY/T/grad/... is a DEVICE pointer owned by
 *     the caller; the library allocates nothing that outlives a call.
 *   - params: flat fp32 [W_0, b_0, W_1, b_1, ... W_L, b_L]; W_l is (out_l, in_l)
 *     row-major — torch's nn.Linear.weight layout, state_dict order
 *     layers.layer_{l}.weight / .bias (dnn.py:32-35).
 *   - X: (N, d_in) row-major fp32 (what torch.cat([... (N,1) ...], -1) yields,
 *     train.py:132,148).  Y: (N, d_out) row-major.  dY: (k, N, d_out): dY[j] is
 *     d Y / d X[:, dir_col[j]] per point.
 *   - stream: a hipStream_t passed as void* (torch's current stream).  Calls only
 *     enqueue work; they never synchronise the device or the stream.
 *   - workspace: query with pinn_query_workspace, allocate once, pass to calls.
 *
 * Buffer contract (pinned by tests/test_abi_contract_gpu.py: guard bands around every buffer, workspaces full of 1e30)
 *   - The workspace may hold ANYTHING on entry: every call writes what it reads (packed weights with their padding,
 *     spill slots, partial sums, gradient copies) and reads no integer, offset or pointer from it.  The one exception
 *     is the caller's own promise adam->packed_valid (pinn_loss_grad_adam_step).
 *   - One workspace may be reused across calls of any kind, descriptor, engine, precision and N, in any order, as long
 *     as it is at least as large as the query for the call at hand; no call writes past the size queried for it.
 *     Results do not depend on the calls that came before.
 *   - Outputs are written at exactly their stated extents, ragged last tiles and padded columns included: Y (N, d_out),
 *     dY (k, N, d_out), d2Y (P, N, d_out), fields (n_fields, N), term_sums (n_terms), col_sums (n_cols), grad_flat /
 *     m / v / params (P), losses (n_loss_rows, or n_iters x n_loss_rows), out2 (2), n_rows_out (1), d (P), tmp (4m),
 *     coef (2m), q (P); X_out up to its capacity of ceil(ny/ix) * ceil(nx/iy) rows (rows past n_rows_out: unspecified).
 *   - Read-only, never written: params (except by the Adam entries and pinn_adam_step), X, T, gY, gdY, gd2Y,
 *     term_scale, col_scale, loss_rows, grad of pinn_adam_step, data / grids / minmax, g, s, y; S, Y, M in
 *     pinn_lbfgs_direction; rows of S, Y other than `slot` and entries of M outside row and column `slot` in
 *     pinn_lbfgs_push.
 *   - grad_flat is += in pinn_jet_backward, pinn_jet2_backward, pinn_residual_loss_grad, pinn_residual2_loss_grad,
 *     pinn_residual_coef_loss_grad (whose coef_grad is += too; its coef is read-only), pinn_residual_weighted_loss_grad
 *     (whose point_w is read-only and whose fields, if given, are overwritten at (n_fields, N)), pinn_mse_loss_grad,
 *     pinn_residual_mse_loss_grad and pinn_residual_mse_split_loss_grad (the caller zeroes it, or accumulates several
 *     terms into it); it is OVERWRITTEN by pinn_loss_grad_adam_step, pinn_adam_loop, pinn_adam_loop_ext and
 *     pinn_adam_loop_balanced (whose lam is in/out and whose lam_log, stats_log rows and group_grads are overwritten).
 *     pinn_balance_update reads grads, updates lam in place and overwrites stats (G, 3) and grad_out (P).  Y, dY, d2Y, fields,
 *     term_sums, col_sums, losses, X_out, n_rows_out, out2 and d are overwritten, whatever they held.
 *   - pinn_lbfgs_loop: writes params (P), trace (n_slots x PINN_LBFGS_TRACE_COLS) and state (the bytes pinn_query_lbfgs_loop
 *     states) at those extents only; `state` is the one buffer whose content a call relies on (pinn_lbfgs_loop_init arms it).
 *   - N = 0 where it is accepted: the sums are zeroed, grad_flat and the workspace are not touched.
 */
#ifndef PINN_HIP_H
#define PINN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version 4 covers pinn_query_fields_workspace / pinn_residual_fields as well: they were ADDED to it (no existing entry,
 * struct or constant changed), so a caller built against the earlier version-4 header runs unchanged and the number
 * stays.  A caller that needs the two entries looks the symbols up. */
#define PINN_ABI_VERSION 4

#define PINN_MAX_DIRS 3   /* tangent directions (inputs with requires_grad) */
#define PINN_MAX_ROLES 8

/* Non-finite inputs.  A NaN anywhere in X, the parameters or the targets propagates as IEEE arithmetic propagates it: the
   point's row of every per-point output is NaN, and so are every sum that includes the point and the gradient.  An
   INFINITE entry of X is read as +-FLT_MAX by the fused MFMA kernels (tile, cooperative, batch, plain forward: their hidden
   layers are padded with zero-weight units, where 0 * inf would be NaN): the row is what the saturated network gives, a weight
   that is exactly 0 times that input gives 0, and the gradient stays finite.  GENERIC, WIDE and bf16 mode take the infinity
   as it is: w * inf saturates tanh, 0 * inf is NaN (the layer-0 weight gradient of that input column; the whole row where
   a real weight is 0).  The sine first layer reads X as it is on every engine: sin(inf) is NaN. */

/* activation (dnn.py:18-21) */
#define PINN_ACT_TANH 0        /* init_type == 'xavier'  */
#define PINN_ACT_LEAKY_RELU 1  /* init_type == 'kaiming', negative_slope 0.01 */
/* Fourier-feature first layer: a_1 = sin(W_0 x + b_0) on the FIRST hidden layer, tanh on every other hidden layer, the
   last layer bare (n_hidden == 1: the only hidden layer is the sine).  W_0 and b_0 are the ordinary first-layer
   parameters of the flat buffer: no struct gains a field.  The argument W_0 x + b_0 is formed in double; sine and cosine
   are within 7e-8 of fp64 for |W_0 x + b_0| <= 2^16 (tested), degrade slowly beyond 2^26 and mean nothing from 2^31 on.
   Served by the generic engine for every first-order request
   and by the fused tile kernel (AUTO, FUSED, FUSED_TILE) for the plain requests: forward, forward jet with k in {0, 2, 3},
   the residual / mse / merged / split loss calls and the folded Adam and L-BFGS loops on them.  Requests whose fused
   kernel has no sine instance (coefficients, point weights, corrected radiation stress, residual fields, pinn_jet_backward,
   dropout) run on the generic engine under AUTO and are refused under an explicit FUSED*; FUSED_COOP, FUSED_BATCH, WIDE,
   bf16, the ensemble entries and the second-order entries (jet2 / residual2) are refused with a message that names the
   sine first layer. */
#define PINN_ACT_SIN_TANH 2

/* engine selector (0 lets the library pick the fastest kernel that supports the shape) */
#define PINN_ENGINE_AUTO 0
#define PINN_ENGINE_GENERIC 1  /* layer-by-layer VALU kernels, any shape */
#define PINN_ENGINE_FUSED 2    /* MFMA chain kernel, one persistent launch, hidden width <= 64 */
#define PINN_ENGINE_WIDE 3     /* 64 < hidden width <= 256.  PINN_PREC_F32: one launch per layer, jets in HBM (wide_kernel.h);
                                * PINN_PREC_BF16: the chain engine, three kernels for all hidden matrices (chain_kernel.h) */
/* sub-values of PINN_ENGINE_FUSED: which of its kernels runs (AUTO / FUSED choose by point count).
 * They are part of the descriptor, not of the process environment: the library reads no
 * environment variables and keeps no mutable state that changes results. */
#define PINN_ENGINE_FUSED_TILE 4  /* one wave per 16-point tile (the large-N kernel) */
#define PINN_ENGINE_FUSED_COOP 5  /* four waves per tile (small point sets; padded hidden width 64 only) */
#define PINN_ENGINE_FUSED_BATCH 6 /* layer-major batches of tiles per wave (narrow nets: hidden width <= 32, tanh, gradient
                                   * passes and pinn_jet_backward; AUTO picks it from 4096 points; other requests fall back
                                   * to _TILE) */

/* GEMM operand precision.  Everything outside the MFMAs (tanh, residual, adjoints, gradient
 * accumulation, Adam) is fp32 in both modes. */
#define PINN_PREC_F32 0   /* v_mfma_f32_16x16x4_f32: exact fp32 (the reference's precision) */
#define PINN_PREC_BF16 1  /* v_mfma_f32_16x16x32_bf16: bf16 operands (weights split hi + lo, jets rounded to bf16), fp32 accumulate
                           * (BASELINE configs[3]); wide engine only.  A tolerance mode, not fp32 parity: loss / gradient within
                           * 5e-3 of the reference at 12 x 256 (measured 2.8e-3 / 3.3e-3, tests/test_config3_gpu.py) */

/* error codes */
#define PINN_OK 0
#define PINN_ERR_INVALID (-1)
#define PINN_ERR_UNSUPPORTED (-2)
#define PINN_ERR_WORKSPACE (-3)
#define PINN_ERR_LAUNCH (-4)

typedef struct pinn_desc {
  int32_t d_in;       /* config layers.input_features  (train.py:52) */
  int32_t d_out;      /* config layers.output_features (train.py:55) */
  int32_t n_hidden;   /* config layers.hidden_layers   (train.py:53) */
  int32_t width;      /* config layers.hidden_width    (train.py:54) */
  int32_t k;          /* number of inputs with requires_grad "true" (train.py:87) */
  int32_t dir_col[PINN_MAX_DIRS]; /* X column of tangent direction j */
  int32_t activation; /* PINN_ACT_* */
  int32_t engine;     /* PINN_ENGINE_* */
  int32_t precision;  /* PINN_PREC_*: operand type of the weight GEMMs */
  /* nn.Dropout(dropout_rate) after every hidden activation (dnn.py:38) while the module is in training mode
   * (train.py:186).  0 = identity (eval mode, and every config the reference ships).  The keep mask of unit f of
   * hidden layer l at point n is a pure function of (dropout_seed, l, f, n) — pinn_dropout_keep below — so a
   * forward call and the reverse sweep that follows it (same seed) see the same mask without storing it; the caller
   * draws a new seed per forward pass.  Kept units are scaled by 1 / (1 - p), tangents included.
   * Gradient passes of tanh networks of hidden width 33..64 run on the fused tile kernel's dropout instances (the mask
   * re-derived in registers); every other call with dropout_p > 0 runs on the generic engine.  AUTO picks accordingly;
   * FUSED is refused for requests it does not serve, WIDE always.
   * pinn_residual_mse_split_loss_grad on those dropout instances runs as two passes (collocation points, then fidelity
   * points): the mask's point index restarts at 0 at the first fidelity point, as it does at every chunk of
   * pinn_residual_fields' staged path.  On the generic engine the index runs through all N points. */
  float dropout_p;
  uint32_t dropout_seed;
} pinn_desc;

/* residual ids */
#define PINN_RES_NAVIER_STOKES 1     /* physics.py:50-88  roles out: h,z,u,v   dirs: t,x,y */
#define PINN_RES_PHYSICS_EQUATION 2  /* physics.py:91-120 roles out: h,U,V,eta_mean,Hrms,k  dirs: x,y */
#define PINN_RES_CONTINUITY_FTEMP 3  /* physics.py:37-47  roles out: h,U,V     dirs: x,y */
#define PINN_RES_CONTINUITY_ONLY 4   /* physics.py:18-33  same + h anchor where x < 25.5 */

/* number of loss terms each residual reports (sums of squares, un-normalised) */
#define PINN_NS_TERMS 3   /* sum fc^2, sum fm_x^2, sum fm_y^2 */
#define PINN_PE_TERMS 3   /* sum fc^2, sum fx^2,  sum fy^2  */
#define PINN_PEW_TERMS 5  /* physics_equation with flags bits 0 and 1 (the wave closure): those three, sum f_d^2, sum f_E^2;
                             its per-point fields are the same five, (fc, fx, fy, f_d, f_E) */
#define PINN_CF_TERMS 1   /* sum fc^2 */
#define PINN_CO_TERMS 3   /* sum fc^2, sum_{x<thr} (h-anchor)^2, count{x<thr} */

typedef struct pinn_residual_spec {
  int32_t residual_id;
  int32_t out_col[PINN_MAX_ROLES]; /* output column of each role, in the role order above; the network may have MORE
                                      output columns than roles, in any order (entries beyond the residual's roles
                                      are ignored, whatever they hold) */
  int32_t dir_of[PINN_MAX_DIRS];   /* index into desc.dir_col of each direction role (entries beyond the residual's
                                      directions are ignored) */
  int32_t flags;                   /* bit 0 with residual_id == PINN_RES_PHYSICS_EQUATION: the corrected radiation stress,
                                      E = rho g Hrms^2 / 8, Sxx = E (2n + 1/2), Syy = E n, n = kh / sinh 2kh, in place of
                                      the reference's E == 0 (physics.py:106); same roles, directions, terms and fields.
                                      Honoured by every entry that takes a spec (engine rules: pinn_residual_loss_grad
                                      and pinn_residual_fields below).
                                      bit 1 with residual_id == PINN_RES_PHYSICS_EQUATION, on top of bit 0: the wave closure —
                                      two more terms and fields (PINN_PEW_TERMS = 5), with s = k h, G = 9.81,
                                      omega = param[0] (rad/s), gamma = param[1] (breaker index):
                                        f_d = G k tanh(s) / omega^2 - 1                   (linear dispersion)
                                        f_E = d/dx (Hrms^2 c_g) + eps,  c_g = (omega / k) (1/2 + n(s))
                                        eps = (3 sqrt(pi) / 2) (omega / 2 pi) Hrms^5 / (gamma^2 h^3) [1 - (1 + q^2)^(-5/2)],
                                        q = Hrms / (gamma h)      (Thornton & Guza 1983, B = 1; the energy equation divided
                                        by rho g / 8; waves travel along +x, as Sxy = 0 has it)
                                      k > 0 and h > 0 are the caller's to ensure (non-finite values propagate).  Bit 1
                                      without bit 0, param[0] <= 0 or param[1] <= 0: PINN_ERR_INVALID, "wave" in the
                                      message, before any device work.  Engine rules: pinn_residual_loss below; every entry
                                      that takes a spec serves the request or refuses it with "wave" in the message.
                                      Bits 0 and 1 on the other residuals and all other bits are ignored. */
  float param[4];                  /* continuity_only: param[0]=threshold (25.5), param[1]=anchor (0.75);
                                      physics_equation with flags bit 1: param[0]=omega, param[1]=gamma */
} pinn_residual_spec;

int32_t pinn_version(void);

/* 1 if unit `feature` of hidden layer `layer` (0-based) is kept at point `point` under (seed, p) — the exact mask
 * the kernels apply (host evaluation of the same function; for tests and for callers that want the mask). */
int32_t pinn_dropout_keep(uint32_t seed, int32_t layer, int32_t feature, int64_t point, float p);
const char* pinn_last_error(void);

/* The corrected physics_equation residual (spec.flags bit 0) at ONE point, evaluated on the host by the very functions the
 * kernels call (for tests and for callers that want to check a jet by hand; no device is touched).
 * v[c * 6 + r]: c = 0 the value, 1 the x-derivative, 2 the y-derivative of role r = h, U, V, eta_mean, Hrms, k.
 * fields <- (fc, fx, fy).  g[c * 6 + r] <- sum_t scale[t] * d(field_t^2) / dv; with scale or g NULL only the fields are
 * formed and g is left alone.  At kh = 0 the stress ratio takes its limit (n = 1/2, n' = 0, n'' = -2/3). */
int32_t pinn_pe_corrected_point(const float v[18], const float scale[3], float fields[3], float g[18]);
/* ... and with the wave closure (spec.flags bits 0 and 1), same conventions: fields <- (fc, fx, fy, f_d, f_E), five scales.
 * omega <= 0 or gamma <= 0: PINN_ERR_INVALID.  k = 0 or h = 0 give non-finite values, as in the kernels. */
int32_t pinn_pe_wave_point(const float v[18], float omega, float gamma, const float scale[5], float fields[5], float g[18]);

/* P = sum_l (in_l*out_l + out_l), layers = [d_in] + [width]*n_hidden + [d_out] (train.py:56) */
int32_t pinn_param_count(const pinn_desc* desc, int64_t* count);

/* bytes of workspace a call on N points needs with the engine desc->engine selects: enough for every call on
 * that descriptor, pinn_jet_backward included (which picks its engine by the rules stated at its declaration). */
int32_t pinn_query_workspace(const pinn_desc* desc, int64_t N, int64_t* bytes);

int32_t pinn_forward(const pinn_desc* desc, const float* params, const float* X, int64_t N,
                     float* Y, void* ws, int64_t ws_bytes, void* stream);

int32_t pinn_forward_jet(const pinn_desc* desc, const float* params, const float* X, int64_t N,
                         float* Y, float* dY, void* ws, int64_t ws_bytes, void* stream);

/* grad_flat (P,) += d/dtheta [ sum(gY*Y) + sum(gdY*dY) ];  gY or gdY may be NULL (treated as 0).  gdY is (k, N, d_out)
 * in the order of desc->dir_col, as pinn_forward_jet writes dY.
 * Engines.  GENERIC: the layer-wise kernels, any shape.  FUSED: fp32, width <= 64, d_in and d_out <= 16, tanh or LeakyReLU,
 * k in {0, 2, 3} or gdY == NULL, dropout_p == 0; anything else is refused with PINN_ERR_UNSUPPORTED and the reason in
 * pinn_last_error().  WIDE: refused.  AUTO: the MFMA path where FUSED would be served, otherwise GENERIC.
 * FUSED has two kernels for this call, both with the caller's adjoints in place of a residual.  The batch kernel serves
 * what it serves for a gradient request: tanh, width <= 32, d_in <= 8, k in {2, 3} with gdY.  FUSED_BATCH forces it at any
 * N; FUSED and AUTO take it from PINN_JET_BACKWARD_BATCH_MIN_TILES 16-point tiles on and the tile kernel below; FUSED_TILE
 * and FUSED_COOP keep the tile kernel.  Every other served request (LeakyReLU, k = 0 or gdY == NULL, d_in > 8, width
 * 33..64) runs on the tile kernel under every FUSED value, FUSED_BATCH included.  pinn_jet_backward_kernel below tells
 * which kernel a call would run.
 * Reproducibility.  GENERIC is bit-reproducible from run to run.  The tile kernel launches one workgroup per 16-point
 * tile, up to W workgroups (W = 1 to 3 per compute unit, by shape); while N <= 16 * W every gradient copy is
 * added to by a single wave in program order and the copies are summed in a fixed order: bit-reproducible.  Above that
 * size several waves share a copy and two runs differ in the last bits, as for every other fused gradient call.
 * The batch kernel, where four gradient copies fit in LDS (e.g. 10 x 10): a copy per wave, no lock and no atomic, each
 * wave adds in program order, the four copies and then the workgroups are summed in a fixed order: bit-reproducible at
 * every N on a given device.  Where the gradient is too large for that (e.g. 40 x 20, 100 x 20) the batch kernel adds
 * into shared copies with atomics and two runs differ in the last bits at every N. */
int32_t pinn_jet_backward(const pinn_desc* desc, const float* params, const float* X, int64_t N,
                          const float* gY, const float* gdY, float* grad_flat,
                          void* ws, int64_t ws_bytes, void* stream);

/* AUTO / FUSED run pinn_jet_backward on the batch kernel from this many 16-point tiles on (4096 points; measured on
 * MI355X at 10 x 10, 20 x 20 and 100 x 20: DESIGN.md 2.4b) */
#define PINN_JET_BACKWARD_BATCH_MIN_TILES 256

/* *kernel = the kernel a pinn_jet_backward call with this descriptor, N and gdY (with_gdY != 0) or without would run:
 * PINN_ENGINE_GENERIC, PINN_ENGINE_FUSED_TILE or PINN_ENGINE_FUSED_BATCH.  A request the call refuses is refused here
 * with the same code and message.  Host logic only: no device is needed or touched. */
int32_t pinn_jet_backward_kernel(const pinn_desc* desc, int64_t N, int32_t with_gdY, int32_t* kernel);

/* ---- second-order jets --------------------------------------------------------------------------------------------
 * k = desc->k differentiated inputs (1..3) give P = k (k + 1) / 2 unordered pairs (i, j), i <= j, stored upper triangle
 * row-major: (0,0), (0,1), .., (0,k-1), (1,1), ..  d2Y: (P, N, d_out), d2Y[p] = d^2 Y / d X[:, dir_col[i]] d X[:, dir_col[j]].
 * Engines: GENERIC runs the VALU layer kernels (any shape, tanh or LeakyReLU, dropout: the mask multiplies all three
 * orders).  FUSED (and its sub-values) runs the MFMA layer kernels (v_mfma_f32_16x16x4_f32): fp32, every layer at most
 * 64 wide, no dropout; other requests are refused with PINN_ERR_UNSUPPORTED (dropout named in its own message).  AUTO
 * takes the MFMA kernels where they apply, else the VALU ones.  WIDE and PINN_PREC_BF16 are refused; k = 0 is
 * PINN_ERR_INVALID.  The workspace of these calls is
 * their own (pinn_query_jet2_workspace); large point sets run in chunks, so it stops growing past about 1 GiB. */
int32_t pinn_query_jet2_workspace(const pinn_desc* desc, int64_t N, int64_t* bytes);

/* physics.py:6-15 applied twice (train.py:191 differentiates the result once more, pinn_jet2_backward).
 * Y (N, d_out) and dY (k, N, d_out) as pinn_forward_jet, either may be NULL; d2Y (P, N, d_out) is required. */
int32_t pinn_forward_jet2(const pinn_desc* desc, const float* params, const float* X, int64_t N,
                          float* Y, float* dY, float* d2Y, void* ws, int64_t ws_bytes, void* stream);

/* train.py:191 through second derivatives: grad_flat (P,) += d/dtheta [ sum(gY*Y) + sum(gdY*dY) + sum(gd2Y*d2Y) ];
 * any of gY, gdY, gd2Y may be NULL (treated as 0). */
int32_t pinn_jet2_backward(const pinn_desc* desc, const float* params, const float* X, int64_t N,
                           const float* gY, const float* gdY, const float* gd2Y, float* grad_flat,
                           void* ws, int64_t ws_bytes, void* stream);

/* ---- lateral mixing nu * lap(U): the first hard-wired residual on the second-order jets -----------------------------
 * (added under ABI version 4, as the fields entries were: no existing entry, struct or constant changed)
 * With L_a = a_xx + a_yy and nu >= 0 the momentum fields become
 *   Navier_Stokes:     fm_x = (physics.py:82) - nu L_u,   fm_y = (physics.py:83) - nu L_v        (fc unchanged)
 *   physics_equation:  fx   = (physics.py:114) - nu L_U,  fy   = (physics.py:115) - nu L_V       (plain and flags bit 0)
 * The derivatives are with respect to the network's inputs AS IT SEES THEM: in the reference's pipeline those are
 * normalised to [-1, 1] (operations.py:4-8), so nu is in those units.  nu == 0 is valid and gives the first-order residual.
 *
 * pinn_residual2_point: one point on the host, by the very functions the kernel calls (no device is touched).
 * v[c * NR + r]: c = 0 the value, 1 + d the derivative along direction role d, of role r (NR = 4 roles and 3 directions
 * for Navier_Stokes, 6 and 2 for physics_equation); lap = (L_u, L_v) resp. (L_U, L_V).  fields <- (fc, f_x, f_y).
 * With scale, g and glap all given: g[c * NR + r] <- sum_t scale[t] d(field_t^2) / dv and glap <- the adjoints of lap,
 * (-nu rx, -nu ry) with rx = 2 scale[1] f_x, ry = 2 scale[2] f_y: the adjoint of the pairs (x, x) and (y, y) of the two
 * momentum roles; every other second-order adjoint is zero.  Any of the three NULL: fields only.
 * Continuity residuals: PINN_ERR_UNSUPPORTED ("no second-order term"). */
int32_t pinn_residual2_point(int32_t residual_id, int32_t flags, float nu, const float* v, const float lap[2],
                             const float* scale, float* fields, float* g, float glap[2]);

/* pinn_residual2_loss_grad: term_sums[t] <- sum over points of (shifted field t)^2 (n_terms floats, overwritten);
 * fields, if not NULL, (n_fields, N) <- the signed shifted fields (overwritten); grad_flat, if not NULL,
 * (P,) += sum_t term_scale[t] d term_sums[t] / d theta (NULL: no backward sweep; term_scale may then be NULL too).
 * term_scale is a DEVICE array as in pinn_residual_loss_grad.  N = 0 zeroes term_sums and touches nothing else.
 * Per chunk of points the call runs the forward layer kernels of pinn_forward_jet2 ONCE, one point-wise residual kernel
 * that writes the adjoint of every channel and output column in the workspace layout, and the backward layer kernels of
 * pinn_jet2_backward: no copy out of or into the workspace, no second forward.  All k (k + 1) / 2 pairs ride along.
 * The workspace is the call's own (pinn_query_residual2_workspace); large point sets run in chunks as for jet2.
 * Rules, decided before any device work, the same for the query (which takes no nu):
 *   nu negative or not finite                    PINN_ERR_INVALID
 *   desc->k != the residual's directions         PINN_ERR_UNSUPPORTED  (3 for Navier_Stokes, 2 for physics_equation)
 *   continuity_ftemp / continuity_only           PINN_ERR_UNSUPPORTED, "no second-order term" in the message
 *   GENERIC                                      any shape, tanh or LeakyReLU, dropout (the mask function of jet2)
 *   FUSED and its sub-values                     the MFMA layer kernels and an MFMA weight gradient: fp32, every layer at
 *                                                most 64 wide, no dropout; otherwise PINN_ERR_UNSUPPORTED with the two
 *                                                messages of pinn_forward_jet2
 *   AUTO                                         MFMA where served, else generic
 *   WIDE, PINN_PREC_BF16                         PINN_ERR_UNSUPPORTED
 * Reproducibility.  term_sums and fields: bit-reproducible on both paths (per-workgroup partial sums, then the fixed-order
 * double reduction of every loss entry).  grad_flat: both weight-gradient kernels add with float atomics, so two runs
 * differ in the last bits once more than one workgroup adds to an element: on the MFMA path from 65 points of a chunk
 * on, on the generic path from 513 points on; below that size the gradient is bit-reproducible too. */
int32_t pinn_query_residual2_workspace(const pinn_desc* desc, const pinn_residual_spec* spec, int64_t N, int64_t* bytes);
int32_t pinn_residual2_loss_grad(const pinn_desc* desc, const pinn_residual_spec* spec, float nu,
                                 const float* term_scale, const float* params, const float* X, int64_t N,
                                 float* term_sums, float* fields /* NULL or (n_fields, N) */,
                                 float* grad_flat /* NULL: no backward sweep */,
                                 void* ws, int64_t ws_bytes, void* stream);

/* ---- runtime closure coefficients: train gamma_b and Cd alongside the network -----------------------------------------
 * (added under ABI version 4, as the fields and residual2 entries were: no existing entry, struct or constant changed)
 * The first-order residuals' physical closures as an optional DEVICE array instead of compile-time constants:
 *   Navier_Stokes                 coef[0] = gamma_b, default 0.78    CB = 3/16 g gamma_b^2 in Fbr_x, Fbr_y (physics.py:76-78)
 *   physics_equation (plain)      coef[0] = Cd,      default 0.002   tau_b = rho Cd U|U|              (physics.py:99-103)
 * The continuity residuals have no coefficient (PINN_ERR_UNSUPPORTED, "no coefficient" in the message); neither has the
 * corrected radiation stress (spec.flags bit 0: PINN_ERR_UNSUPPORTED, "corrected" in the message).
 * The coefficients are a device array so that an optimiser updates them without a host round trip, as term_scale.  It
 * follows that NO ENTRY VALIDATES THEIR VALUES: a negative, huge or non-finite coefficient is evaluated as given, and
 * what it does to the sums and gradients is the caller's business. */
#define PINN_MAX_COEFS 4
/* *n <- the number of coefficients of the residual: 1, 1, 0, 0 for the four ids (0 for physics_equation with flags bit 0) */
int32_t pinn_residual_coef_count(int32_t residual_id, int32_t flags, int32_t* n);
/* *value <- the default of coefficient j: the constant the other entries have compiled in */
int32_t pinn_residual_coef_default(int32_t residual_id, int32_t j, float* value);

/* pinn_residual_coef_point: one point on the host, by the very functions the kernels call (no device is touched; coef is a
 * HOST array here).  v as in pinn_residual2_point: v[c * NR + r], c = 0 the value, 1 + d the derivative along direction
 * role d, of role r (NR = 4 roles and 3 directions for Navier_Stokes, 6 and 2 for physics_equation).
 * fields <- (fc, f_x, f_y) with the given coefficient.  With scale, g and gcoef all given: g[c * NR + r] <- sum_t scale[t]
 * d(field_t^2) / dv and gcoef[j] <- d/d coef[j] sum_t scale[t] field_t^2:
 *   Navier_Stokes      (rx Hx H + ry Hy H) 3/8 g gamma_b,   H = h + z
 *   physics_equation   D rho (rx U|U| + ry V|V|),           D = 1 / (rho (eta_mean + h))
 * with rx = 2 scale[1] f_x, ry = 2 scale[2] f_y.  Any of the three NULL: fields only.
 * At the default coefficients fields and g equal pinn_residual2_point's at nu = 0 to rounding, not bit for bit: the
 * products rho Cd and 3/16 g gamma_b^2 are formed in fp32 at run time here and in double at compile time there. */
int32_t pinn_residual_coef_point(int32_t residual_id, const float* v, const float* coef, const float* scale,
                                 float* fields, float* g, float* gcoef);

/* pinn_residual_coef_loss_grad: pinn_residual_loss_grad with the residual's coefficients read from `coef` (device, n_coef
 * floats, read-only; NULL is PINN_ERR_INVALID) and their gradient out of the same pass:
 *   term_sums (n_terms)  <- sum over points of field_t^2                                   (overwritten)
 *   grad_flat (P,)       += sum_t term_scale[t] d term_sums[t] / d theta
 *   coef_grad (n_coef,)  += sum_t term_scale[t] d term_sums[t] / d coef[j]
 * grad_flat == NULL: forward only (term_scale may then be NULL too, and coef_grad must be).  coef_grad == NULL with
 * grad_flat given: the coefficient VALUES only (a frozen coefficient).  N = 0 zeroes term_sums and touches nothing else.
 * The workspace is the call's own (pinn_query_residual_coef_workspace), so that AUTO may move between engines.
 * Rules, all decided before any device work; the query follows the same rules:
 *   desc->k != the residual's directions     PINN_ERR_UNSUPPORTED  (3 for Navier_Stokes, 2 for physics_equation)
 *   continuity_ftemp / continuity_only       PINN_ERR_UNSUPPORTED, "no coefficient" in the message
 *   spec.flags bit 0 (corrected stress)      PINN_ERR_UNSUPPORTED, "corrected" in the message
 *   GENERIC                                  any shape, tanh or LeakyReLU, dropout
 *   FUSED and FUSED_TILE                     the tile kernel's coefficient instances: fp32, tanh, width <= 64, d_in and
 *                                            d_out <= 16, dropout_p == 0; otherwise PINN_ERR_UNSUPPORTED with the reason
 *   FUSED_COOP, FUSED_BATCH, WIDE, bf16      PINN_ERR_UNSUPPORTED (no such instances)
 *   AUTO                                     the tile instances where FUSED is served, else GENERIC
 * Reproducibility.  term_sums and coef_grad: bit-reproducible from run to run on both engines (the coefficient gradient
 * is summed per workgroup beside the term sums and takes the same fixed-order double reduction).  A forward-only call
 * (grad_flat == NULL) returns the very bits of the gradient call's term_sums on the same engine: it runs on that call's
 * grid, and the fields are formed without fused multiply-adds so that every instance rounds them alike.  grad_flat: as for every
 * tile-kernel gradient call — several waves share a workgroup's gradient copy, so two runs differ in the last bits once a
 * workgroup holds more than one tile; on the generic engine the weight gradient adds with float atomics. */
int32_t pinn_query_residual_coef_workspace(const pinn_desc* desc, const pinn_residual_spec* spec, int64_t N, int64_t* bytes);
int32_t pinn_residual_coef_loss_grad(const pinn_desc* desc, const pinn_residual_spec* spec, const float* coef,
                                     const float* term_scale, const float* params, const float* X, int64_t N,
                                     float* term_sums, float* grad_flat /* NULL: no backward sweep */,
                                     float* coef_grad /* NULL: no coefficient gradient */,
                                     void* ws, int64_t ws_bytes, void* stream);

/* ---- per-point weights on the residual's squares ---------------------------------------------------------------------
 * pinn_residual_weighted_loss_grad: pinn_residual_loss_grad with a weight on every point's squared fields.
 * Let n_w = min(n_terms, n_fields) of the residual: 3, 3, 1, 2 for Navier_Stokes, physics_equation, continuity_ftemp,
 * continuity_only.  point_w is a device array (w_rows, N), row-major, read-only:
 *   w_rows == 1     one weight per point, shared by all weighted terms: w_t[n] = point_w[n]
 *   w_rows == n_w   row t weights term t:                               w_t[n] = point_w[t * N + n]
 *   any other w_rows, or point_w == NULL: PINN_ERR_INVALID
 *   term_sums (n_terms)  <- sum_n w_t[n] f_t[n]^2 for t < n_w, f_t being field t exactly as pinn_residual_fields defines
 *                           it                                                               (overwritten)
 *                           continuity_only's third term, the count of points with x < threshold, is NEVER weighted: it
 *                           is a normaliser, not a loss
 *   grad_flat (P,)       += sum_t term_scale[t] d term_sums[t] / d theta
 *   fields               NULL, or (n_fields, N): overwritten with the UNWEIGHTED SIGNED fields, the quantity
 *                           pinn_residual_fields writes.  The caller forms the gradient with respect to a weight from it:
 *                           d / d w_t[n] = term_scale[t] f_t[n]^2.  There is no further output.
 * grad_flat == NULL: forward only (term_scale may then be NULL too); with fields given this is loss plus residual map in
 * one pass.  N = 0 zeroes term_sums and touches nothing else.  The workspace is the call's own
 * (pinn_query_residual_weighted_workspace), so that AUTO may move between engines.
 * NO ENTRY VALIDATES THE WEIGHTS' VALUES, as for the coefficients above: they never leave the device.  A negative or
 * non-finite weight is evaluated as given.  A zero weight removes its point from the sums and the gradient only if the
 * point's residual is finite: 0 * inf is NaN.  The lanes of a ragged last tile read the weight of the last point of
 * the row, never past the row's end.
 * Rules, all decided before any device work; the query follows the same rules:
 *   desc->k != the residual's directions     PINN_ERR_UNSUPPORTED
 *   spec.flags bit 0 (corrected stress)      PINN_ERR_UNSUPPORTED, "corrected" in the message
 *   GENERIC                                  any shape, tanh or LeakyReLU, dropout
 *   FUSED and FUSED_TILE                     the tile kernel's weighted instances: fp32, tanh, width <= 64, d_in and
 *                                            d_out <= 16, dropout_p == 0; otherwise PINN_ERR_UNSUPPORTED with the reason
 *   FUSED_COOP, FUSED_BATCH, WIDE, bf16      PINN_ERR_UNSUPPORTED (no such instances)
 *   AUTO                                     the tile instances where FUSED is served, else GENERIC
 * Reproducibility.  term_sums and fields: bit-reproducible from run to run on both engines (per-workgroup sums, fixed-order
 * double reduction).  A forward-only call returns the very bits of the gradient call's term_sums on the same engine: it
 * runs on that call's grid.  grad_flat: as for every tile-kernel gradient call (see pinn_residual_coef_loss_grad). */
int32_t pinn_query_residual_weighted_workspace(const pinn_desc* desc, const pinn_residual_spec* spec, int64_t N, int64_t* bytes);
int32_t pinn_residual_weighted_loss_grad(const pinn_desc* desc, const pinn_residual_spec* spec,
                                         const float* term_scale,
                                         const float* point_w, int32_t w_rows,
                                         const float* params, const float* X, int64_t N,
                                         float* term_sums,
                                         float* fields    /* NULL or (n_fields, N) */,
                                         float* grad_flat /* NULL: no backward sweep */,
                                         void* ws, int64_t ws_bytes, void* stream);

/* term_sums[t] = sum over points of (residual field t)^2  (device, n_terms floats, overwritten)
 * Corrected radiation stress (spec.flags bit 0 on physics_equation) — the rule of every loss entry that takes a spec
 * (pinn_residual_loss, pinn_residual_loss_grad, pinn_residual_mse_loss_grad, pinn_residual_mse_split_loss_grad,
 * pinn_loss_grad_adam_step, pinn_adam_loop): the request runs on the engine the descriptor selects, or is refused with
 * PINN_ERR_UNSUPPORTED and the word "corrected" in pinn_last_error(); it is never moved to another engine (pinn_query_workspace
 * does not see the spec).  GENERIC: any shape, tanh or LeakyReLU, dropout, k = 2 or 3.  FUSED: tanh, k = 2, dropout_p == 0 — on
 * the batch kernel where a gradient request of that shape runs there, else on the tile kernel (also under FUSED_COOP and at
 * the small N where the cooperative kernel would serve the plain residual: it has no such instance); the split request is
 * one pass at every width.  LeakyReLU and k = 3 on FUSED are refused (use GENERIC).  Every descriptor whose engine comes out
 * as WIDE — width 65..256 under AUTO or WIDE, bf16 — is refused (use GENERIC).  With dropout_p > 0 AUTO runs the generic
 * engine (the fused dropout instances do not carry the corrected residual) and FUSED is refused.
 * Wave closure (spec.flags bits 0 and 1, PINN_PEW_TERMS term sums) — the same entries, the same rule with "wave" in every
 * refusal, and its own instances of the tile kernel only.  GENERIC: any shape, tanh or LeakyReLU, dropout, k = 2 or 3 (the
 * residual reads directions x and y).  AUTO, FUSED, FUSED_TILE: the tile kernel at every N, for tanh, k = 2, width <= 64,
 * dropout_p == 0 (never the batch or the cooperative kernel); the split request is one pass at every width.  FUSED_BATCH,
 * FUSED_COOP, every descriptor whose engine comes out as WIDE, the sine first layer under an explicit FUSED*, and LeakyReLU
 * or k = 3 on FUSED are refused (use GENERIC).  Dropout and the sine first layer under AUTO run the generic engine.  On the
 * fused engine at most 7 fidelity columns: the fifth term's partial sum takes the last column's slot (8: refused).
 * Out of scope, refused with "wave" in the message: the coefficient, weighted, ensemble, balanced-loop and
 * pinn_adam_loop_ext entries and pinn_residual2_* (nu together with the wave closure).  pinn_residual_coef_count gives 0. */
int32_t pinn_residual_loss(const pinn_desc* desc, const pinn_residual_spec* spec,
                           const float* params, const float* X, int64_t N,
                           float* term_sums, void* ws, int64_t ws_bytes, void* stream);

/* ---- per-point residual fields -----------------------------------------------------------------------------------
 * The residual's signed field values at every point, before squaring: Navier_Stokes (fc, fm_x, fm_y), physics_equation
 * (fc, fx, fy), continuity_ftemp / continuity_only (fc, da) with da = h - anchor on the points with x < threshold of
 * continuity_only and 0 everywhere else (always 0 for continuity_ftemp).  desc->k must equal the residual's number of
 * directions (3 for Navier_Stokes, 2 for the others): PINN_ERR_UNSUPPORTED otherwise.  N >= 1.
 * Engines.  FUSED (every sub-value: one MFMA kernel, the tile kernel run forward-only with a field-storing epilogue):
 * fp32, width <= 64, d_in and d_out <= 16, tanh or LeakyReLU, dropout_p == 0; anything else is refused with
 * PINN_ERR_UNSUPPORTED and the reason in pinn_last_error().  GENERIC, WIDE: the engine's pinn_forward_jet into a staging
 * area in the workspace, 65536 points at a time, then one point-wise fp32 kernel per chunk (the precision mode belongs to
 * the jet).  AUTO: the MFMA path where FUSED would be served, else the staged one on the engine AUTO picks for
 * pinn_forward_jet.  With dropout_p > 0 (staged path only) the mask's point index restarts at every chunk.
 * The call has a workspace of its own (pinn_query_workspace answers what it always did).
 * Corrected radiation stress (spec.flags bit 0 on physics_equation): k must be 2.  AUTO and FUSED run the tile kernel's own
 * field instances where FUSED serves fields and the network is tanh; LeakyReLU under FUSED is refused ("corrected" in the
 * message), under AUTO it is staged like every GENERIC and WIDE request.  pinn_query_fields_workspace takes the spec and
 * answers for the path the call will take.  The wave closure (bits 0 and 1): the same rule, five fields. */
#define PINN_NS_FIELDS 3
#define PINN_PE_FIELDS 3
#define PINN_CF_FIELDS 2
#define PINN_CO_FIELDS 2
int32_t pinn_query_fields_workspace(const pinn_desc* desc, const pinn_residual_spec* spec, int64_t N, int64_t* bytes);
/* fields (n_fields, N) row-major, overwritten: fields[f][n] = residual field f at X[n]
 * (physics.py:81-83, 113-115, 20-23, 27-28); sum_n fields[t][n]^2 == pinn_residual_loss's term_sums[t] */
int32_t pinn_residual_fields(const pinn_desc* desc, const pinn_residual_spec* spec, const float* params,
                             const float* X, int64_t N, float* fields,
                             void* ws, int64_t ws_bytes, void* stream);

/* as above, and grad_flat (P,) += sum_t term_scale[t] * d term_sums[t] / d theta.
 * term_scale is a DEVICE array (n_terms floats) so that a data-dependent
 * normaliser (continuity_only's count, a global N under data parallelism) never
 * needs a host round trip.  For mean-of-squares losses term_scale[t] = weight/N. */
int32_t pinn_residual_loss_grad(const pinn_desc* desc, const pinn_residual_spec* spec,
                                const float* term_scale,
                                const float* params, const float* X, int64_t N,
                                float* term_sums, float* grad_flat,
                                void* ws, int64_t ws_bytes, void* stream);

/* fidelity: col_sums[j] = sum_n (T[n,j] - Y[n,out_col[j]])^2 ;
 * grad_flat += sum_j col_scale[j] * d col_sums[j] / d theta   (train.py:136-141).
 * T is (N, n_cols) row-major; out_col is a HOST array; col_scale/col_sums are device. */
int32_t pinn_mse_loss_grad(const pinn_desc* desc, const float* params, const float* X,
                           const float* T, int64_t N, int32_t n_cols, const int32_t* out_col,
                           const float* col_scale, float* col_sums, float* grad_flat,
                           void* ws, int64_t ws_bytes, void* stream);

/* residual + fidelity on ONE point set in one pass (train_newmethod.py:122-159: a single forward
 * feeds both F.mse_loss on the `trues` columns and the residual):
 * grad_flat += sum_t term_scale[t] d term_sums[t]/d theta + sum_j col_scale[j] d col_sums[j]/d theta */
int32_t pinn_residual_mse_loss_grad(const pinn_desc* desc, const pinn_residual_spec* spec,
                                    const float* term_scale, const float* T, int32_t n_cols,
                                    const int32_t* out_col, const float* col_scale,
                                    const float* params, const float* X, int64_t N,
                                    float* term_sums, float* col_sums, float* grad_flat,
                                    void* ws, int64_t ws_bytes, void* stream);

/* train.py:131-157 in ONE launch: the reference's loss_func runs the network twice per iteration, on
 * the fidelity points (train.py:132-141) and on the collocation points (train.py:148-154).  Here X
 * holds the n_res collocation points FIRST and the N - n_res fidelity points after them; T holds
 * the fidelity targets only, (N - n_res, n_cols).  The residual terms are summed over the first
 * n_res points, the squared errors over the rest (fidelity points ride through the jet kernels
 * with unused tangents: meant for N_fid << N_res or small N, where launches dominate). */
int32_t pinn_residual_mse_split_loss_grad(const pinn_desc* desc, const pinn_residual_spec* spec,
                                          const float* term_scale, const float* T, int32_t n_cols,
                                          const int32_t* out_col, const float* col_scale,
                                          const float* params, const float* X, int64_t N, int64_t n_res,
                                          float* term_sums, float* col_sums, float* grad_flat,
                                          void* ws, int64_t ws_bytes, void* stream);

/* train.py:189-193 as TWO launches (fused engine, one-pass requests): loss_func's forward + residual + backward, then
 * ONE kernel that finishes the loss sums and the gradient, applies torch.optim.Adam's update (pinn_adam_step's
 * arithmetic, bit for bit) to params / m / v and refreshes the packed weights in `ws` that the next call's first
 * kernel reads.  At the reference's own problem sizes (N_res = 243, config_CMB.json:43) the iteration is bound by
 * its launches: pack + pass + two reductions + zero-fill + update were six of them.
 *   X, n_res: as pinn_residual_mse_split_loss_grad (n_res == N: residual term only, n_cols may be 0;
 *             n_res < 0: both terms on every point, train_newmethod.py:122-159).
 *   grad_flat is OVERWRITTEN with this iteration's gradient (no zero-fill needed).
 *   adam->loss_rows / losses: optional — the finishing kernel also forms the weighted loss values the loop logs
 *             (double accumulation over the few sums), saving the caller a launch per iteration.
 *   adam->packed_valid: nonzero iff the previous call on this `ws` was this function with the same desc and
 *             nothing has written params since — the call then skips the packing kernel.
 * Returns PINN_ERR_UNSUPPORTED, having launched nothing, when the request would not run as one pass of the fused
 * engine (wide / generic engines, large split requests): use the loss call followed by pinn_adam_step. */
typedef struct pinn_adam_state {
  float* m;              /* exp_avg    (P) */
  float* v;              /* exp_avg_sq (P) */
  int64_t step;          /* 1-based, as torch counts */
  double lr, beta1, beta2, eps;
  int32_t packed_valid;
  int32_t n_loss_rows;   /* 0, or: also write losses[r] = sum_j loss_rows[r][j] * S_j, S = [col_sums (n_cols) | term_sums] */
  const float* loss_rows;/* (n_loss_rows, n_cols + n_terms) row-major weights (train.py:141,154,157: fidelity / residual / total) */
  float* losses;         /* (n_loss_rows) */
} pinn_adam_state;
int32_t pinn_loss_grad_adam_step(const pinn_desc* desc, const pinn_residual_spec* spec,
                                 const float* term_scale, const float* T, int32_t n_cols,
                                 const int32_t* out_col, const float* col_scale,
                                 float* params, const float* X, int64_t N, int64_t n_res,
                                 float* term_sums, float* col_sums, float* grad_flat,
                                 const pinn_adam_state* adam, void* ws, int64_t ws_bytes, void* stream);

/* n_iters consecutive Adam iterations of pinn_loss_grad_adam_step on the same point set (train.py:188-193, the
 * `for epoch in range(adam_maxit)` loop without the host in it: 2 n_iters launches enqueued by one call; at the
 * reference's problem sizes the Python-side cost of an iteration had become as large as its kernels).  Iteration i uses
 * step adam->step + i and learning rate lr[i] (HOST array: the StepLR schedule, train.py:109-113); when
 * adam->n_loss_rows > 0 it writes its weighted losses to adam->losses + i * n_loss_rows.  adam->lr is ignored.
 * Same refusal rule as pinn_loss_grad_adam_step (nothing is launched when unsupported). */
int32_t pinn_adam_loop(const pinn_desc* desc, const pinn_residual_spec* spec,
                       const float* term_scale, const float* T, int32_t n_cols,
                       const int32_t* out_col, const float* col_scale,
                       float* params, const float* X, int64_t N, int64_t n_res,
                       float* term_sums, float* col_sums, float* grad_flat,
                       const pinn_adam_state* adam, int32_t n_iters, const double* lr,
                       void* ws, int64_t ws_bytes, void* stream);

/* ---- device-enqueued Adam runs with closure coefficients or point weights -------------------------------------------------
 * (added under ABI version 4, as the entries above were: no existing entry, struct or constant changed)
 * pinn_adam_loop for the two requests it does not carry: the residual with runtime coefficients (pinn_residual_coef_loss_grad)
 * and the residual with point weights (pinn_residual_weighted_loss_grad), fixed or self-adaptive.  One call enqueues n_iters
 * iterations; iteration i uses step adam->step + i and the HOST arrays lr[i] (network), lr_coef[i] (coefficients), lr_w[i]
 * (multipliers) and is, in stream order:
 *   1. the residual pass: the tile kernel's coefficient / weighted gradient instance on (X, N_res), on the very grid the
 *      single entry uses — term_sums, coef_grad and fields keep that entry's bit-reproducibility;
 *   2. the fidelity pass: pinn_mse_loss_grad's pass on its own point set (Xf, T, N_fid), on the kernel that entry would take
 *      (at hidden width 33..64 under AUTO / FUSED the cooperative kernel while the points are at most one 16-point tile per
 *      compute unit, else the tile kernel); skipped when N_fid == 0 (col_sums, if given, is then zeroed).  Xf may alias X;
 *   3. ONE finishing kernel:
 *        parameter blocks   gradient of parameter p = (fidelity pass's) + (residual pass's), each summed over that pass's own
 *                           gradient copies in pinn_loss_grad_adam_step's order; grad_flat[p] OVERWRITTEN with it; Adam on
 *                           params / m / v (pinn_adam_step's arithmetic, bit for bit); packed weights refreshed
 *        one sums block     term_sums from the residual pass, col_sums from the fidelity pass, the optional weighted losses
 *                           (adam->loss_rows, row stride n_cols + n_terms, written to adam->losses + i * n_loss_rows);
 *                           coefficients: coef_log row i <- coef (the values iteration i RAN WITH), coef_grad[c] <- the
 *                           pass's coefficient gradient (what pinn_residual_coef_loss_grad adds to a zeroed array) times
 *                           coef_mask[c] if a mask is given, then Adam with lr_coef[i] on coef / coef_m / coef_v in place
 *        multiplier blocks  self-adaptive weights only, one thread per element (t, n) of lam: from the pass's unweighted
 *                           signed fields, sf = (term_scale[t] f) f (w_rows == 1: summed over the weighted terms in term
 *                           order), g = -((2 lam) sf) for sa_mask 0 (w = lam^2) or g = -sf for sa_mask 1 (w = lam), no fused
 *                           multiply-add; Adam with lr_w[i] DESCENDS along g (lam ascends the loss) on lam / lam_m / lam_v;
 *                           point_w <- lam_new^2 or lam_new for the next pass
 * Three launches per iteration, two without fidelity points; a zero-fill per pass where the gradient copies do not fit in
 * LDS; one packing kernel per call unless adam->packed_valid (the caller's promise, as in pinn_loss_grad_adam_step); with
 * lam, one kernel per call that forms point_w from lam before the first pass.  adam->lr is ignored.
 * pinn_adam_extras: exactly one of the two groups.
 *   coefficients  coef (n_coef, required), coef_grad (NULL: every coefficient frozen — values only, coef is not written and
 *                 coef_m, coef_v, coef_mask, lr_coef are not read; otherwise coef_m, coef_v and lr_coef are required),
 *                 coef_mask (NULL: all trainable; else n_coef floats 0 / 1: a 0 entry sees gradient 0 and does not move
 *                 while its moments are zero), coef_log (NULL or (n_iters, n_coef))
 *   weights       point_w (w_rows, N_res), w_rows 1 or n_w as in pinn_residual_weighted_loss_grad.  lam == NULL: fixed
 *                 weights, point_w is read only; fields may be given and is overwritten every iteration.  lam given:
 *                 lam, lam_m, lam_v (w_rows, N_res), fields (n_fields, N_res) and lr_w are required, sa_mask is 0 or 1.
 * Rules, all decided before any device work (nothing is launched on a refusal); the query follows the same rules:
 *   both groups (coef and point_w)              PINN_ERR_UNSUPPORTED  ("no kernel carries both")
 *   neither group, or extras NULL               PINN_ERR_INVALID      (use pinn_adam_loop)
 *   the residual request                        served where pinn_residual_coef_loss_grad / pinn_residual_weighted_loss_grad
 *                                               run the tile kernel: AUTO, FUSED, FUSED_TILE; fp32, tanh, width <= 64, d_in
 *                                               and d_out <= 16, dropout_p == 0, k = the residual's directions
 *   GENERIC, WIDE, FUSED_COOP, FUSED_BATCH, bf16, LeakyReLU, width > 64, dropout, k mismatch
 *                                               PINN_ERR_UNSUPPORTED with the reason (AUTO is NOT moved to the generic engine
 *                                               here: use the single entries and pinn_adam_step)
 *   spec.flags bit 0 (corrected stress)         PINN_ERR_UNSUPPORTED, "corrected" in the message
 *   the continuity residuals with coef          PINN_ERR_UNSUPPORTED, "no coefficient" in the message
 *   w_rows other than 1 or n_w, sa_mask other than 0 or 1, N_res < 1, N_fid < 0, NULL pointers   PINN_ERR_INVALID
 *   n_iters == 0                                PINN_OK, nothing launched
 * n_cols: the fidelity columns, 0..PINN_MAX_ROLES, the row length of col_sums and the column offset of the term sums in
 * adam->loss_rows also when N_fid == 0.  N_fid > 0 needs n_cols >= 1, Xf, T (N_fid, n_cols), out_col, col_scale, col_sums.
 * The workspace is the entry's own (pinn_query_adam_ext_workspace: packed weights, one scratch area, and a region of partial
 * sums and of gradient copies for EACH pass); it grows with N_res and N_fid and is never smaller than the single entries'. */
typedef struct pinn_adam_extras {
  /* exactly one of the two groups */
  float* coef; float* coef_m; float* coef_v; float* coef_grad;   /* (n_coef); coef_grad NULL: all frozen, values only   */
  const float* coef_mask;                                        /* NULL: all trainable, else (n_coef) 0/1              */
  float* coef_log;                                               /* NULL or (n_iters, n_coef)                           */
  float* point_w; int32_t w_rows;                                /* (w_rows, N_res): fixed weights, read only ...       */
  float* fields;                                                 /* NULL or (n_fields, N_res); required with lam        */
  float* lam; float* lam_m; float* lam_v; int32_t sa_mask;       /* ... or self-adaptive: point_w is then written (0 lam^2, 1 lam) */
} pinn_adam_extras;
int32_t pinn_query_adam_ext_workspace(const pinn_desc* desc, const pinn_residual_spec* spec, const pinn_adam_extras* extras,
                                      int64_t N_res, int64_t N_fid, int64_t* bytes);
int32_t pinn_adam_loop_ext(const pinn_desc* desc, const pinn_residual_spec* spec, const float* term_scale,
                           const float* Xf, const float* T, int64_t N_fid, int32_t n_cols, const int32_t* out_col,
                           const float* col_scale, float* params, const float* X, int64_t N_res,
                           float* term_sums, float* col_sums, float* grad_flat, const pinn_adam_state* adam,
                           const pinn_adam_extras* extras, int32_t n_iters, const double* lr, const double* lr_coef,
                           const double* lr_w, void* ws, int64_t ws_bytes, void* stream);

/* ---- gradient-statistics loss balancing -----------------------------------------------------------------------------------
 * (added under ABI version 4, as the entries above were: no existing entry, struct or constant changed)
 * The weights of a weighted sum of loss groups, set from the groups' own gradients (Wang, Teng & Perdikaris 2021, "learning-
 * rate annealing": MAX_MEAN; Wang et al. 2023, gradient-norm balancing: NORM).  Group j = 0 .. G-1 has a flat fp32 gradient
 * g_j of P entries, a weight lam[j] and three statistics, as doubles: A = max|g_j|, S = sum|g_j|, Q = sum g_j^2.
 *   MAX_MEAN   lam_hat[j] = A[ref] / (S[j] / P) for j != ref; lam[ref] is left alone
 *   NORM       lam_hat[j] = (sum_i sqrt(Q[i])) / sqrt(Q[j]) for every j, the sum in group order; ref is ignored
 *   then       lam[j] <- (float)((1 - alpha) * (double)lam[j] + alpha * lam_hat[j]): formed in double, no fused multiply-add,
 *              rounded to fp32 once
 * A group whose lam_hat is not a finite positive number keeps its lam bit for bit: a zero denominator, A[ref] = 0, a NaN or
 * infinite statistic (under NORM a NaN or infinite Q makes the SUM non-finite, so every group keeps its weight).
 * pinn_balance_weights_host: the rule alone, on HOST arrays, no device touched — the very function the kernels call.
 * NONE copies lam_in to lam_out.  PINN_ERR_INVALID: alpha outside (0, 1], G outside 1..PINN_BALANCE_MAX_GROUPS, ref outside
 * 0..G-1, P < 1, an unknown mode, NULL pointers (stats may be NULL under NONE). */
#define PINN_BALANCE_NONE      0   /* combine only */
#define PINN_BALANCE_MAX_MEAN  1
#define PINN_BALANCE_NORM      2
#define PINN_BALANCE_MAX_GROUPS 8
#define PINN_BALANCE_STATS 3       /* per group: A = max|g|, S = sum|g|, Q = sum g^2, as doubles */
int32_t pinn_balance_weights_host(int32_t mode, int32_t G, int32_t ref, double alpha, int64_t P,
                                  const double* stats /* (G,3) */, const float* lam_in, float* lam_out);
/* The same on the device, for G flat gradients (row j of grads, row stride ld >= P), independent of engine and descriptor —
 * the loss calls of any engine can fill the rows.  In stream order, at most three small launches:
 *   statistics   one pass over (G, P): per-block partials of A, S, Q in double (g^2 is exact there), then one block folds them
 *                in an order fixed by (P, G) alone: bit-reproducible.  A NaN entry makes all three statistics of its group NaN
 *                (the max keeps it, unlike fmaxf).  stats, if given, is OVERWRITTEN at (G, 3).
 *   update       the rule above on lam, in place
 *   combination  with grad_out: grad_out[i] = ((lam[0] g_0[i]) + (lam[1] g_1[i])) + ..., group order, the NEW weights, no
 *                fused multiply-add; OVERWRITTEN at (P).  grad_out may alias none of the inputs.
 * Mode NONE skips statistics and update and only combines: lam is read only, stats, if given, is left alone.
 * Refusals, before any device work: the arguments pinn_balance_weights_host refuses; ld < P, NULL grads or lam:
 * PINN_ERR_INVALID; a workspace below pinn_query_balance_workspace's answer: PINN_ERR_WORKSPACE (the workspace may hold
 * anything on entry). */
int32_t pinn_query_balance_workspace(int64_t P, int32_t G, int64_t* bytes);
int32_t pinn_balance_update(int32_t mode, int32_t G, int32_t ref, double alpha,
                            const float* grads /* (G, ld) device, row j = g_j */, int64_t P, int64_t ld,
                            float* lam        /* (G) device, in/out */,
                            double* stats     /* NULL or (G,3) device, overwritten */,
                            float* grad_out   /* NULL or (P) device, overwritten */,
                            void* ws, int64_t ws_bytes, void* stream);

/* Device-enqueued Adam runs with two balanced groups: the PDE residual on the collocation points (group 0) and the fidelity
 * MSE on its own points (group 1).  pinn_adam_loop_ext's arguments with `balance` in place of `extras` and lr only.  One call
 * enqueues n_iters iterations; iteration i uses step adam->step + i and the HOST array lr[i] and is, in stream order:
 *   1. the plain residual pass on (X, N_res), weighted by the caller's term_scale;
 *   2. the fidelity pass (no input derivatives) on (Xf, T, N_fid), weighted by the caller's col_scale; Xf may alias X;
 *   3. on update iterations only — (adam->step + i - 1) % every == 0 — two launches: the statistics of the two per-group
 *      gradients, each summed over its pass's gradient copies in pinn_loss_grad_adam_step's order, and the rule on balance->lam;
 *   4. ONE finishing kernel: g = (lam[0] g_res) + (lam[1] g_fid), no fused multiply-add, on the same sums of the copies;
 *      grad_flat OVERWRITTEN with g; Adam on params / m / v (pinn_adam_step's arithmetic, bit for bit); packed weights
 *      refreshed; term_sums, col_sums and the optional weighted losses as in pinn_adam_loop_ext.
 * Three launches on ordinary iterations, five on update iterations; a zero-fill per pass where the gradient copies do not fit
 * in LDS; one packing kernel per call unless adam->packed_valid.  adam->lr is ignored.
 * term_sums, col_sums and adam->losses are weighted by the caller's scales and loss_rows, NOT by lam: lam_log gives the caller
 * what it needs to form the balanced total.
 * One packed copy of the weights serves both passes and the finishing kernel, so both passes run in natural unit order: the
 * residual pass takes the cooperative kernel where pinn_residual_loss_grad would, else the tile kernel's natural-order
 * instance — never the batch kernel and never the width-64 instances with permuted inputs / outputs, which the single entry
 * may choose.  Its term_sums therefore equal the single entry's bit for bit only where that entry takes the same kernel.
 * Rules, all decided before any device work (nothing is launched on a refusal); the query follows the same rules:
 *   fp32, tanh, width <= 64, d_in and d_out <= 16, dropout_p == 0, k = the residual's directions; engine AUTO, FUSED,
 *   FUSED_TILE, FUSED_COOP (padded width 64 only, as in the single entries)     served
 *   FUSED_BATCH, GENERIC, WIDE, bf16, LeakyReLU, the sine first layer, width > 64, dropout, k mismatch
 *                                               PINN_ERR_UNSUPPORTED with the reason (AUTO is NOT moved to another engine:
 *                                               use the loss calls, pinn_balance_update and pinn_adam_step)
 *   spec.flags bit 0 (corrected stress)         PINN_ERR_UNSUPPORTED, "corrected" in the message
 *   N_res < 1, N_fid < 1, every < 1, mode other than MAX_MEAN / NORM, ref other than 0 / 1, alpha outside (0, 1],
 *   NULL balance or lam, NULL pointers          PINN_ERR_INVALID
 *   n_iters == 0                                PINN_OK, nothing launched
 * The workspace is the entry's own (pinn_query_adam_balanced_workspace): pinn_adam_loop_ext's layout and the statistics'
 * partials; never smaller than pinn_query_adam_ext_workspace's answer for the same (N_res, N_fid). */
typedef struct pinn_balance {
  int32_t mode;        /* MAX_MEAN or NORM */
  int32_t every;       /* >= 1: iteration i updates iff (adam->step + i - 1) % every == 0 */
  int32_t ref;         /* 0 = residual group, 1 = fidelity group */
  double  alpha;
  float*  lam;         /* (2) device in/out: [residual, fidelity] */
  float*  lam_log;     /* NULL or (n_iters, 2): the weights iteration i STEPPED with (after its update, if any) */
  double* stats_log;   /* NULL or (n_iters, 2, 3): rows of update iterations overwritten, others untouched */
  float*  group_grads; /* NULL or (2, P): iteration i's g_res, g_fid as summed from the copies, overwritten */
} pinn_balance;
int32_t pinn_query_adam_balanced_workspace(const pinn_desc* desc, const pinn_residual_spec* spec, int64_t N_res, int64_t N_fid,
                                           int64_t* bytes);
int32_t pinn_adam_loop_balanced(const pinn_desc* desc, const pinn_residual_spec* spec, const float* term_scale,
                                const float* Xf, const float* T, int64_t N_fid, int32_t n_cols, const int32_t* out_col,
                                const float* col_scale, float* params, const float* X, int64_t N_res,
                                float* term_sums, float* col_sums, float* grad_flat, const pinn_adam_state* adam,
                                const pinn_balance* balance, int32_t n_iters, const double* lr,
                                void* ws, int64_t ws_bytes, void* stream);

/* ---- ensembles: M networks of one shape in one launch --------------------------------------------------------------
 * (added under ABI version 4, as the fields entries were: no existing entry, struct or constant changed)
 * A deep ensemble or a seed sweep trains M networks of the same descriptor on a problem that fills a few workgroups of the
 * chip.  These entries run all M members through ONE launch of the fused tile kernel's ensemble instances (a 2-D grid:
 * gx workgroups per member x M members) and one finishing launch, whatever M is.  Member m gets the arithmetic of the
 * single-network entry on params[m]; what differs is the number of workgroups per member (gx, below) and with it the order
 * of the partial sums.
 * Layout: params, grad_flat (and the Adam moments m, v) are (M, P) row-major; term_sums (M, n_terms), col_sums (M, n_cols),
 * adam->losses (M, n_loss_rows) — in pinn_ensemble_adam_loop (n_iters, M, n_loss_rows).  term_scale, col_scale, out_col,
 * spec and adam->loss_rows are shared by all members.
 * flags: PINN_ENSEMBLE_OWN_X — X is (M, N, d_in), member m reads its own point set; PINN_ENSEMBLE_OWN_T — T is per member,
 * (M, rows, n_cols) with rows = N - n_res (split), N (n_res < 0).  Otherwise X (N, d_in) and T are shared.
 * n_res: as pinn_loss_grad_adam_step — n_res == N residual term only (T may be NULL, n_cols may be 0; col_sums, if given,
 * is zeroed), 0 <= n_res < N the split request, n_res < 0 both terms on every point.
 * Served: engine AUTO, FUSED or FUSED_TILE (always the tile kernel, at every N), fp32, tanh, width <= 64, d_in and
 * d_out <= 16, dropout_p == 0, k = 2 or 3.  Refused with PINN_ERR_UNSUPPORTED and the reason in pinn_last_error(), decided
 * before any device work (nothing is launched): engine GENERIC, WIDE, FUSED_COOP, FUSED_BATCH; bf16; width > 64;
 * LeakyReLU; dropout_p > 0; the corrected radiation stress ("corrected" in the message); k other than 2 or 3; the split
 * request at padded width 64 (hidden width 33..64: the tile kernel carries no split code there).
 * M < 1 or M > 65535: PINN_ERR_INVALID.  M = 1 is valid.  N >= 1.
 * Grid: gx = the single-network tile-kernel grid for N points, clamped to max(1, cap / M) with cap the tile kernel's own
 * workgroup cap for the shape (CUs x workgroups per CU); beyond M = cap, gx = 1 and the M workgroups queue.
 * The workspace is the entries' own: pinn_ensemble_query_workspace (it grows with M). */
#define PINN_ENSEMBLE_OWN_X 1
#define PINN_ENSEMBLE_OWN_T 2
#define PINN_ENSEMBLE_MAX_MEMBERS 65535
int32_t pinn_ensemble_query_workspace(const pinn_desc* desc, int32_t M, int64_t N, int64_t* bytes);
/* *gx = workgroups per member, *copy_in_lds = 1 if a workgroup's gradient copy lives in LDS, 0 if in the workspace.
 * Refused as the calls are, as far as the descriptor alone decides.  Host logic only: no device is needed (without one
 * the answer is that of a 256-CU device). */
int32_t pinn_ensemble_plan(const pinn_desc* desc, int32_t M, int64_t N, int32_t* gx, int32_t* copy_in_lds);
/* Member m: term_sums[m] / col_sums[m] <- the sums of pinn_residual_loss_grad / pinn_residual_mse_split_loss_grad /
 * pinn_residual_mse_loss_grad (by n_res) at params[m]; grad_flat[m] += the weighted gradient.  Three launches (pack, pass,
 * finish) and a zero-fill where the gradient copies live in the workspace. */
int32_t pinn_ensemble_loss_grad(const pinn_desc* desc, const pinn_residual_spec* spec, int32_t M,
                                const float* term_scale, const float* T, int32_t n_cols,
                                const int32_t* out_col, const float* col_scale,
                                const float* params, const float* X, int64_t N, int64_t n_res, int32_t flags,
                                float* term_sums, float* col_sums, float* grad_flat,
                                void* ws, int64_t ws_bytes, void* stream);
/* pinn_loss_grad_adam_step for M members: two launches per iteration, whatever M is.  pinn_adam_state is reused with
 * m, v of (M, P) and losses of (M, n_loss_rows); one step count, learning rate and set of betas for all members.
 * grad_flat (M, P) is OVERWRITTEN.  adam->packed_valid: as in pinn_loss_grad_adam_step, for the M packed copies (the
 * previous call on this `ws` was this function with the same desc, M and request, and nothing has written params since). */
int32_t pinn_ensemble_adam_step(const pinn_desc* desc, const pinn_residual_spec* spec, int32_t M,
                                const float* term_scale, const float* T, int32_t n_cols,
                                const int32_t* out_col, const float* col_scale,
                                float* params, const float* X, int64_t N, int64_t n_res, int32_t flags,
                                float* term_sums, float* col_sums, float* grad_flat,
                                const pinn_adam_state* adam, void* ws, int64_t ws_bytes, void* stream);
/* pinn_adam_loop for M members: n_iters iterations, 2 n_iters launches, enqueued by one call.  Iteration i uses step
 * adam->step + i and lr[i] (HOST array, shared by all members) and writes its weighted losses to
 * adam->losses + i * M * n_loss_rows. */
int32_t pinn_ensemble_adam_loop(const pinn_desc* desc, const pinn_residual_spec* spec, int32_t M,
                                const float* term_scale, const float* T, int32_t n_cols,
                                const int32_t* out_col, const float* col_scale,
                                float* params, const float* X, int64_t N, int64_t n_res, int32_t flags,
                                float* term_sums, float* col_sums, float* grad_flat,
                                const pinn_adam_state* adam, int32_t n_iters, const double* lr,
                                void* ws, int64_t ws_bytes, void* stream);

/* torch.optim.Adam single-tensor update on flat buffers (amsgrad off, weight_decay 0,
 * maximize off): m,v are exp_avg / exp_avg_sq; step is the 1-based step count;
 * lr is a host double (StepLR changes it between steps, train.py:193); the scalar
 * factors are formed in double as Python forms them and cast to fp32 once. */
int32_t pinn_adam_step(float* params, const float* grad, float* m, float* v, int64_t P,
                       int64_t step, double lr, double beta1, double beta2, double eps,
                       void* stream);

/* L-BFGS two-loop recursion of torch.optim.LBFGS (train.py:116-125, one .step(closure), train.py:200)
 * on device.  S, Y: (m x P) row-major rings of steps and gradient differences, M = S Y^T (m x m, fp64,
 * physical row indices); logical pair i (0 = oldest) is physical row (head + i) % m; k pairs in use.
 * pinn_lbfgs_push stores (s, y) in row `slot` and refreshes row and column `slot` of M.
 * pinn_lbfgs_direction writes d = -H_k g (H the initial scaling ys/yy); tmp: 4m doubles, coef: 2m
 * floats, q: P floats of scratch.  m <= 256.
 * What the caller must initialise:
 *  - S and Y must be zeroed once, before the first push.  Both calls read ALL m rows of S and Y, also the
 *    rows no pair has been stored in yet, and push writes row `slot` only.  Zero is the contract: finite
 *    rows would give the same direction today (an unused row's coefficient is exactly 0), but nothing
 *    tests or promises that.
 *  - tmp, coef and q may hold anything on entry: each is written before it is read.
 *  - Of M, pinn_lbfgs_direction reads only the rows and columns of the k pairs in use, and a push has
 *    written each of them.  (Push also writes the entries of row and column `slot` that belong to unused
 *    rows: they are s . 0 = 0.)
 * tests/test_lbfgs_gpu.py fills the scratch and the unused part of M with 1e30 and gets the same bits. */
int32_t pinn_lbfgs_push(float* S, float* Y, double* M, int32_t m, int64_t P, int32_t slot,
                        const float* s, const float* y, void* stream);
int32_t pinn_lbfgs_direction(const float* S, const float* Y, const double* M, int32_t m, int64_t P,
                             int32_t head, int32_t k, const float* g, double H, float* d,
                             double* tmp, float* coef, float* q, void* stream);

/* ---- device-resident L-BFGS: runs of strong-Wolfe evaluations enqueued by one call -----------------------------------
 * (added under ABI version 4, as the fields and residual2 entries were: no existing entry, struct or constant changed)
 * torch.optim.LBFGS.step(closure) with line_search_fn = "strong_wolfe" (train.py:116-125,200) without the host in it.
 * HIP has no device-side launch, so the host enqueues a fixed sequence of SLOTS and the device decides what each means:
 *     slot:  x_trial = x + t d                       (t, d on the device; x is `params`)
 *            loss + gradient pass at x_trial          (the very host code of the loss entries, params = x_trial: whatever
 *                                                      engine the descriptor selects)
 *            controller: one step of the strong-Wolfe state machine
 *              CONTINUE  next trial t, the gradient filed in its pool row; the accept kernels exit at once
 *              ACCEPT    x += t* d, s, y, the stopping tests, ring push (only when y.s > 1e-10), H = y.s / y.y,
 *                        d = -H_k g (the six-launch recursion of pinn_lbfgs_direction), gtd = g.d, t = lr, search re-armed
 *              STOP      the done flag with a reason; every later slot is inert
 * The first slot after pinn_lbfgs_loop_init is the evaluation at t = 0 (torch's orig_loss).  Every slot is a useful
 * evaluation: a line search of three evaluations takes three slots.
 *
 * The line search is torch's _strong_wolfe (torch/optim/lbfgs.py) restated branch for branch as a resumable state machine
 * (csrc/lbfgs_line_search.h: one source for host and device), c1 = 1e-4, c2 = 0.9, its own tolerance_change = 1e-9, and it
 * returns the LOW end of the bracket as torch does.  pinn_lbfgs_ls_init / pinn_lbfgs_ls_step run the very functions the
 * controller kernel calls, on the host; no device is touched.  The state carries no vectors, only rows of a four-row
 * gradient pool: row 0 holds the gradient of the iterate, g_slot_for_new says where the caller files the gradient of the
 * trial about to be evaluated, g_acc_slot which row holds the gradient of the accepted point.
 * Known deviation: lbfgs.FlatLBFGS hands _strong_wolfe a Python-float loss and fp32 0-dim tensors for g.d, so part of its
 * scalar arithmetic is fp32; here every scalar (g.d, y.s, y.y, |g|_1, the whole line search) is fp64, formed from
 * per-workgroup partial sums combined in a fixed order.  Same algorithm, same branches; a decision can flip at a rounding
 * boundary.  The loss value is the fp32 number float(loss) would have been (double accumulation, one rounding). */
#define PINN_LS_EVALUATE 0   /* evaluate f and g.d at st->t, file the gradient in row st->g_slot_for_new, call ls_step again */
#define PINN_LS_DONE 1       /* st->t_acc, st->f_acc, st->g_acc_slot */
#define PINN_LS_POOL_ROWS 4
typedef struct pinn_ls_state {
  double f0, gtd0, d_norm;           /* the point t = 0 and max|d| */
  double t;                          /* the trial step to evaluate (EVALUATE) */
  double t_prev, f_prev, gtd_prev;   /* bracketing phase: the previous point */
  double br_t[2], br_f[2], br_gtd[2];/* the bracket */
  double t_acc, f_acc;               /* DONE: the accepted step and its loss */
  int32_t phase;                     /* 0 bracketing, 1 zoom, 2 done */
  int32_t ls_iter, max_ls, n_evals;
  int32_t low_pos, high_pos, insuf_progress, br_n;
  int32_t g_prev_slot, br_slot[2];   /* pool rows of the previous point and of the bracket ends */
  int32_t g_slot_for_new, g_acc_slot;
} pinn_ls_state;
int32_t pinn_lbfgs_ls_init(pinn_ls_state* st, double f0, double gtd0, double t0, double d_norm, int32_t max_ls);
int32_t pinn_lbfgs_ls_step(pinn_ls_state* st, double f_new, double gtd_new);   /* PINN_LS_EVALUATE / PINN_LS_DONE, < 0: error */

typedef struct pinn_lbfgs_opts {
  double lr, tolerance_grad, tolerance_change;
  int32_t max_iter, max_eval, history_size;
} pinn_lbfgs_opts;

/* what a slot did (trace column 2) and why the loop stopped (trace column 6, ctrl.reason) */
#define PINN_LBFGS_ACT_INERT 0      /* the done flag was up: nothing evaluated, nothing written but this trace row */
#define PINN_LBFGS_ACT_CONTINUE 1   /* a trial inside a line search */
#define PINN_LBFGS_ACT_ACCEPT 2     /* the line search ended at this evaluation: iterate updated */
#define PINN_LBFGS_ACT_INITIAL 3    /* the evaluation at t = 0 */
#define PINN_LBFGS_STOP_NONE 0
#define PINN_LBFGS_STOP_GRADIENT 1  /* max|g| <= tolerance_grad */
#define PINN_LBFGS_STOP_STEP 2      /* max|s| <= tolerance_change */
#define PINN_LBFGS_STOP_LOSS 3      /* |f - f_prev| < tolerance_change */
#define PINN_LBFGS_STOP_MAX_ITER 4
#define PINN_LBFGS_STOP_MAX_EVAL 5
#define PINN_LBFGS_STOP_DIRECTION 6 /* g.d > -tolerance_change */

/* The control block: the first bytes of `state`.  The host may read it after its own synchronisation; it writes it only
 * through pinn_lbfgs_loop_init. */
typedef struct pinn_lbfgs_ctrl {
  int32_t phase;       /* 0: the next slot is the evaluation at t = 0; 1: inside a line search */
  int32_t done;        /* 1: stopped, every later slot is inert */
  int32_t reason;      /* PINN_LBFGS_STOP_* */
  int32_t action;      /* PINN_LBFGS_ACT_* of the slot in flight (the accept kernels read it) */
  int32_t head, k, slot, m;          /* the ring: oldest row, pairs in use, row of the last push, history_size */
  int32_t n_iter, n_evals, max_iter, max_eval;
  int32_t push;        /* this accept stores a pair */
  int32_t file_row, acc_row;         /* pool rows: of the gradient just evaluated, of the accepted point */
  int32_t n_slots;     /* slots run since init, inert ones included */
  int64_t P;
  double t;            /* the trial step of the next slot */
  double f, gtd, d_norm, H;          /* at the iterate: loss, g.d, max|d|, initial scaling */
  double f_prev;       /* prev_loss of torch */
  double t_acc, gmax;  /* of the last accept */
  double lr, tolerance_grad, tolerance_change;
  pinn_ls_state ls;
} pinn_lbfgs_ctrl;

/* trace: (n_slots, PINN_LBFGS_TRACE_COLS) doubles, overwritten.  Per slot: 0 evaluation index (1-based), 1 iteration index
 * (after the slot), 2 action, 3 the step t evaluated, 4 its loss f, 5 g_new.d, 6 stop reason (0: none), 7 accepted step t*,
 * 8 its loss, 9 max|g| at the accepted point (7..9: ACCEPT and INITIAL rows, else 0), 10 .. 10 + n_loss_rows the weighted
 * losses of this evaluation, zeros up to column 17.  Inert slots: zeros. */
#define PINN_LBFGS_TRACE_COLS 18

/* ws_bytes: the pass's workspace (pinn_query_workspace's answer); state_bytes: control block, d, x_trial, g_new, the
 * four-row gradient pool, prev_g, s, y, q (P floats each), S and Y (history_size x P floats each), M (history_size^2
 * doubles), the recursion's scratch and the reduction partials — every region on a 256-byte boundary. */
int32_t pinn_query_lbfgs_loop(const pinn_desc* desc, int64_t N, int32_t history_size, int64_t* ws_bytes, int64_t* state_bytes);
/* zeroes the state (S and Y with it) and arms the control block; P is the descriptor's parameter count */
int32_t pinn_lbfgs_loop_init(void* state, int64_t state_bytes, int64_t P, const pinn_lbfgs_opts* opts, void* stream);
/* n_slots slots.  X, n_res, T, n_cols, out_col, the scales and loss_rows as in pinn_loss_grad_adam_step (loss_rows:
 * (n_loss_rows, n_cols + n_terms), 1 <= n_loss_rows <= 8); total_row names the row that is the objective.
 * params is x: it holds the ACCEPTED iterate whenever a call returns; trial weights never reach it.  The state carries
 * over between calls: two calls of n slots are one call of 2n.  trace may be NULL.
 * Refused before any device work: history_size (of the query) outside 1..256, n_slots < 0, null pointers, a state smaller
 * than the query's -> PINN_ERR_INVALID / PINN_ERR_WORKSPACE; dropout_p > 0 -> PINN_ERR_UNSUPPORTED (a seed per forward pass
 * has no place in a fixed schedule); every refusal the loss request itself would get, with its own message.
 * Reproducible wherever the pass is: no float atomics, every reduction is per-workgroup partials combined in a fixed order. */
int32_t pinn_lbfgs_loop(const pinn_desc* desc, const pinn_residual_spec* spec, const float* term_scale, const float* T,
                        int32_t n_cols, const int32_t* out_col, const float* col_scale, float* params, const float* X,
                        int64_t N, int64_t n_res, int32_t n_loss_rows, const float* loss_rows, int32_t total_row,
                        void* state, int64_t state_bytes, int32_t n_slots, double* trace,
                        void* ws, int64_t ws_bytes, void* stream);

/* ---- the device-resident L-BFGS loop of an ensemble ---------------------------------------------------------------------
 * pinn_lbfgs_loop for the M networks of pinn_ensemble_loss_grad: every member runs its own strong-Wolfe search, its own
 * ring and its own stopping tests, and ONE schedule of launches per slot advances them all (kernels on a grid whose second
 * axis is the member, the pass is pinn_ensemble_loss_grad's).  Member j gets the arithmetic pinn_lbfgs_loop applies to
 * row j of params; where the ensemble pass gives the bits of the single-network pass (one working wave per member), the
 * whole loop does.  One pinn_lbfgs_opts for all members.  A member that has stopped is inert in every later slot: zero
 * trace rows, its row of params untouched, its control block unchanged but for `action`; its pass still runs.
 *
 * The state, every region on a 256-byte boundary, a(x) = x rounded up to a multiple of 256:
 *   M control blocks (pinn_lbfgs_ctrl) at a stride of a(sizeof(pinn_lbfgs_ctrl)) bytes: member j's at j * stride, so the
 *     host fetches all of them in one copy of M * stride bytes;
 *   d (M, P) floats at M * stride; x_trial (M, P) floats — the weights of the last evaluation — a(4 M P) bytes further;
 *   then g_new (M, P), the column sums and the term sums (M x PINN_MAX_ROLES floats reserved each), and M member blocks
 *   (gradient pool, prev_g, s, y, q, partials, losses, recursion scratch, S, Y, M).
 *   state_bytes = M a(sizeof(pinn_lbfgs_ctrl)) + 3 a(4 M P) + 2 a(4 M PINN_MAX_ROLES) + M member_bytes,
 *   member_bytes = a(4 PINN_LS_POOL_ROWS P) + 4 a(4 P) + a(8 * 256 * 8) + a(32) + a(8 * 4 * 256) + a(4 * 2 * 256)
 *                  + 2 a(4 history_size P) + a(8 history_size^2).
 *
 * pinn_ensemble_query_lbfgs_loop: ws_bytes is pinn_ensemble_query_workspace's answer, state_bytes the formula above.  Host
 *   logic only, like pinn_ensemble_plan.
 * pinn_ensemble_lbfgs_loop_init: zeroes the state and arms the M control blocks; P is the descriptor's parameter count.
 * pinn_ensemble_lbfgs_loop: n_slots slots.  params (M, P): row j holds member j's ACCEPTED iterate whenever a call returns.
 *   X, T, flags (PINN_ENSEMBLE_OWN_X / _OWN_T), n_res, n_cols, out_col and the scales as pinn_ensemble_loss_grad; loss_rows,
 *   total_row as pinn_lbfgs_loop, shared by the members; history_size the one the state was initialised with (it sizes the
 *   recursion kernels' grids: a member whose control block holds another is not advanced).  trace: (n_slots, M,
 *   PINN_LBFGS_TRACE_COLS) doubles, the rows of pinn_lbfgs_loop's trace, one per member, or NULL.  Two calls of n slots are
 *   one call of 2n.  Writes params, trace and state at those extents only; after the init `state` is the one buffer whose
 *   content a call relies on.
 * Refused before any device work, the reason in pinn_last_error(): everything pinn_ensemble_loss_grad refuses, in its own
 *   words; M outside 1..PINN_ENSEMBLE_MAX_MEMBERS; history_size outside 1..256; n_slots < 0; n_loss_rows / total_row as
 *   pinn_lbfgs_loop; null pointers; a state or workspace smaller than the query's answer (PINN_ERR_WORKSPACE). */
int32_t pinn_ensemble_query_lbfgs_loop(const pinn_desc* desc, int32_t M, int64_t N, int32_t history_size, int64_t* ws_bytes,
                                       int64_t* state_bytes);
int32_t pinn_ensemble_lbfgs_loop_init(void* state, int64_t state_bytes, int32_t M, int64_t P, const pinn_lbfgs_opts* opts,
                                      void* stream);
int32_t pinn_ensemble_lbfgs_loop(const pinn_desc* desc, const pinn_residual_spec* spec, int32_t M, const float* term_scale,
                                 const float* T, int32_t n_cols, const int32_t* out_col, const float* col_scale, float* params,
                                 const float* X, int64_t N, int64_t n_res, int32_t flags, int32_t n_loss_rows,
                                 const float* loss_rows, int32_t total_row, int32_t history_size, void* state,
                                 int64_t state_bytes, int32_t n_slots, double* trace, void* ws, int64_t ws_bytes, void* stream);

/* ---- staging of the collocation points on the device (train.py:246-277, operations.py:4-30) --------------------
 * The reference loads each input variable as a (ny, nx) float64 grid (scipy.io.loadmat), subsamples it with
 * [::interval_x, ::interval_y] (train.py:260), maps it onto [-1, 1] with the variable's (min, max) (operations.py:4-8;
 * a degenerate range gives zeros), flattens it COLUMN-major (train.py:265-267), stacks the variables as columns and
 * drops every row that holds a NaN (train.py:276-277).  These two calls do the same on grids already resident on the
 * device, in float64 and in NumPy's order of operations, casting to fp32 last (train.py:88): bit-identical to the
 * host path.  pinn_nanminmax_f64 is np.nanmin / np.nanmax (operations.py:26-27; {NaN, NaN} for an all-NaN array).
 * grids: HOST array of d_in DEVICE pointers (ny * nx doubles each, row-major); minmax: device (d_in, 2) doubles;
 * X_out: device, room for ceil(ny/ix) * ceil(nx/iy) rows of d_in floats; n_rows_out: device, rows actually written. */
int32_t pinn_nanminmax_f64(const double* data, int64_t n, double* out2, void* ws, int64_t ws_bytes, void* stream);
int64_t pinn_stage_workspace_bytes(int64_t ny, int64_t nx, int32_t interval_x, int32_t interval_y);
int32_t pinn_stage_grid_columns(const double* const* grids, int32_t d_in, int64_t ny, int64_t nx, int32_t interval_x,
                                int32_t interval_y, const double* minmax, float* X_out, int64_t* n_rows_out,
                                void* ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PINN_HIP_H */
