// fused_kernel.h — the MI355X fast path: one persistent kernel that, per tile of 16
// collocation points and per wave, runs
//     forward-mode jet through every layer  (dnn.py:54-55 + physics.py:6-15)
//  -> PDE residual + its adjoint             (physics.py:18-120, train.py:131-157)
//  -> reverse sweep: d loss / d theta        (train.py:191)
// entirely on v_mfma_f32_16x16x4_f32 (exact fp32, fmaf-chain numerics).
//
// Layout ("acc layout"): a 16(feature) x 16(point) tile lives in one f4 per lane;
// lane = (p = lane&15 point, q = lane>>4), register r  <->  feature 4q + r, point p.
// That is the C/D layout of the 16x16x4 MFMA, and — with the K index permuted so that
// k-step (tile kt, reg r) carries features {16kt + 4q + r : q = 0..3} — it is ALSO its B
// operand layout: a layer's accumulators feed the next layer's MFMAs with no data
// movement.  The matching A operand (weights) is then W[16MT + m][16kt + 4kq + r],
// r = 0..3 contiguous: one 16-byte load from the row-major (padded) weights.  The
// reverse sweep uses the same chain on W^T.  Only the weight-gradient GEMM
// (dW = Zbar . A^T, contraction over points) needs points on the K axis: each
// 16x16 block is transposed through a wave-private, XOR-swizzled 1 KB LDS pad.
//
// Activations needed by the reverse sweep are spilled to a per-wave global scratch
// slot in fragment-native order (fully coalesced 16 B/lane both ways; written once,
// read once).  dW/db are accumulated in a per-workgroup LDS copy of the (padded)
// gradient with plain vector read-modify-write under a per-layer wave-level lock
// (LDS fp32 atomics are ~150 cycles per wave-instruction on gfx950), written out once
// per workgroup and summed across workgroups by a second kernel in a fixed order.
#pragma once
#include <string.h>
#include <type_traits>
#include "common.h"
#include "residuals.h"

namespace pinn {

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int FUSED_WAVES = 4;
constexpr int FUSED_W16_WAVES = 3;   // waves per SIMD the width-16 kernels are compiled for (workgroups per CU follow in pinn_fused.hip)
constexpr int FUSED_FLUSH_ROWS = 4;  // row blocks of the gradient flush read per round trip
constexpr int FUSED_THREADS = FUSED_WAVES * 64;
constexpr int TB_FLOATS = 256;                // one 16x16 fp32 block, XOR-swizzled (see transpose_write)
constexpr int TB_PER_WAVE = 8;                // 4 pads for the Zbar tiles + 4 for the A tiles of one quantity
constexpr int MAX_SUMS = 12;               // residual terms at [0,4), fidelity columns at [4,12)
constexpr int MSE_SUM0 = 4;
// The ONE term -> slot rule of a row of partial sums: terms [0, MSE_SUM0) in their own slots; a residual with more terms (the
// wave closure's fifth) fills the row from its END, behind the fidelity columns, which then have one slot fewer
// (WAVE_MAX_COLS, common.h).  Used by the epilogue that adds into the row and by everything that reduces it (pinn_fused.hip:
// finish_sums2, the reduce_sums calls).  Every residual with at most MSE_SUM0 terms sees terms at [0, n_terms) as before.
__host__ __device__ constexpr int term_slot(int t) { return t < MSE_SUM0 ? t : MAX_SUMS - 1 - (t - MSE_SUM0); }
static_assert(term_slot(PINN_PEW_TERMS - 1) == MSE_SUM0 + WAVE_MAX_COLS, "the fifth term's slot is the eighth column's");

struct FusedParams {
  int d_in, d_out, L, act;
  int dir_col[PINN_MAX_DIRS];
  int64_t N, n_tiles;
  const float* X;
  const float* Wp;    // padded weights, row-major [out][in] per layer
  const float* WTp;   // padded transposed weights, row-major [in][out] per layer
  const float* Bp;    // padded biases
  float* scratch;     // activation spill, scratch_per_wave floats per wave
  int64_t scratch_per_wave;
  float* Y; float* dY;  // forward outputs (may be null).  k_fused<..., EPI_FIELD> stores no outputs: there Y is the residual
                        // fields' array, field-major (NF, N), and dY is null — a member of its own would change the kernel
                        // argument block of EVERY k_fused instance, and with it the register allocation of the
                        // register-starved width-64 forward kernels (measured: AGPRs 8 -> 4, spilled SGPRs 36 -> 39)
                        // k_fused<..., EPI_WEIGHTED>: Y is the optional array of the unweighted signed fields, (NF, N) as for
                        // EPI_FIELD, or null; dY is null
  int loss_kind;        // bit 0: PDE residual, bit 1: fidelity MSE (both: one pass, train_newmethod.py:122-159)
  int residual_id;
  int out_col[PINN_MAX_ROLES];   // residual: output column of each role
  int q_of[PINN_MAX_DIRS];   // engine quantity (1 + direction index) of each residual direction role
  float thr, anchor; int xcol;
  const float* scale;        // residual: device term scales (null when no gradient wanted)
  int n_cols;                // mse: number of target columns
  int mse_col[PINN_MAX_ROLES];   // mse: output column of each target column
  const float* T;            // mse: targets (N, n_cols); split mode: (N - n_split, n_cols)
  int64_t n_split;           // < 0: every loss term on every point; >= 0: residual on points < n_split, mse on the rest
                             // k_fused<..., EPI_WEIGHTED> (no split, no fidelity term): the row stride of the point weights
                             // instead, 0 (one row for every term) or N (a row per weighted term)
  const float* mse_scale;    // mse: device column scales
  float* wg_sums;            // [grid][MAX_SUMS]
  float* wg_grads;           // [grid][PP]: acc_lds: written once at kernel end; else the workgroups' live global copies
  int acc_lds;               // 1: the workgroup's gradient copy lives in LDS
  int PW, PB;                // padded weight / bias float counts
  int lds_acc_floats;        // floats reserved for the LDS gradient copy (0 if unused)
  int batch_T;               // k_fused_batch: tiles per wave and batch of the instance to launch; k_fused_ens: ENS_OWN_X / ENS_OWN_T
  int io1;                   // k_fused<..., IO1 = true>: inputs / outputs in k-step-major order (see k_fused)
  uint32_t drop_seed, drop_thresh;   // k_fused<..., DROP = true>: nn.Dropout in training mode (common.h: dropout_bits)
  float drop_scale, drop_keep;       // 1 / (1 - p), 1 - p
  const float* gY;                   // k_fused<..., EPI_ADJ>: the caller's output adjoints, gY (N, d_out) and gdY (K1 - 1, N, d_out)
                                     // k_fused<..., EPI_COEF>: the residual's coefficients instead (n_coef floats; gdY null) — a
                                     // member of their own would grow the argument block of every instance (see Y above)
                                     // k_fused<..., EPI_WEIGHTED>: the point weights instead, (w_rows, N) row-major (gdY null)
  const float* gdY;                  // in the engine's direction order (row c - 1 belongs to dir_col[c - 1]); either may be null
};

// host: the residual's roles (spec: normalised by check_spec, pinn_abi.hip) -> P
inline void set_residual_roles(FusedParams& P, const Net& n, const pinn_residual_spec& spec) {
  P.residual_id = spec.residual_id;
  for (int j = 0; j < PINN_MAX_ROLES; ++j) P.out_col[j] = spec.out_col[j];
  for (int d = 0; d < PINN_MAX_DIRS; ++d) P.q_of[d] = 1 + spec.dir_of[d];
  P.thr = spec.param[0]; P.anchor = spec.param[1];
  P.xcol = n.dir_col[spec.dir_of[0]];
}
// host: the loss part of P (memset to 0 before) for a loss request of the fused or the wide engine
inline void set_loss(FusedParams& P, const Net& n, const LossReq& rq) {
  P.n_split = rq.n_split;
  P.loss_kind = rq.kind == 0 ? 1 : (rq.kind == 1 ? 2 : 3);
  if (P.loss_kind & 1) { P.scale = rq.scale; set_residual_roles(P, n, rq.spec); }
  else for (int j = 0; j < PINN_MAX_ROLES; ++j) P.out_col[j] = -1;
  if (P.loss_kind & 2) {
    P.n_cols = rq.n_cols; P.T = rq.T; P.mse_scale = rq.mse_scale;
    for (int j = 0; j < PINN_MAX_ROLES; ++j) P.mse_col[j] = j < rq.n_cols ? rq.out_col[j] : -1;
  }
}

__device__ __forceinline__ f4 mfma4(float a, float b, f4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

template <int WP> __device__ __forceinline__ int w_off_p(int l) { return l == 0 ? 0 : WP * 16 + (l - 1) * WP * WP; }
template <int WP> __device__ __forceinline__ int b_off_p(int l) { return l * WP; }

// Weight fragments of one layer: w[MT][kt] = Wl[16MT + m][16kt + 4kq .. +3]  (Wl row-major, row
// stride 16*NT_IN).  Loaded one phase AHEAD of the GEMM that uses them (software prefetch: with
// one wave per SIMD nothing else hides the L2/MALL latency of these loads).
template <int NT_IN, int NT_OUT>
__device__ __forceinline__ void load_w(const float* __restrict__ Wl, f4 (&w)[NT_OUT][NT_IN], int m, int kq) {
  constexpr int LDW = 16 * NT_IN;
#pragma unroll
  for (int MT = 0; MT < NT_OUT; ++MT)
#pragma unroll
    for (int kt = 0; kt < NT_IN; ++kt)
      w[MT][kt] = *reinterpret_cast<const f4*>(Wl + (16 * MT + m) * LDW + 16 * kt + 4 * kq);
}

// acc[c][MT] += sum_k W[16MT + m][k] * bin[c][k]      (KR < 4: only the first KR k-steps of every k-tile carry data)
template <int NT_IN, int NT_OUT, int K1, int KR = 4>
__device__ __forceinline__ void gemm_chain(const f4 (&w)[NT_OUT][NT_IN], const f4 (&bin)[K1][NT_IN],
                                           f4 (&acc)[K1][NT_OUT]) {
#pragma unroll
  for (int MT = 0; MT < NT_OUT; ++MT)
#pragma unroll
    for (int kt = 0; kt < NT_IN; ++kt)
#pragma unroll
      for (int r = 0; r < KR; ++r)
#pragma unroll
        for (int c = 0; c < K1; ++c) acc[c][MT] = mfma4(w[MT][kt][r], bin[c][kt][r], acc[c][MT]);
}


// One 16-row block of a layer's A operand: w[kt] = Wl[16MT + m][16kt + 4kq .. +3]  (row stride 16*NT_IN)
template <int NT_IN>
__device__ __forceinline__ void load_wblk(const float* __restrict__ Wl, int MT, f4 (&w)[NT_IN], int m, int kq) {
#pragma unroll
  for (int kt = 0; kt < NT_IN; ++kt)
    w[kt] = *reinterpret_cast<const f4*>(Wl + (16 * MT + m) * (16 * NT_IN) + 16 * kt + 4 * kq);
}

// acc[c][MT] += W[16MT + m][:] . bin[c]  with the weights STREAMED one 16-row block ahead of the
// MFMAs that use them: two blocks (8 f4 at width 64) are live instead of two whole layers, and
// nothing but `wa` is carried from one GEMM to the next (no loop-carried register copies).  `wa`
// holds block 0 on entry; while the last block computes, block 0 of the NEXT phase's matrix
// (`Wnext`, same row stride) is fetched into `wa`: its latency hides behind this GEMM's tail and
// the vector work between the two GEMMs.
// PACING.  One wave per SIMD issues in order: while it issues a run of vector-memory instructions the matrix pipe idles, and
// an instruction costs two to three times in a run what it costs alone between MFMAs (tools/ubench_coexec.hip).
// A paced stream issues nothing in a run: a block's MFMAs are one flat index i, and the block's memory instructions go out one
// by one from SLOTS in front of MFMA 0, GAP, 2 GAP, ...  A block's slots carry, in this order,
//   the NT_IN loads of the next weight block (consumed a block later),
//   in block 0 the `head` operations (the forward layers' bias loads: consumed after the GEMM),
//   in block MID_BLOCK (1, or 0 for short GEMMs) the `mid` operations: HBM traffic that must not sit in FRONT of a weight
//     load in the in-order vmcnt queue.  A spill store / activation reload issued before the GEMM has to complete before the
//     first streamed block (requested after it, consumed 2048 cycles later) can be used; issued here, the next load behind
//     it is consumed two blocks (4096 cycles) later and its own consumer a GEMM later.
// `head` and `mid` are objects with a compile-time COUNT and op<J>(), which issues their J-th instruction.  Where a block has
// fewer slots than operations they are dealt evenly over the slots, several per slot.  A GAP that leaves the block ONE slot
// (PACE_OFF) gives the unpaced order: everything in one run at the block's head.  -enable-misched=0 alone does not keep the
// source order (instruction selection clusters neighbouring loads and lets the MFMAs, which hang on no chain, drift past
// them): every occupied slot is fenced with sched_barrier(0).
struct NoMid { __device__ __forceinline__ void operator()() const {} };   // (wide_kernel.h's default hook)

// compile-time loop: f(std::integral_constant<int, I>) for I = I0 .. N - 1 (the index must be a constant where it picks a
// register, a slot or an immediate)
template <int I, int N, class F>
__device__ __forceinline__ void const_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    const_for<I + 1, N>(f);
  }
}
struct NoOps {
  static constexpr int COUNT = 0;
  template <int J> __device__ __forceinline__ void op() const {}
};
// the K1 * NT blocks of a layer's activation jet to / from the wave's slot: block J = (c, MT) = (J / NT, J % NT), 1 KB each
template <int NT, int K1, bool ON = true>
struct SpillOps {
  static constexpr int COUNT = ON ? K1 * NT : 0;
  float* __restrict__ slot;
  const f4 (&v)[K1][NT];
  int lane;
  template <int J> __device__ __forceinline__ void op() const { *reinterpret_cast<f4*>(slot + J * 256 + lane * 4) = v[J / NT][J % NT]; }
};
template <int NT, int K1>
struct UnspillOps {
  static constexpr int COUNT = K1 * NT;
  const float* __restrict__ slot;
  f4 (&v)[K1][NT];
  int lane;
  template <int J> __device__ __forceinline__ void op() const { v[J / NT][J % NT] = *reinterpret_cast<const f4*>(slot + J * 256 + lane * 4); }
};
// The bias is added behind the GEMM rather than used as the accumulators' initial value: as an initial value its L2
// latency sat exposed in front of every layer's first MFMA, and every accumulator chain starts from the inline constant 0.
template <int NT>
struct BiasOps {
  static constexpr int COUNT = NT;
  const float* __restrict__ b;
  f4 (&bias)[NT];
  int q;
  template <int J> __device__ __forceinline__ void op() const { bias[J] = *reinterpret_cast<const f4*>(b + 16 * J + 4 * q); }
};
// MFMAs per slot: 2 (against 1 and 4: DESIGN 3.3).  PACE_OFF is what the REVERSE stream passes (paced, its 4 + 16 loads lost
// in every round of the same A/B) and the forward-only kernel of pinn_fused_plain.hip (not measured paced).
// Widths 16 and 32 run 2-3 waves per SIMD, which hide issue time already: paced, 2 -> 100x20 -> 3 on this kernel lost 2 % and
// 2 -> 10x10 -> 6 gained 0.1 %, so the tile kernel paces its forward stream and its weight gradient at width 64 only.
constexpr int PACE_GAP = 2, PACE_OFF = 1 << 20, PACE_MIN_WP = 64;
template <int NT_IN, int NT_OUT, int K1, class Mid = NoOps, class Head = NoOps, int GAP = PACE_GAP>
__device__ __forceinline__ void gemm_stream(const float* __restrict__ Wl, const float* __restrict__ Wnext,
                                            f4 (&wa)[NT_IN], const f4 (&bin)[K1][NT_IN], f4 (&acc)[K1][NT_OUT],
                                            int m, int kq, const Mid& mid = Mid(), const Head& head = Head()) {
  constexpr int MID_BLOCK = NT_OUT >= 3 ? 1 : 0;
  constexpr int NM = NT_IN * 4 * K1;                       // MFMAs of a block: i = (kt * 4 + r) * K1 + c
  constexpr int NSLOT = (NM + GAP - 1) / GAP;
  const_for<0, NT_OUT>([&](auto mt_) {
    constexpr int MT = decltype(mt_)::value;
    constexpr int NHEAD = MT == 0 ? Head::COUNT : 0, NMID = MT == MID_BLOCK ? Mid::COUNT : 0;
    constexpr int NOPS = NT_IN + NHEAD + NMID;
    f4 wb[NT_IN];
    const float* __restrict__ wsrc = (MT + 1 < NT_OUT ? Wl + (16 * (MT + 1) + m) * (16 * NT_IN) : Wnext + m * (16 * NT_IN)) + 4 * kq;
    const_for<0, NM>([&](auto i_) {
      constexpr int i = decltype(i_)::value;
      if constexpr (i % GAP == 0) {
        constexpr int S = i / GAP;                           // this slot's operations: [K_LO, K_HI)
        constexpr int K_LO = NOPS <= NSLOT ? (S < NOPS ? S : NOPS) : (S * NOPS + NSLOT - 1) / NSLOT;
        constexpr int K_HI = NOPS <= NSLOT ? (S + 1 < NOPS ? S + 1 : NOPS) : ((S + 1) * NOPS + NSLOT - 1) / NSLOT;
        if constexpr (K_HI > K_LO && i > 0) __builtin_amdgcn_sched_barrier(0);
        const_for<K_LO, K_HI>([&](auto k_) {
          constexpr int k = decltype(k_)::value;
          if constexpr (k < NT_IN) wb[k] = *reinterpret_cast<const f4*>(wsrc + 16 * k);
          else if constexpr (k < NT_IN + NHEAD) head.template op<k - NT_IN>();
          else mid.template op<k - NT_IN - NHEAD>();
        });
        if constexpr (K_HI > K_LO && NSLOT > 1) __builtin_amdgcn_sched_barrier(0);
      }
      constexpr int kt = i / (4 * K1), r = (i / K1) % 4, c = i % K1;
      acc[c][MT] = mfma4(wa[kt][r], bin[c][kt][r], acc[c][MT]);
    });
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int kt = 0; kt < NT_IN; ++kt) wa[kt] = wb[kt];
  });
}

template <int NT, int K1>
__device__ __forceinline__ void zero_tiles(f4 (&v)[K1][NT]) {
#pragma unroll
  for (int c = 0; c < K1; ++c)
#pragma unroll
    for (int MT = 0; MT < NT; ++MT) v[c][MT] = f4{0.f, 0.f, 0.f, 0.f};
}

template <int NT, int K1>
__device__ __forceinline__ void init_bias(const float* __restrict__ b, f4 (&acc)[K1][NT], int q) {
#pragma unroll
  for (int MT = 0; MT < NT; ++MT) {
    acc[0][MT] = *reinterpret_cast<const f4*>(b + 16 * MT + 4 * q);
#pragma unroll
    for (int c = 1; c < K1; ++c) acc[c][MT] = f4{0.f, 0.f, 0.f, 0.f};
  }
}

// activation and its first derivative (dnn.py:18-21): tanh ('xavier') or LeakyReLU(0.01) ('kaiming')
template <int ACT, int NT, int K1>
__device__ __forceinline__ void activate(f4 (&acc)[K1][NT]) {
#pragma unroll
  for (int MT = 0; MT < NT; ++MT)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float z = acc[0][MT][r];
      float a, s;
      if constexpr (ACT == PINN_ACT_TANH) { a = tanh_f32(z); s = fmaf(-a, a, 1.f); }
      else { a = z > 0.f ? z : 0.01f * z; s = z > 0.f ? 1.f : 0.01f; }
      acc[0][MT][r] = a;
#pragma unroll
      for (int c = 1; c < K1; ++c) acc[c][MT][r] *= s;
    }
}

// adjoint of activate(): G holds (abar', abardot'_j) on entry, (zbar, zbardot_j) on exit
template <int ACT, int NT, int K1>
__device__ __forceinline__ void activate_adjoint(f4 (&G)[K1][NT], const f4 (&A)[K1][NT]) {
#pragma unroll
  for (int MT = 0; MT < NT; ++MT)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float a = A[0][MT][r];
      if constexpr (ACT == PINN_ACT_TANH) {
        const float s = fmaf(-a, a, 1.f);
        float cross = 0.f;
#pragma unroll
        for (int c = 1; c < K1; ++c) {
          cross = fmaf(G[c][MT][r], A[c][MT][r], cross);
          G[c][MT][r] *= s;
        }
        G[0][MT][r] = fmaf(-2.f * a, cross, s * G[0][MT][r]);   // tanh'' = -2 a (1 - a^2)
      } else {
        const float s = a > 0.f ? 1.f : 0.01f;                   // piecewise linear: no second-derivative term
#pragma unroll
        for (int c = 0; c < K1; ++c) G[c][MT][r] *= s;
      }
    }
}


// nn.Dropout(p) after every hidden activation in training mode (dnn.py:36-38, train.py:186), fused: the keep mask is
// the counter-based hash of common.h (dropout_bits(seed, layer, unit, point)), re-derived lane-locally wherever it is
// needed — in the activation and again in its adjoint — so nothing is stored.  The point's part of the hash is formed
// once per tile (DropLane), the (layer, unit) part per register.
struct DropLane {
  uint32_t h0, hi, thresh;
  float scale, keep_p;
  __device__ __forceinline__ void init(uint32_t seed, uint32_t thr, float sc, float kp, int64_t point) {
    h0 = dropout_fmix(seed ^ ((uint32_t)point * 0x9E3779B1u));
    hi = (uint32_t)((uint64_t)point >> 32);
    thresh = thr; scale = sc; keep_p = kp;
  }
  __device__ __forceinline__ float mask(int layer, int unit) const {     // 1 / (1 - p) for a kept unit, 0 for a dropped one
    const uint32_t x = h0 ^ (((uint32_t)layer * 0x01000193u + (uint32_t)unit) * 0x9E3779B1u + hi);
    return dropout_fmix(x) >= thresh ? scale : 0.f;
  }
};

// out-of-place forms: read the accumulators, write the next GEMM's B operand / the layer adjoint
// The bias is added here rather than used as the accumulators' initial value: its load is issued
// before the GEMM and consumed after it (as an initial value its L2 latency sat exposed in front of
// every layer's first MFMA), and every accumulator chain starts from the inline constant 0.
template <int NT>
__device__ __forceinline__ void load_bias(const float* __restrict__ b, f4 (&bias)[NT], int q) {
#pragma unroll
  for (int MT = 0; MT < NT; ++MT) bias[MT] = *reinterpret_cast<const f4*>(b + 16 * MT + 4 * q);
}
template <int ACT, int NT, int K1, bool DROP = false>
__device__ __forceinline__ void activate_to(const f4 (&acc)[K1][NT], const f4 (&bias)[NT], f4 (&a)[K1][NT],
                                            const DropLane* dl = nullptr, int layer = 0, int q = 0) {
  if constexpr (ACT == PINN_ACT_TANH && !DROP) {
    // explicit packed fp32 on the register pairs (0, 1) and (2, 3) of every f4: bias add, tanh (tanh_f32x2), s = 1 - a^2 and
    // the tangent products — per element the operations of the scalar form below in the same order (bitwise the same result)
#pragma unroll
    for (int MT = 0; MT < NT; ++MT)
#pragma unroll
      for (int h = 0; h < 4; h += 2) {
        const f2 z = f2{acc[0][MT][h], acc[0][MT][h + 1]} + f2{bias[MT][h], bias[MT][h + 1]};
        const f2 av = tanh_f32x2(z);
        const f2 s = __builtin_elementwise_fma(-av, av, f2{1.f, 1.f});
        a[0][MT][h] = av[0]; a[0][MT][h + 1] = av[1];
#pragma unroll
        for (int c = 1; c < K1; ++c) {
          const f2 t = f2{acc[c][MT][h], acc[c][MT][h + 1]} * s;
          a[c][MT][h] = t[0]; a[c][MT][h + 1] = t[1];
        }
      }
    return;
  }
#pragma unroll
  for (int MT = 0; MT < NT; ++MT)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float z = acc[0][MT][r] + bias[MT][r];
      float av, s;
      if constexpr (ACT == PINN_ACT_TANH) { av = tanh_f32(z); s = fmaf(-av, av, 1.f); }
      else { av = z > 0.f ? z : 0.01f * z; s = z > 0.f ? 1.f : 0.01f; }
      if constexpr (DROP) {      // a <- m a / (1 - p): the same mask multiplies the value and its tangents
        const float m = dl->mask(layer, 16 * MT + 4 * q + r);
        av *= m; s *= m;
      }
      a[0][MT][r] = av;
#pragma unroll
      for (int c = 1; c < K1; ++c) a[c][MT][r] = acc[c][MT][r] * s;
    }
}
// DROP: the stored jet is the masked one (a_out = m t, adot_out = m t' zdot with m = mask / (1 - p)); then
// d a_out / dz = m t', d adot_out / dz = -2 t adot_out and d adot_out / dzdot = m t': the formulas below with
// a := t = a_out (1 - p) and s := m t' (pinn_generic.hip, k_bwd_layer).  A dropped unit has a_out = adot_out = 0, s = 0.
template <int ACT, int NT, int K1, bool DROP = false>
__device__ __forceinline__ void activate_adjoint_to(const f4 (&G)[K1][NT], const f4 (&A)[K1][NT], f4 (&Z)[K1][NT],
                                                    const DropLane* dl = nullptr, int layer = 0, int q = 0) {
#pragma unroll
  for (int MT = 0; MT < NT; ++MT)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float a = A[0][MT][r];
      if constexpr (DROP) a *= dl->keep_p;
      if constexpr (ACT == PINN_ACT_TANH) {
        float s = fmaf(-a, a, 1.f);
        if constexpr (DROP) s *= dl->mask(layer, 16 * MT + 4 * q + r);
        float cross = 0.f;
#pragma unroll
        for (int c = 1; c < K1; ++c) {
          cross = fmaf(G[c][MT][r], A[c][MT][r], cross);
          Z[c][MT][r] = G[c][MT][r] * s;
        }
        Z[0][MT][r] = fmaf(-2.f * a, cross, s * G[0][MT][r]);
      } else {
        const float s = a > 0.f ? 1.f : 0.01f;
#pragma unroll
        for (int c = 0; c < K1; ++c) Z[c][MT][r] = G[c][MT][r] * s;
      }
    }
}

// ---- the sine first layer (PINN_ACT_SIN_TANH): layer 0's activation and its adjoint; layers >= 1 take the tanh forms above ----
// forward: a = sin z, adot_j = cos z * zdot_j.  z_0 is NOT the MFMA chain's fp32 sum: at a Fourier layer's arguments its
// rounding is the largest error of the whole pass (residuals.h, sincos_f64arg), so the value is formed in double from the
// unit's row of the padded W_0 (row stride 16) and the point's row of X (d_in terms, vector ALU; the MFMAs carry the
// tangents, which are columns of W_0 and exact).  q: the lane group, so register r of tile MT is unit 16 MT + 4 q + r.
template <int NT, int K1>
__device__ __forceinline__ void activate_sin_to(const f4 (&acc)[K1][NT], const f4 (&bias)[NT], f4 (&a)[K1][NT],
                                                const float* __restrict__ W0, const float* __restrict__ xrow, int d_in, int q) {
#pragma unroll
  for (int MT = 0; MT < NT; ++MT)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float sn, cs;
      sincos_f64arg(sin_layer_z(W0 + (16 * MT + 4 * q + r) * 16, bias[MT][r], xrow, d_in), sn, cs);
      a[0][MT][r] = sn;
#pragma unroll
      for (int c = 1; c < K1; ++c) a[c][MT][r] = acc[c][MT][r] * cs;
    }
}
// reverse: zbardot_j = cos z * abardot_j ;  zbar = cos z * abar - sin z * sum_j abardot_j * zdot_j.
// cos z cannot be rebuilt from the stored a_1 = sin z and is not spilled either (a slot per wave more would change ws_layout):
// z_0 = W_0 x + b_0 is formed AGAIN, at the end of the reverse sweep where only the adjoint G and the output Z are live — W_0
// and b_0 reloaded, the forward's own double sum (activate_sin_to: z_0 bit for bit).  The tangents zdot_j are the columns
// dir_col[j] of W_0; they come out of W_0 as the A operand against the unit tangent, one quantity at a time, so that a single
// temporary tile row is live beside cos z, sin z and the cross sum.  `in` is the layer-0 input jet (input_jet of the body).
template <int NT, int K1, int KRI>
__device__ __forceinline__ void sin_adjoint_to(const float* __restrict__ W0, const float* __restrict__ B0, const f4 (&in)[K1][1],
                                               const f4 (&G)[K1][NT], f4 (&Z)[K1][NT], int p, int q,
                                               const float* __restrict__ xrow, int d_in) {
  f4 w0[NT][1];
  load_w<1, NT>(W0, w0, p, q);
  f4 bias[NT];
  load_bias<NT>(B0, bias, q);
  f4 cz[NT], sz[NT], cross[NT];
#pragma unroll
  for (int MT = 0; MT < NT; ++MT) {
    cross[MT] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float sn, cs;
      sincos_f64arg(sin_layer_z(W0 + (16 * MT + 4 * q + r) * 16, bias[MT][r], xrow, d_in), sn, cs);
      sz[MT][r] = sn; cz[MT][r] = cs;
    }
  }
#pragma unroll
  for (int c = 1; c < K1; ++c) {
    f4 bv[1][1], zd[1][NT];
    bv[0][0] = in[c][0];
    zero_tiles<NT, 1>(zd);
    gemm_chain<1, NT, 1, KRI>(w0, bv, zd);
#pragma unroll
    for (int MT = 0; MT < NT; ++MT)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        cross[MT][r] = fmaf(G[c][MT][r], zd[0][MT][r], cross[MT][r]);
        Z[c][MT][r] = G[c][MT][r] * cz[MT][r];
      }
  }
#pragma unroll
  for (int MT = 0; MT < NT; ++MT)
#pragma unroll
    for (int r = 0; r < 4; ++r) Z[0][MT][r] = fmaf(-sz[MT][r], cross[MT][r], cz[MT][r] * G[0][MT][r]);
}

// acc-layout 16x16 block (features x points) -> operand layout of the weight-gradient GEMM:
// lane (m = lane&15 feature, kq = lane>>4), element s  <-  value(feature m, point 4s + kq).
// Pad layout: row = point (64 B), 16-byte chunk c of a row stored at chunk c ^ (point & 3):
// the b32 column reads are conflict-free, the b128 row writes 2-way.  All writes of a batch are
// issued before any read so the LDS round trip is paid once per batch, not once per block
// (one wave's LDS instructions execute in program order: no barrier needed).
__device__ __forceinline__ void transpose_write(float* __restrict__ tb, f4 v, int p, int q) {
  *reinterpret_cast<f4*>(tb + p * 16 + 4 * (q ^ (p & 3))) = v;
}
__device__ __forceinline__ f4 transpose_read(const float* __restrict__ tb, int p, int q) {
  f4 o;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int pt = 4 * s + q;                                // point index of element s for lane group q
    o[s] = tb[pt * 16 + 4 * ((p >> 2) ^ (pt & 3)) + (p & 3)];   // feature p of that point
  }
  return o;
}

// Second pad layout (weight_grad of the tile kernel only): row = FEATURE (16 points = 64 B), the row's four
// 16-byte chunks rotated by 2 * (feature >> 2).  The write side does the transposition — lane (point p, q) scatters its
// features 4q + r as dwords (two ds_write2_b32, 2-way on the 32 write banks: free) — and the read side takes element s
// <-> point 4 kq + s (the contraction order over points is free as long as both operands use the same one): ONE
// conflict-free ds_read_b128 per block instead of two ds_read2st64_b32 behind a 2-way-conflicted ds_write_b128.
// Measured A/B (round 3, same box): 8x64 6.295 -> 6.258 ms, 10x10 on the tile kernel 0.774 -> 0.764, 100x20 24.19 -> 24.02.
template <int H>   // half H of a block's write: features 4q + 2H and 4q + 2H + 1, one ds_write2_b32
__device__ __forceinline__ void transpose_write2_half(float* __restrict__ tb, f4 v, int p, int q) {
  float* d = tb + (4 * q) * 16 + 4 * (((p >> 2) + 2 * q) & 3) + (p & 3);
  d[(2 * H) * 16] = v[2 * H];
  d[(2 * H + 1) * 16] = v[2 * H + 1];
}
__device__ __forceinline__ void transpose_write2(float* __restrict__ tb, f4 v, int p, int q) {
  transpose_write2_half<0>(tb, v, p, q);
  transpose_write2_half<1>(tb, v, p, q);
}
__device__ __forceinline__ f4 transpose_read2(const float* __restrict__ tb, int p, int q) {   // p: feature, q: point group
  return *reinterpret_cast<const f4*>(tb + p * 16 + 4 * ((q + 2 * (p >> 2)) & 3));
}

// t + (t of lane ^ 16) and t + (t of lane ^ 32) for the bias row sums: v_permlane16_swap / v_permlane32_swap (gfx950) exchange
// whole 16- / 32-lane rows between two registers inside the vector ALU.  Swapping t with a copy of itself leaves
// {r0, r0, r2, r2} and {r1, r1, r3, r3} (rows r0..r3 of t), resp. {lo, lo} and {hi, hi}; their sum is the __shfl_xor form's
// (the operands of an fp32 add commute: bitwise the same) without its ds_bpermute, its address and its LDS round trip.
__device__ __forceinline__ float add_xor16(float t) {
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(t), __float_as_uint(t), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float add_xor32(float t) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(t), __float_as_uint(t), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

constexpr int MAX_LOCKS = 128;

// Where dW/db contributions go.
//  LDSACC: the workgroup's LDS copy of the padded gradient.  LDS fp32 atomics (ds_add_f32)
//    measured ~150 cycles per wave-instruction on gfx950 and dominated the kernel; a plain
//    ds_read_b128 / v_add / ds_write_b128 is ~free.  So each layer's block is guarded by a
//    wave-level spin lock (one ds_cmpst by lane 0) and updated with plain vector RMW.
//  !LDSACC (gradient too large for LDS, e.g. the reference's 100x20 net): the workgroup's copy lives
//    in global memory instead and is updated the same way, under the same LDS locks — plain vector
//    read-modify-write; the waves of a workgroup share one CU's L1, so workgroup-scope fences are all
//    the coherence it takes.  (global_atomic_add_f32 into 16 shared copies was 78 % of the 100x20 step:
//    89.7 ms with, 20.0 ms without the atomics.)
// Weight blocks are stored fragment-native: tile (MT, NT), lane, reg r holds
// dW[16MT + 4(lane>>4) + r][16NT + (lane&15)]  at  woff + ((MT*NT_N + NT)*64 + lane)*4 + r.
template <bool LDSACC>
struct GradSink {
  static constexpr bool LDS = LDSACC;
  float* acc;
  int* locks;
  __device__ __forceinline__ void lock(int l, int lane) const {
    if (lane == 0) {
      int expected = 0;
      while (!__hip_atomic_compare_exchange_strong(locks + l, &expected, 1, __ATOMIC_ACQUIRE, __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_WORKGROUP)) {
        expected = 0;
        __builtin_amdgcn_s_sleep(1);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    __builtin_amdgcn_wave_barrier();
  }
  __device__ __forceinline__ void unlock(int l, int lane) const {
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if (lane == 0) __hip_atomic_store(locks + l, 0, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __device__ __forceinline__ void add1(int idx, float v) const { acc[idx] += v; }
};

// dW[16MT + 4q + r][16NT + n] += sum_c sum_points Z[c][MT](feature, point) * A[c][NT](feature, point)
// db[16MT + m]                += sum_points Z[0][MT](feature m, point)
// A: the layer-input jet in acc layout (registers).
// UNIT_A (layer 0): A[0] is the coordinate block and A[c >= 1] the constant unit tangent delta(feature, dir_col[c - 1]), the same
// for every point.  In operand layout (lane = feature p, element s = a point) that is a lane predicate, so those operands are
// built in registers and only A[0] goes through the pad: per tile 6 LDS writes, 3 LDS reads and the tangent part of the input jet
// less, the same products into the same accumulators in the same k-order.
template <int MT_N, int NT_N, int K1, bool UNIT_A = false, bool PACED = true, class Sink>
__device__ __forceinline__ void weight_grad(const Sink& sink, int layer, int woff, int boff, const f4 (&Z)[K1][MT_N],
                                            const f4 (&A)[K1][NT_N], float* __restrict__ tb, int lane,
                                            const int* __restrict__ dir_col = nullptr) {
  static_assert(!UNIT_A || NT_N == 1, "unit tangents: the layer-0 input block");
  const int p = lane & 15, q = lane >> 4;
  f4 dw[MT_N][NT_N];
  float bs[MT_N], bcur[MT_N];
#pragma unroll
  for (int MT = 0; MT < MT_N; ++MT)
#pragma unroll
    for (int NT = 0; NT < NT_N; ++NT) dw[MT][NT] = f4{0.f, 0.f, 0.f, 0.f};
  // Global gradient copy (!Sink::LDS): take the layer's lock and request the current values NOW, so
  // that the global round trip hides behind the transposes and MFMAs below instead of sitting in the
  // flush (waves of a workgroup are on different layers almost always: holding the lock longer is free).
  f4 early[Sink::LDS ? 1 : MT_N][Sink::LDS ? 1 : NT_N];
  if constexpr (!Sink::LDS) {
    sink.lock(layer, lane);
#pragma unroll
    for (int MT = 0; MT < MT_N; ++MT)
#pragma unroll
      for (int NT = 0; NT < NT_N; ++NT)
        early[MT][NT] = *reinterpret_cast<const f4*>(sink.acc + woff + ((MT * NT_N + NT) * 64 + lane) * 4);
  }
  // Transposes run one quantity AHEAD of the MFMAs that consume them: the LDS round trip of quantity c+1 (same pads:
  // quantity c's reads have already landed in registers) overlaps the MT_N*NT_N*4 MFMAs of quantity c.  The stage of a
  // quantity is 2 (MT_N + NT_N) ds_write2_b32 and then MT_N + NT_N ds_read_b128, 24 at width 64, in this order (one wave's
  // LDS instructions execute in program order: a pad is read after it is written and rewritten after it is read, no
  // barrier).  In one run such a stage costs 24 issue cycles per write and 14 per read among fp32 MFMAs, and the run
  // overflows the 4-bit lgkmcnt; dealt out one by one between the MFMAs it costs about 1 (tools/ubench_coexec.hip, DESIGN
  // 3.1).  So stage(c + 1)'s instruction k is issued in front of MFMA floor(k * SPAN / NOPS) of quantity c, SPAN = the
  // quantity's MFMAs less a tail of an eighth that covers the last read's latency: at width 64 one LDS instruction per
  // 2-3 MFMAs, so 15 consecutive ones span 35 MFMAs (1.1 k cycles) and never 15 are outstanding.  stage(0) has no MFMAs
  // to hide behind and stays in front (issued from the preceding GEMM's tail it was worth 0.0 %, round 3).
  f4 zt[2][MT_N], at[2][NT_N];
  auto stage_op = [&](auto c_, auto k_, f4 (&z)[MT_N], f4 (&a)[NT_N]) {
    constexpr int c = decltype(c_)::value, k = decltype(k_)::value;
    constexpr int NB = MT_N + ((UNIT_A && c > 0) ? 0 : NT_N);      // blocks through the pads: Z's, then A's
    if constexpr (k < 2 * NB) {
      constexpr int B = k / 2;
      if constexpr (B < MT_N) transpose_write2_half<k % 2>(tb + B * TB_FLOATS, Z[c][B], p, q);
      else transpose_write2_half<k % 2>(tb + (4 + B - MT_N) * TB_FLOATS, A[c][B - MT_N], p, q);
    } else {
      constexpr int B = k - 2 * NB;
      if constexpr (B < MT_N) z[B] = transpose_read2(tb + B * TB_FLOATS, p, q);
      else a[B - MT_N] = transpose_read2(tb + (4 + B - MT_N) * TB_FLOATS, p, q);
    }
  };
  auto unit_operand = [&](int c, f4 (&a)[NT_N]) {
    const float e = (p == dir_col[c - 1]) ? 1.f : 0.f;
    a[0] = f4{e, e, e, e};
  };
  const_for<0, 3 * (MT_N + NT_N)>([&](auto k_) { stage_op(std::integral_constant<int, 0>{}, k_, zt[0], at[0]); });
  constexpr int NM = 4 * MT_N * NT_N;                       // MFMAs of a quantity: i = (s * MT_N + MT) * NT_N + NT
  constexpr int SPAN = PACED ? NM - (NM >= 8 ? NM / 8 : 1) : 1;   // (!PACED: the whole stage in front of the quantity's first MFMA)
  const_for<0, K1>([&](auto c_) {
    constexpr int c = decltype(c_)::value;
    constexpr int NOPS = c + 1 < K1 ? 3 * (MT_N + ((UNIT_A && c + 1 > 0) ? 0 : NT_N)) : 0;
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (UNIT_A && c + 1 < K1) unit_operand(c + 1, at[(c + 1) & 1]);
    if constexpr (c == 0) {   // bias: zt[MT][s] = zbar(feature p, point 4s + q): sum the 4 regs here ...
#pragma unroll
      for (int MT = 0; MT < MT_N; ++MT) bs[MT] = (zt[0][MT][0] + zt[0][MT][1]) + (zt[0][MT][2] + zt[0][MT][3]);
    }
    __builtin_amdgcn_sched_barrier(0);
    const_for<0, NM>([&](auto i_) {
      constexpr int i = decltype(i_)::value;
      if constexpr (i < SPAN && NOPS > 0) {
        constexpr int K_LO = (i * NOPS + SPAN - 1) / SPAN, K_HI = ((i + 1) * NOPS + SPAN - 1) / SPAN;
        if constexpr (K_HI > K_LO && i > 0) __builtin_amdgcn_sched_barrier(0);
        const_for<K_LO, K_HI>([&](auto k_) { stage_op(std::integral_constant<int, c + 1>{}, k_, zt[(c + 1) & 1], at[(c + 1) & 1]); });
        if constexpr (K_HI > K_LO && PACED) __builtin_amdgcn_sched_barrier(0);
      }
      constexpr int s = i / (MT_N * NT_N), MT = (i / NT_N) % MT_N, NT = i % NT_N;
      dw[MT][NT] = mfma4(zt[c & 1][MT][s], at[c & 1][NT][s], dw[MT][NT]);
    });
  });
  // ... and the 4 lane groups here, after the last MFMA block (row swaps in the vector ALU: add_xor16 / add_xor32)
#pragma unroll
  for (int MT = 0; MT < MT_N; ++MT) {
    bs[MT] = add_xor32(add_xor16(bs[MT]));
  }
  if constexpr (!Sink::LDS) {
#pragma unroll
    for (int MT = 0; MT < MT_N; ++MT)
#pragma unroll
      for (int NT = 0; NT < NT_N; ++NT)
        *reinterpret_cast<f4*>(sink.acc + woff + ((MT * NT_N + NT) * 64 + lane) * 4) = early[MT][NT] + dw[MT][NT];
  } else {
    sink.lock(layer, lane);
    // one LDS round trip per FUSED_FLUSH_ROWS row blocks (all reads issued, then adds + writes) instead of
    // one per 16x16 block: with a single wave per SIMD the serialized read-add-write chain is exposed
    constexpr int FR = FUSED_FLUSH_ROWS < MT_N ? FUSED_FLUSH_ROWS : MT_N;
#pragma unroll
    for (int M0 = 0; M0 < MT_N; M0 += FR) {
      f4 cur[FR][NT_N];
#pragma unroll
      for (int MT = M0; MT < M0 + FR && MT < MT_N; ++MT)
#pragma unroll
        for (int NT = 0; NT < NT_N; ++NT)
          cur[MT - M0][NT] = *reinterpret_cast<const f4*>(sink.acc + woff + ((MT * NT_N + NT) * 64 + lane) * 4);
      if (M0 == 0) {   // the bias sums' current values ride the first batch of reads (every lane group reads, group 0 writes below)
#pragma unroll
        for (int MT = 0; MT < MT_N; ++MT) bcur[MT] = sink.acc[boff + 16 * MT + p];
      }
      __builtin_amdgcn_sched_barrier(0);   // (a pair: with one, the width-32 kernels' register allocation changes)
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int MT = M0; MT < M0 + FR && MT < MT_N; ++MT)
#pragma unroll
        for (int NT = 0; NT < NT_N; ++NT)
          *reinterpret_cast<f4*>(sink.acc + woff + ((MT * NT_N + NT) * 64 + lane) * 4) = cur[MT - M0][NT] + dw[MT][NT];
    }
  }
  if (q == 0) {
#pragma unroll
    for (int MT = 0; MT < MT_N; ++MT) {
      if constexpr (Sink::LDS) sink.acc[boff + 16 * MT + p] = bcur[MT] + bs[MT];
      else sink.add1(boff + 16 * MT + p, bs[MT]);
    }
  }
  sink.unlock(layer, lane);
}

__device__ __forceinline__ float pick4(f4 v, int i) {
  return i == 0 ? v[0] : (i == 1 ? v[1] : (i == 2 ? v[2] : v[3]));
}
// output column o of the (single) output tile, for this lane's point
__device__ __forceinline__ float gather_out(f4 tile, int o, int p) {
  return __shfl(pick4(tile, o & 3), p + 16 * (o >> 2), 64);
}
// (the operands are passed BY VALUE: written as `(qi == c) ? out[c][0] : v` the conditional load became a select of
// ADDRESSES and one load — a dynamically indexed stack array.  The output tiles then lived in scratch memory, 64-80 bytes
// per lane in every residual instance, and each of the epilogue's reloads waited with vmcnt(0), i.e. for the reverse
// sweep's prefetched weight blocks as well)
__device__ __forceinline__ f4 select4(bool take, f4 a, f4 b) { return take ? a : b; }
template <int K1>
__device__ __forceinline__ f4 pick_q(const f4 (&out)[K1][1], int qi) {
  f4 v = out[0][0];
#pragma unroll
  for (int c = 1; c < K1; ++c) v = select4(qi == c, out[c][0], v);
  return v;
}

// Per-lane lookup built once per kernel: which role (residual output role / mse target column)
// lands in this lane's accumulator register r2 (-1: none), and which residual quantity maps to
// engine quantity ce (-1: none).  Kept as small integers so that nothing but these is hoisted
// out of the tile loop (hoisted lane predicates would each pin an SGPR pair).
template <int K1>
struct ScatterMap {
  int role_of[4];
  int cinv[K1];
};

// roles' adjoints g[c][r] (identical in all four lane groups) -> adjoint tile G in acc layout,
// through the wave-private LDS pad (idle at this point): row (c*NR + r) holds the 16 points.
template <int K1, int NC, int NR, bool ACCUM = false>
__device__ __forceinline__ void scatter_adjoint(float* __restrict__ tb, const float (&g)[NC][NR],
                                                const ScatterMap<K1>& sm, f4 (&G)[K1][1], bool valid, int p, int q) {
  if (q == 0) {
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int r = 0; r < NR; ++r) tb[(c * NR + r) * 16 + p] = g[c][r];
  }
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int ce = 0; ce < K1; ++ce)
#pragma unroll
    for (int r2 = 0; r2 < 4; ++r2) {
      const int ci = sm.cinv[ce], ro = sm.role_of[r2];
      const bool ok = valid && ci >= 0 && ci < NC && ro >= 0;
      const float val = tb[ok ? (ci * NR + ro) * 16 + p : p];
      G[ce][0][r2] = (ACCUM ? G[ce][0][r2] : 0.f) + (ok ? val : 0.f);
    }
  __builtin_amdgcn_wave_barrier();
}

// The residual's closure (residuals.h) from the parameter block — the one place here that knows which residual takes what:
// continuity its anchor switch, this point's mask and the anchor value; the wave closure (omega, gamma), which
// set_residual_roles puts into P.thr and P.anchor (spec.param[0..1]); the others nothing.
template <class RES>
__device__ __forceinline__ typename RES::Closure residual_closure(const FusedParams& P, bool masked) {
  if constexpr (std::is_same<RES, ResContinuity>::value) return {P.residual_id == PINN_RES_CONTINUITY_ONLY, masked, P.anchor};
  else if constexpr (std::is_same<RES, ResPhysicsEquationWave>::value) return {P.thr, P.anchor};
  else return {};
}

// Evaluate one residual family on the gathered jet; writes the adjoint tile G (acc layout).
template <class RES, int K1, bool GRAD>
__device__ __forceinline__ void residual_tile(const FusedParams& P, const f4 (&out)[K1][1], f4 (&G)[K1][1],
                                              float (&sums)[MAX_SUMS], const ScatterMap<K1>& sm,
                                              float* __restrict__ tb, bool valid, bool masked, int p, int q,
                                              bool primary = true) {
  constexpr int NR = RES::NR, ND = RES::ND, NT = RES::NT;
  float v[1 + ND][NR], g[1 + ND][NR], sq[NT], sc[NT];
#pragma unroll
  for (int c = 0; c <= ND; ++c) {
    const f4 tile = (c == 0) ? out[0][0] : pick_q<K1>(out, P.q_of[c - 1]);
#pragma unroll
    for (int r = 0; r < NR; ++r) v[c][r] = gather_out(tile, P.out_col[r], p);
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) sc[t] = GRAD ? P.scale[t] : 0.f;
  RES::template eval<GRAD>(v, residual_closure<RES>(P, masked), sc, g, sq);
  if (valid && q == 0 && primary) {
#pragma unroll
    for (int t = 0; t < NT; ++t) sums[term_slot(t)] += sq[t];
  }
  if constexpr (GRAD) scatter_adjoint<K1, 1 + ND, NR>(tb, g, sm, G, valid, p, q);
}

// P.out_col entries of roles the residual does not use must be -1 (pinn_abi.hip check_spec normalises every spec):
// the search below covers all PINN_MAX_ROLES entries, and a stale 0 would claim output column 0.
template <int K1>
__device__ __forceinline__ void build_scatter_maps(const FusedParams& P, int q, ScatterMap<K1>& sm, ScatterMap<K1>& sm_mse) {
#pragma unroll
  for (int r2 = 0; r2 < 4; ++r2) {
    int ro = -1, rm = -1;
    for (int r = PINN_MAX_ROLES - 1; r >= 0; --r) {
      ro = (P.out_col[r] == 4 * q + r2) ? r : ro;
      rm = (r < P.n_cols && P.mse_col[r] == 4 * q + r2) ? r : rm;
    }
    sm.role_of[r2] = ro;
    sm_mse.role_of[r2] = rm;
  }
  sm.cinv[0] = 0; sm_mse.cinv[0] = 0;
#pragma unroll
  for (int ce = 1; ce < K1; ++ce) {
    int ci = -1;
    for (int d = PINN_MAX_DIRS - 1; d >= 0; --d) ci = (P.q_of[d] == ce) ? 1 + d : ci;
    sm.cinv[ce] = ci;
    sm_mse.cinv[ce] = -1;
  }
}

// Everything that happens on the output tile of one 16-point tile: optional Y/dY stores, PDE
// residual and/or fidelity MSE (train.py:131-157), loss partial sums, output adjoint G.
// EPI_ADJ ("external adjoint", pinn_jet_backward): no residual, no MSE, no stores, no loss sums — the output adjoint
// comes from the caller (load_adjoint below) and loss_epilogue is not called at all.
// EPI_FIELD (pinn_residual_fields): forward only — the residual's signed field values of every point are stored
// (field_epilogue below) and nothing else happens: no sums, no Y / dY stores, no adjoint, no reverse sweep.
// EPI_PEC: the loss epilogue with the residual family fixed to ResPhysicsEquationCorrected (pec_epilogue below): serves what
// EPI_GENERIC serves (residual, residual + fidelity columns, split mode) but stores no Y / dY.  EPI_FIELD_PEC: EPI_FIELD
// for that residual.  EPI_WAVE / EPI_FIELD_WAVE: the same pair for ResPhysicsEquationWave (the wave units of
// pinn_fused_tile.hip; no batch instances).  All are compile-time choices with translation units of their own (the pec units of
// pinn_fused_tile.hip and pinn_fused_batch.hip), so the generic epilogues do not grow by a branch.
// EPI_COEF (pinn_residual_coef_loss_grad): the EPI_NS / EPI_PE epilogue with the residual's closure coefficient read from
// a device array (coef_epilogue below) and its gradient summed beside the term sums; translation units of its own too
// (pinn_fused_tile.hip, TF_COEF).
// EPI_WEIGHTED (pinn_residual_weighted_loss_grad): the residual epilogue of any first-order family with one weight per point
// and weighted term (weighted_epilogue below), and an optional store of the signed fields; translation units of its own
// (pinn_fused_tile.hip, TF_WEIGHTED).
constexpr int EPI_GENERIC = 0, EPI_NS = 1, EPI_PE = 2, EPI_CONT = 3, EPI_ADJ = 4, EPI_FIELD = 5, EPI_PEC = 6, EPI_FIELD_PEC = 7,
              EPI_COEF = 8, EPI_WEIGHTED = 9, EPI_WAVE = 10, EPI_FIELD_WAVE = 11;
constexpr int COEF_SUM = 3;   // EPI_COEF: the term slot of [0, MSE_SUM0) that carries gc[0] (PINN_NS_TERMS = PINN_PE_TERMS = 3 leave it free)

// The mirror of the generic epilogue's Y / dY store: lane (p, q), register r of G[c][0] is output o = 4q + r of point pt;
// G[0] <- gY, G[c] <- gdY row c - 1.  Zero for o >= d_out, for the invalid points of the last tile and for a null array.
template <int K1>
__device__ __forceinline__ void load_adjoint(const FusedParams& P, f4 (&G)[K1][1], int64_t pt, bool valid, int q) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int o = 4 * q + r;
    const bool ok = valid && o < P.d_out;
    G[0][0][r] = (ok && P.gY != nullptr) ? P.gY[pt * P.d_out + o] : 0.f;
#pragma unroll
    for (int c = 1; c < K1; ++c)
      G[c][0][r] = (ok && P.gdY != nullptr) ? P.gdY[((int64_t)(c - 1) * P.N + pt) * P.d_out + o] : 0.f;
  }
}

// EPI_FIELD: gather the roles' jets as residual_tile does, evaluate RES::fields and store field f of point pt at
// fields[f * N + pt] (fields = P.Y, see FusedParams) — field-major, as dY: each field is a contiguous map and a tile's store of one field is 64
// contiguous bytes (lane group q == 0, one float per valid point).
template <class RES, int K1>
__device__ __forceinline__ void field_tile(const FusedParams& P, const f4 (&out)[K1][1], int64_t pt, bool valid,
                                           bool masked, int p, int q) {
  constexpr int NR = RES::NR, ND = RES::ND, NF = RES::NF;
  float v[1 + ND][NR], f[NF];
#pragma unroll
  for (int c = 0; c <= ND; ++c) {
    const f4 tile = (c == 0) ? out[0][0] : pick_q<K1>(out, P.q_of[c - 1]);
#pragma unroll
    for (int r = 0; r < NR; ++r) v[c][r] = gather_out(tile, P.out_col[r], p);
  }
  RES::fields(v, residual_closure<RES>(P, masked), f);
  if (valid && q == 0) {
#pragma unroll
    for (int t = 0; t < NF; ++t) P.Y[(int64_t)t * P.N + pt] = f[t];
  }
}
// K1 decides the family (the host refuses any other pairing): 4 = Navier-Stokes; 3 = physics_equation or continuity, told
// apart by one wave-uniform branch on residual_id.
template <int K1>
__device__ __forceinline__ void field_epilogue(const FusedParams& P, const f4 (&out)[K1][1], int64_t pt, int64_t ptc,
                                               bool valid, int p, int q) {
  static_assert(K1 == 3 || K1 == 4, "EPI_FIELD: K1 = 1 + the residual's directions");
  if constexpr (K1 == 4) field_tile<ResNavierStokes, K1>(P, out, pt, valid, false, p, q);
  else if (P.residual_id == PINN_RES_PHYSICS_EQUATION) field_tile<ResPhysicsEquation, K1>(P, out, pt, valid, false, p, q);
  else {
    const bool masked = P.residual_id == PINN_RES_CONTINUITY_ONLY && P.X[ptc * P.d_in + P.xcol] < P.thr;
    field_tile<ResContinuity, K1>(P, out, pt, valid, masked, p, q);
  }
}

// EPI_COEF: residual_tile with a coefficient residual (residuals.h: ResNavierStokesCoef, ResPhysicsEquationCoef).  The
// coefficients are P.gY (see FusedParams: only the EPI_ADJ instances read it otherwise, and FusedParams must not grow);
// the point's coefficient gradient gc[0] joins sums[COEF_SUM] under the term sums' own predicate, so it reaches the host
// side through wg_sums and the fixed-order double reduction and is bit-reproducible as they are.
template <class RES, int K1, bool GRAD>
__device__ __forceinline__ void residual_tile_coef(const FusedParams& P, const f4 (&out)[K1][1], f4 (&G)[K1][1],
                                                   float (&sums)[MAX_SUMS], const ScatterMap<K1>& sm,
                                                   float* __restrict__ tb, bool valid, int p, int q) {
  constexpr int NR = RES::NR, ND = RES::ND, NT = RES::NT, NC = RES::NC;
  static_assert(NT <= COEF_SUM && NC == 1, "EPI_COEF: one coefficient, its gradient in the free term slot");
  float v[1 + ND][NR], g[1 + ND][NR], sq[NT], sc[NT], cf[NC], gc[NC];
#pragma unroll
  for (int c = 0; c <= ND; ++c) {
    const f4 tile = (c == 0) ? out[0][0] : pick_q<K1>(out, P.q_of[c - 1]);
#pragma unroll
    for (int r = 0; r < NR; ++r) v[c][r] = gather_out(tile, P.out_col[r], p);
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) sc[t] = GRAD ? P.scale[t] : 0.f;
#pragma unroll
  for (int j = 0; j < NC; ++j) cf[j] = P.gY[j];
  RES::template eval<GRAD>(v, cf, sc, g, sq, gc);
  if (valid && q == 0) {
#pragma unroll
    for (int t = 0; t < NT; ++t) sums[t] += sq[t];
    if (GRAD) sums[COEF_SUM] += gc[0];
  }
  if constexpr (GRAD) scatter_adjoint<K1, 1 + ND, NR>(tb, g, sm, G, valid, p, q);
}
// K1 decides the family (the host refuses any other pairing): 4 = Navier-Stokes, 3 = physics_equation.  Residual loss only:
// no output stores, no fidelity columns, no split.
template <int K1, bool GRAD>
__device__ __forceinline__ void coef_epilogue(const FusedParams& P, const f4 (&out)[K1][1], f4 (&G)[K1][1],
                                              float (&sums)[MAX_SUMS], const ScatterMap<K1>& sm,
                                              float* __restrict__ tb, bool valid, int p, int q) {
  static_assert(K1 == 3 || K1 == 4, "EPI_COEF: K1 = 1 + the residual's directions");
#pragma unroll
  for (int c = 0; c < K1; ++c) G[c][0] = f4{0.f, 0.f, 0.f, 0.f};
  if constexpr (K1 == 4) residual_tile_coef<ResNavierStokesCoef, K1, GRAD>(P, out, G, sums, sm, tb, valid, p, q);
  else residual_tile_coef<ResPhysicsEquationCoef, K1, GRAD>(P, out, G, sums, sm, tb, valid, p, q);
}

// EPI_WEIGHTED: residual_tile with a weight on every point's squares.  The weights are P.gY, (w_rows, N) row-major with row
// stride P.n_split (0: one row serves every term; N: row t weights term t), the optional fields array is P.Y (see FusedParams:
// it must not grow).  Term t < NW = min(terms, fields) takes scale[t] * w_t into the adjoint and w_t * sq[t] into its sum;
// terms from NW on (continuity_only's point count) go in unweighted.  The weight is read at the CLAMPED point index ptc, so
// the lanes of a ragged last tile stay inside their row; their sums and adjoints are dropped by `valid` as everywhere.
template <class RES, int K1, bool GRAD>
__device__ __forceinline__ void residual_tile_weighted(const FusedParams& P, const f4 (&out)[K1][1], f4 (&G)[K1][1],
                                                       float (&sums)[MAX_SUMS], const ScatterMap<K1>& sm,
                                                       float* __restrict__ tb, int64_t pt, int64_t ptc, bool valid,
                                                       bool masked, int p, int q) {
  constexpr int NR = RES::NR, ND = RES::ND, NT = RES::NT, NF = RES::NF, NW = NT < NF ? NT : NF;
  float v[1 + ND][NR], g[1 + ND][NR], sq[NT], sc[NT], w[NW];
#pragma unroll
  for (int c = 0; c <= ND; ++c) {
    const f4 tile = (c == 0) ? out[0][0] : pick_q<K1>(out, P.q_of[c - 1]);
#pragma unroll
    for (int r = 0; r < NR; ++r) v[c][r] = gather_out(tile, P.out_col[r], p);
  }
#pragma unroll
  for (int t = 0; t < NW; ++t) w[t] = P.gY[(int64_t)t * P.n_split + ptc];
  // the weighted sums and the field store take the fields formed apart from the adjoint's arithmetic (residuals.h,
  // isolated_fields): the forward-only and the gradient instance round them alike
  float f[NF];
  isolated_fields<RES>(v, residual_closure<RES>(P, masked), f);
#pragma unroll
  for (int t = 0; t < NT; ++t) sc[t] = GRAD ? (t < NW ? P.scale[t] * w[t] : P.scale[t]) : 0.f;
  RES::template eval<GRAD>(v, residual_closure<RES>(P, masked), sc, g, sq);
  if (valid && q == 0) {
#pragma unroll
    for (int t = 0; t < NT; ++t) sums[t] = t < NW ? __fmaf_rn(w[t], f[t] * f[t], sums[t]) : sums[t] + sq[t];
    if (P.Y != nullptr) {   // the signed fields, as field_tile stores them
#pragma unroll
      for (int t = 0; t < NF; ++t) P.Y[(int64_t)t * P.N + pt] = f[t];
    }
  }
  if constexpr (GRAD) scatter_adjoint<K1, 1 + ND, NR>(tb, g, sm, G, valid, p, q);
}
// K1 decides the family as for field_epilogue.  Residual loss only: no Y / dY stores, no fidelity columns, no split.
template <int K1, bool GRAD>
__device__ __forceinline__ void weighted_epilogue(const FusedParams& P, const f4 (&out)[K1][1], f4 (&G)[K1][1],
                                                  float (&sums)[MAX_SUMS], const ScatterMap<K1>& sm,
                                                  float* __restrict__ tb, int64_t pt, int64_t ptc, bool valid, int p, int q) {
  static_assert(K1 == 3 || K1 == 4, "EPI_WEIGHTED: K1 = 1 + the residual's directions");
#pragma unroll
  for (int c = 0; c < K1; ++c) G[c][0] = f4{0.f, 0.f, 0.f, 0.f};
  if constexpr (K1 == 4) residual_tile_weighted<ResNavierStokes, K1, GRAD>(P, out, G, sums, sm, tb, pt, ptc, valid, false, p, q);
  else if (P.residual_id == PINN_RES_PHYSICS_EQUATION)
    residual_tile_weighted<ResPhysicsEquation, K1, GRAD>(P, out, G, sums, sm, tb, pt, ptc, valid, false, p, q);
  else {
    const bool masked = P.residual_id == PINN_RES_CONTINUITY_ONLY && P.X[ptc * P.d_in + P.xcol] < P.thr;
    residual_tile_weighted<ResContinuity, K1, GRAD>(P, out, G, sums, sm, tb, pt, ptc, valid, masked, p, q);
  }
}

// EPI_PEC: loss_epilogue_impl's generic part (below) with ONE residual family and without the output stores — the split
// rule and the fidelity columns are its lines, repeated here because that function must stay as the compiler sees it today.
// EPI_WAVE: the same epilogue with RES = ResPhysicsEquationWave (five terms: residual_tile's term_slot rule; at most
// WAVE_MAX_COLS fidelity columns, which the host checks).
template <int K1, bool GRAD, bool SPLIT, class RES = ResPhysicsEquationCorrected>
__device__ __forceinline__ void pec_epilogue(const FusedParams& P, const f4 (&out)[K1][1], f4 (&G)[K1][1],
                                             float (&sums)[MAX_SUMS], const ScatterMap<K1>& sm,
                                             const ScatterMap<K1>& sm_mse, float* __restrict__ tb, int64_t pt,
                                             int64_t ptc, bool valid, int p, int q) {
  static_assert(K1 == 3, "EPI_PEC: K1 = 1 + the residual's two directions");
#pragma unroll
  for (int c = 0; c < K1; ++c) G[c][0] = f4{0.f, 0.f, 0.f, 0.f};
  const bool valid_r = SPLIT ? (valid && pt < P.n_split) : valid;
  const bool valid_m = SPLIT ? (valid && pt >= P.n_split) : valid;
  if (P.loss_kind & 1) residual_tile<RES, K1, GRAD>(P, out, G, sums, sm, tb, valid_r, false, p, q);
  if (P.loss_kind & 2) {
    float gm[1][PINN_MAX_ROLES];
#pragma unroll
    for (int j = 0; j < PINN_MAX_ROLES; ++j) {
      gm[0][j] = 0.f;
      if (j < P.n_cols) {
        const float y = gather_out(out[0][0], P.mse_col[j], p);
        const int64_t trow = SPLIT ? (valid_m ? ptc - P.n_split : 0) : ptc;
        const float d = P.T[trow * P.n_cols + j] - y;                 // train.py:141 (true - pred)
        if (valid_m && q == 0) sums[MSE_SUM0 + j] += d * d;
        if (GRAD) gm[0][j] = -2.f * P.mse_scale[j] * d;
      }
    }
    if constexpr (GRAD) scatter_adjoint<K1, 1, PINN_MAX_ROLES, true>(tb, gm, sm_mse, G, valid_m, p, q);
  }
}

template <int K1, bool GRAD, bool SPLIT, int EPI = EPI_GENERIC>
__device__ __forceinline__ void loss_epilogue_impl(const FusedParams& P, const f4 (&out)[K1][1], f4 (&G)[K1][1],
                                              float (&sums)[MAX_SUMS], const ScatterMap<K1>& sm,
                                              const ScatterMap<K1>& sm_mse, float* __restrict__ tb, int64_t pt,
                                              int64_t ptc, bool valid, int p, int q, bool primary = true) {
  static_assert(EPI != EPI_ADJ, "EPI_ADJ has no epilogue: k_fused calls load_adjoint instead");
  static_assert(EPI != EPI_FIELD && EPI != EPI_FIELD_PEC && EPI != EPI_FIELD_WAVE, "EPI_FIELD has its own epilogue: k_fused calls field_epilogue instead");
  static_assert(EPI != EPI_PEC && EPI != EPI_WAVE, "EPI_PEC has its own epilogue: loss_epilogue calls pec_epilogue instead");
  // EPI != 0: an epilogue specialised to ONE residual family, residual loss only, no output stores.
  // The generic epilogue keeps every family, the fidelity columns and the Y/dY stores behind runtime
  // switches; at width 64 that costs 146 spilled SGPRs (372 v_readlane per tile) against 4 with the
  // specialised form, and the 2^20-point Navier-Stokes step 1.1 % (6.89 -> 6.82 ms, same box).
  if constexpr (EPI != EPI_GENERIC) {
#pragma unroll
    for (int c = 0; c < K1; ++c) G[c][0] = f4{0.f, 0.f, 0.f, 0.f};
    if constexpr (EPI == EPI_NS) {
      if constexpr (K1 >= 4) residual_tile<ResNavierStokes, K1, GRAD>(P, out, G, sums, sm, tb, valid, false, p, q, primary);
    } else if constexpr (EPI == EPI_PE) {
      if constexpr (K1 >= 3) residual_tile<ResPhysicsEquation, K1, GRAD>(P, out, G, sums, sm, tb, valid, false, p, q, primary);
    } else {
      if constexpr (K1 >= 3) {
        const bool masked = P.residual_id == PINN_RES_CONTINUITY_ONLY && P.X[ptc * P.d_in + P.xcol] < P.thr;
        residual_tile<ResContinuity, K1, GRAD>(P, out, G, sums, sm, tb, valid, masked, p, q, primary);
      }
    }
    return;
  }
  // primary == false (cooperative kernel, waves 1..3): compute the output adjoint only — no stores, no sums
  if (P.Y != nullptr && valid && primary) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int o = 4 * q + r;
      if (o < P.d_out) {
        P.Y[pt * P.d_out + o] = out[0][0][r];
        if (P.dY != nullptr) {
#pragma unroll
          for (int c = 1; c < K1; ++c) P.dY[((int64_t)(c - 1) * P.N + pt) * P.d_out + o] = out[c][0][r];
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < K1; ++c) G[c][0] = f4{0.f, 0.f, 0.f, 0.f};
  // split mode (train.py:131-157 in one launch): collocation points first, fidelity points after them
  // SPLIT is a template parameter so that the common (unsplit) epilogue is untouched: even two extra
  // compares in this register-starved region cost the 2^20-point step 0.5-2.5 % (measured)
  const bool valid_r = SPLIT ? (valid && pt < P.n_split) : valid;
  const bool valid_m = SPLIT ? (valid && pt >= P.n_split) : valid;
  if (P.loss_kind & 1) {
    if (P.residual_id == PINN_RES_NAVIER_STOKES) {
      if constexpr (K1 >= 4) residual_tile<ResNavierStokes, K1, GRAD>(P, out, G, sums, sm, tb, valid_r, false, p, q, primary);
    } else if (P.residual_id == PINN_RES_PHYSICS_EQUATION) {
      if constexpr (K1 >= 3) residual_tile<ResPhysicsEquation, K1, GRAD>(P, out, G, sums, sm, tb, valid_r, false, p, q, primary);
    } else {
      if constexpr (K1 >= 3) {
        const bool masked = P.residual_id == PINN_RES_CONTINUITY_ONLY && P.X[ptc * P.d_in + P.xcol] < P.thr;
        residual_tile<ResContinuity, K1, GRAD>(P, out, G, sums, sm, tb, valid_r, masked, p, q, primary);
      }
    }
  }
  if (P.loss_kind & 2) {
    float gm[1][PINN_MAX_ROLES];
#pragma unroll
    for (int j = 0; j < PINN_MAX_ROLES; ++j) {
      gm[0][j] = 0.f;
      if (j < P.n_cols) {
        const float y = gather_out(out[0][0], P.mse_col[j], p);
        const int64_t trow = SPLIT ? (valid_m ? ptc - P.n_split : 0) : ptc;
        const float d = P.T[trow * P.n_cols + j] - y;                 // train.py:141 (true - pred)
        if (valid_m && q == 0 && primary) sums[MSE_SUM0 + j] += d * d;
        if (GRAD) gm[0][j] = -2.f * P.mse_scale[j] * d;
      }
    }
    if constexpr (GRAD) scatter_adjoint<K1, 1, PINN_MAX_ROLES, true>(tb, gm, sm_mse, G, valid_m, p, q);
  }
}

// SPLIT_OK = false leaves the split-mode code out of the kernel altogether: k_fused at width 64 is so
// register-starved around the epilogue that even a never-taken second copy of it cost the 2^20-point
// step 5 % (and two extra compares in the single copy 0.5-2.5 %); the host runs split requests that
// would land on that kernel as two passes instead (pinn_fused.hip).
template <int K1, bool GRAD, bool SPLIT_OK = true, int EPI = EPI_GENERIC>
__device__ __forceinline__ void loss_epilogue(const FusedParams& P, const f4 (&out)[K1][1], f4 (&G)[K1][1],
                                              float (&sums)[MAX_SUMS], const ScatterMap<K1>& sm,
                                              const ScatterMap<K1>& sm_mse, float* __restrict__ tb, int64_t pt,
                                              int64_t ptc, bool valid, int p, int q, bool primary = true) {
  if constexpr (EPI == EPI_PEC || EPI == EPI_WAVE) {     // (primary: the cooperative kernel's, which has no such instance)
    typedef typename std::conditional<EPI == EPI_WAVE, ResPhysicsEquationWave, ResPhysicsEquationCorrected>::type RES;
    if constexpr (SPLIT_OK) {
      if (P.n_split >= 0) { pec_epilogue<K1, GRAD, true, RES>(P, out, G, sums, sm, sm_mse, tb, pt, ptc, valid, p, q); return; }
    }
    pec_epilogue<K1, GRAD, false, RES>(P, out, G, sums, sm, sm_mse, tb, pt, ptc, valid, p, q);
    return;
  } else if constexpr (SPLIT_OK && EPI == EPI_GENERIC) {
    if (P.n_split >= 0) {
      loss_epilogue_impl<K1, GRAD, true>(P, out, G, sums, sm, sm_mse, tb, pt, ptc, valid, p, q, primary);
      return;
    }
  }
  if constexpr (EPI != EPI_PEC && EPI != EPI_WAVE) loss_epilogue_impl<K1, GRAD, false, EPI>(P, out, G, sums, sm, sm_mse, tb, pt, ptc, valid, p, q, primary);
}

// Diagnostic build only (-DPINN_DIAG): s_memtime stamps per phase, printed by wave 0 of block 0.
// Stamps drain the memory counters, so read the SHARES, never the total (cdna guide §7).
#ifdef PINN_DIAG
#define PINN_STAMP(i)                                                                      \
  do {                                                                                     \
    unsigned long long t_;                                                                 \
    __builtin_amdgcn_sched_barrier(0);                                                     \
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory"); \
    __builtin_amdgcn_sched_barrier(0);                                                     \
    diag[i] += t_ - tprev;                                                                 \
    tprev = t_;                                                                            \
  } while (0)
#else
#define PINN_STAMP(i) do { } while (0)
#endif

// KRO > 0 (the specialised-epilogue kernels of width 64): network inputs and outputs sit in K-STEP-MAJOR order — input
// column f at padded index perm16(f) = 4 (f & 3) + (f >> 2), i.e. lane group f, register 0 for d_in <= 4, and output o at
// padded row perm16(o) — so the first layer's forward GEMM is ONE k-step instead of four and the output layer's reverse
// GEMM KRO = ceil(d_out / 4) k-steps (Navier-Stokes 3 -> 8x64 -> 4: 96 of the tile's 5696 MFMAs gone).  The packing
// kernels place the weights accordingly (pinn_fused.hip, PACK_IN / PACK_OUT) and the host hands the epilogue PADDED row
// indices in out_col / dir_col, so the epilogue code is the same.
//
// Ensembles (k_fused_ens below; pinn_fused_tile.hip, TF_ENS): launched on a 2-D grid (gx, M), member = blockIdx.y.  blockIdx.x
// and gridDim.x keep their per-member meaning, so the body is the single-network code: the ensemble kernel only shifts the
// pointers it was given to its member's share, once (ens_member), and k_fused stays as it was.
// Member strides: packed Wp / WTp PW floats, Bp PB floats, spill slots gridDim.x * FUSED_WAVES * scratch_per_wave, wg_sums
// gridDim.x * MAX_SUMS, wg_grads gridDim.x * (PW + PB); X and T are shared by all members unless a flag bit says that
// every member has its own array: ENS_OWN_X / ENS_OWN_T, carried in batch_T — a field no k_fused instance reads — because
// FusedParams must not grow (see Y above).
constexpr int ENS_OWN_X = 1, ENS_OWN_T = 2;
__device__ __forceinline__ void ens_member(FusedParams& P) {
  const int64_t mem = blockIdx.y, gx = gridDim.x;
  P.Wp += mem * P.PW; P.WTp += mem * P.PW; P.Bp += mem * P.PB;
  P.scratch += mem * gx * FUSED_WAVES * P.scratch_per_wave;
  P.wg_sums += mem * gx * MAX_SUMS;
  P.wg_grads += mem * gx * (P.PW + P.PB);
  if (P.batch_T & ENS_OWN_X) P.X += mem * P.N * P.d_in;
  if (P.batch_T & ENS_OWN_T) P.T += mem * (P.n_split >= 0 ? P.N - P.n_split : P.N) * P.n_cols;
}

// The kernel's body is the TEXT of fused_tile_body.inc, included into k_fused and into k_fused_ens: k_fused's statements are
// the ones they were, token for token, so every existing instance compiles as before (a shared __device__ function around
// the body changed the register allocation of a third of them).
template <int WP, int K1, bool GRAD, bool LDSACC, int ACT, int EPI = EPI_GENERIC, int KRO = 0, bool DROP = false>
__global__ __launch_bounds__(FUSED_THREADS, WP == 16 ? FUSED_W16_WAVES : FUSED_WAVES / 4) void k_fused(const FusedParams P) {
  static_assert(!DROP || (ACT == PINN_ACT_TANH && KRO == 0), "dropout instances: tanh, natural unit order");
  static_assert(EPI != EPI_ADJ || (GRAD && KRO == 0 && !DROP), "external-adjoint instances: gradient pass, natural unit order, no dropout");
  static_assert(EPI != EPI_FIELD || (!GRAD && !LDSACC && KRO == 0 && !DROP), "field instances: forward only, natural unit order, no dropout");
  static_assert(EPI != EPI_FIELD_PEC || (!GRAD && !LDSACC && KRO == 0 && !DROP && K1 == 3), "field instances: forward only, natural unit order, no dropout");
  static_assert(EPI != EPI_PEC || (KRO == 0 && !DROP && K1 == 3 && ACT == PINN_ACT_TANH), "corrected-residual instances: tanh, k = 2, natural unit order, no dropout");
  static_assert(EPI != EPI_FIELD_WAVE || (!GRAD && !LDSACC && KRO == 0 && !DROP && K1 == 3), "field instances: forward only, natural unit order, no dropout");
  static_assert(EPI != EPI_WAVE || (KRO == 0 && !DROP && K1 == 3 && ACT == PINN_ACT_TANH), "wave-closure instances: tanh, k = 2, natural unit order, no dropout");
  static_assert(EPI != EPI_COEF || (KRO == 0 && !DROP && (K1 == 3 || K1 == 4) && ACT == PINN_ACT_TANH), "coefficient instances: tanh, k = 2 or 3, natural unit order, no dropout");
  static_assert(EPI != EPI_WEIGHTED || (KRO == 0 && !DROP && (K1 == 3 || K1 == 4) && ACT == PINN_ACT_TANH), "weighted instances: tanh, k = 2 or 3, natural unit order, no dropout");
  static_assert(ACT != PINN_ACT_SIN_TANH || (EPI == EPI_GENERIC && KRO == 0 && !DROP && (K1 == 1 || K1 == 3 || K1 == 4)), "sine-first-layer instances: generic epilogue, k = 0, 2 or 3, natural unit order, no dropout");
#include "fused_tile_body.inc"
}

// The ensemble instances (pinn_fused_tile.hip, TF_ENS): gradient passes of tanh networks with the generic epilogue in natural
// unit order, launched on a 2-D grid (gx, M) — one row of workgroups per member.
// Width 16 is compiled for FUSED_ENS_W16_WAVES = 2 waves per SIMD, not k_fused's three: at three (168 registers) the
// width-16 gradient kernels keep 40 to 216 bytes per lane in scratch memory, at two they keep none.
constexpr int FUSED_ENS_W16_WAVES = 2;
template <int WP, int K1, bool LDSACC>
__global__ __launch_bounds__(FUSED_THREADS, WP == 16 ? FUSED_ENS_W16_WAVES : FUSED_WAVES / 4) void k_fused_ens(const FusedParams P_arg) {
  static_assert(K1 == 3 || K1 == 4, "ensemble instances: k = 2 or 3");
  constexpr bool GRAD = true, DROP = false;
  constexpr int ACT = PINN_ACT_TANH, EPI = EPI_GENERIC, KRO = 0;
  FusedParams P_mem = P_arg;
  ens_member(P_mem);
  const FusedParams& P = P_mem;
#include "fused_tile_body.inc"
}

// launcher: fused_launch.h (launch_tile); the instances, one translation unit per (family, WP): pinn_fused_tile.hip

}  // namespace pinn
