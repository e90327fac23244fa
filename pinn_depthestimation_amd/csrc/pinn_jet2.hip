// pinn_jet2.hip — second-order forward-mode jets, generic VALU and MFMA layer kernels (pinn_forward_jet2 /
// pinn_jet2_backward): compute_gradient (physics.py:6-15) applied twice, and the parameter gradient of anything
// built from the result (train.py:191).  Shape-agnostic like pinn_generic.hip: one thread per point, one kernel
// per layer, jets in a feature-major workspace [channel c][feature f][point n].
//
// Channels (K differentiated inputs, P = K (K+1) / 2 unordered pairs, upper triangle row-major):
//   c = 0            value                 a
//   c = 1 + i        first order           adot_i  = d a / d x_{dir_col[i]}
//   c = 1 + K + p    second order, pair p  addot_ij = d^2 a / d x_i d x_j   (p = pair_index(i, j), i <= j)
// Seeds a = x, adot_i = e_{dir_col[i]}, addot = 0.  Each linear layer maps every channel through the same W
// (z = W a + b, zdot = W adot, zddot = W addot); each hidden activation, with t = act(z):
//   tanh:  s = 1 - t^2,  adot_i = s zdot_i,  addot_ij = s zddot_ij - 2 t s zdot_i zdot_j
//   leaky: adot = sigma zdot, addot = sigma zddot  (sigma the slope: what torch's double backward gives)
//   dropout: the (seed, layer, feature, point) mask, scaled by 1 / (1 - p), multiplies all three orders.
// Reverse sweep, per hidden unit, from the output adjoints (A, Adot_i, Addot_p) to the pre-activation ones,
// with S = mask * s:
//   Zddot_p = S Addot_p
//   Zdot_i  = S Adot_i - 2 t S sum_j Addot_{p(i,j)} zdot_j (x2 when j == i: d zdot_i^2 / d zdot_i = 2 zdot_i)
//   Z       = S [A - 2 t sum_i Adot_i zdot_i - sum_p Addot_p (2 t zddot_p + 2 (1 - 3 t^2) zdot_i zdot_j)]
// (d s / dz = -2 t s, d (t s) / dz = s (1 - 3 t^2)); LeakyReLU: every channel Z_c = S A_c.  The linear layer then
// gives dW += sum_c Z_c (x) a_c, db += Z_0 and the input adjoints W^T Z_c, channel by channel.
//
// The sweep needs the pre-activation jets of every hidden layer as well as the post-activation ones, about
// 2 C sum(widths) 4 bytes per point: requests larger than JET2_WS_BUDGET run in point chunks.
#include "common.h"
#include "reduce_adam.h"
#include "residuals.h"

namespace pinn {

namespace {

constexpr int TPB = 256;
constexpr int OB = 8;                          // outputs register-blocked per pass
constexpr int64_t JET2_WS_BUDGET = 1ll << 30;  // workspace bytes above which a call runs in point chunks
constexpr int WG_PTS = 64;
constexpr int64_t WG_CHUNK = 512;              // points per weight-gradient block

template <int K>
struct J2 {
  static constexpr int P = K * (K + 1) / 2;
  static constexpr int C = 1 + K + P;
};

__host__ __device__ constexpr int pair_index(int i, int j, int K) {  // i <= j
  return i * K - i * (i - 1) / 2 + (j - i);
}

struct Drop2 {
  uint32_t thresh;  // 0 = off
  uint32_t seed;
  int layer;
  float scale;      // 1 / (1 - p)
};

__device__ inline float drop_mask(const Drop2& dr, int feature, int64_t point) {
  if (!dr.thresh) return 1.f;
  return dropout_bits(dr.seed, dr.layer, feature, point) >= dr.thresh ? dr.scale : 0.f;
}

// second-order activation of one hidden unit: z[C] pre-activation jets -> out[C] post-activation jets (m = mask)
template <int K>
__device__ inline void act2_fwd(int act, float m, const float (&z)[J2<K>::C], float (&out)[J2<K>::C]) {
  constexpr int C = J2<K>::C;
  if (act == PINN_ACT_TANH) {
    const float t = tanh_f32(z[0]);
    const float S = m * fmaf(-t, t, 1.f);
    out[0] = m * t;
#pragma unroll
    for (int i = 0; i < K; ++i) out[1 + i] = S * z[1 + i];
    const float q = -2.f * t * S;
#pragma unroll
    for (int i = 0; i < K; ++i)
#pragma unroll
      for (int l = i; l < K; ++l) {
        const int c = 1 + K + pair_index(i, l, K);
        out[c] = fmaf(q, z[1 + i] * z[1 + l], S * z[c]);
      }
  } else {
    const float S = m * (z[0] > 0.f ? 1.f : 0.01f);   // nn.LeakyReLU(0.01) dnn.py:21
    out[0] = m * (z[0] > 0.f ? z[0] : 0.01f * z[0]);
#pragma unroll
    for (int c = 1; c < C; ++c) out[c] = S * z[c];
  }
}

// its adjoint: A[C] adjoints of the post-activation jets, z[C] the stored pre-activation jets -> Z[C]
template <int K>
__device__ inline void act2_adj(int act, float m, const float (&A)[J2<K>::C], const float (&z)[J2<K>::C],
                                float (&Z)[J2<K>::C]) {
  constexpr int C = J2<K>::C;
  if (act == PINN_ACT_TANH) {
    const float t = tanh_f32(z[0]);
    const float S = m * fmaf(-t, t, 1.f);
    const float curv = 2.f * fmaf(-3.f * t, t, 1.f);   // 2 (1 - 3 t^2)
    float inner = A[0];
#pragma unroll
    for (int i = 0; i < K; ++i) inner = fmaf(-2.f * t * A[1 + i], z[1 + i], inner);
#pragma unroll
    for (int i = 0; i < K; ++i) {
      float cross = 0.f;   // sum_j Addot_{p(i,j)} zdot_j, the diagonal pair twice
#pragma unroll
      for (int l = 0; l < K; ++l) {
        const int c = 1 + K + (i <= l ? pair_index(i, l, K) : pair_index(l, i, K));
        cross = fmaf(i == l ? 2.f * A[c] : A[c], z[1 + l], cross);
      }
      Z[1 + i] = S * fmaf(-2.f * t, cross, A[1 + i]);
#pragma unroll
      for (int l = i; l < K; ++l) {
        const int c = 1 + K + pair_index(i, l, K);
        inner = fmaf(-A[c], fmaf(2.f * t, z[c], curv * z[1 + i] * z[1 + l]), inner);
        Z[c] = S * A[c];
      }
    }
    Z[0] = S * inner;
  } else {
    const float S = m * (z[0] > 0.f ? 1.f : 0.01f);
#pragma unroll
    for (int c = 0; c < C; ++c) Z[c] = S * A[c];
  }
}

// a0[c][i][n] for the chunk's points n0 + n
template <int K>
__global__ void k2_seed(const float* __restrict__ X, int d_in, int64_t Nc, int64_t n0, int dir0, int dir1, int dir2,
                        float* __restrict__ a0) {
  constexpr int C = J2<K>::C;
  int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= Nc) return;
  const int dirs[3] = {dir0, dir1, dir2};
  for (int i = 0; i < d_in; ++i) {
    a0[(int64_t)i * Nc + n] = X[(n0 + n) * d_in + i];
#pragma unroll
    for (int c = 1; c < C; ++c) a0[((int64_t)c * d_in + i) * Nc + n] = (c <= K && dirs[c - 1] == i) ? 1.f : 0.f;
  }
}

// One linear layer for all C channels; hidden layers also store the pre-activation jets (z_out) and apply the
// second-order activation (a_out).  The output layer writes its z jets to a_out.
template <int K>
__global__ void k2_fwd_layer(const float* __restrict__ Wt, const float* __restrict__ b, int in_dim, int out_dim,
                             const float* __restrict__ a_in, float* __restrict__ z_out, float* __restrict__ a_out,
                             int64_t Nc, int64_t n0, int hidden, int act, Drop2 dr) {
  constexpr int C = J2<K>::C;
  int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= Nc) return;
  for (int o0 = 0; o0 < out_dim; o0 += OB) {
    float acc[C][OB];
#pragma unroll
    for (int j = 0; j < OB; ++j) {
      acc[0][j] = (o0 + j < out_dim) ? b[o0 + j] : 0.f;
#pragma unroll
      for (int c = 1; c < C; ++c) acc[c][j] = 0.f;
    }
    for (int i = 0; i < in_dim; ++i) {
      float av[C];
#pragma unroll
      for (int c = 0; c < C; ++c) av[c] = a_in[((int64_t)c * in_dim + i) * Nc + n];
#pragma unroll
      for (int j = 0; j < OB; ++j) {
        const float w = (o0 + j < out_dim) ? Wt[(int64_t)(o0 + j) * in_dim + i] : 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c][j] = fmaf(w, av[c], acc[c][j]);
      }
    }
#pragma unroll
    for (int j = 0; j < OB; ++j) {
      const int o = o0 + j;
      if (o >= out_dim) break;
      if (!hidden) {
#pragma unroll
        for (int c = 0; c < C; ++c) a_out[((int64_t)c * out_dim + o) * Nc + n] = acc[c][j];
        continue;
      }
#pragma unroll
      for (int c = 0; c < C; ++c) z_out[((int64_t)c * out_dim + o) * Nc + n] = acc[c][j];
      float zj[C], out[C];
#pragma unroll
      for (int c = 0; c < C; ++c) zj[c] = acc[c][j];
      act2_fwd<K>(act, drop_mask(dr, o, n0 + n), zj, out);
#pragma unroll
      for (int c = 0; c < C; ++c) a_out[((int64_t)c * out_dim + o) * Nc + n] = out[c];
    }
  }
}

// g (in/out): on entry the adjoints of this layer's OUTPUT jets; hidden layers turn them into the pre-activation
// adjoints in place (formulas at the top; z_hid = the stored pre-activation jets).  g_in = W^T g, channel by
// channel (skipped when need_gin == 0).
template <int K>
__global__ void k2_bwd_layer(const float* __restrict__ Wt, int in_dim, int out_dim, float* __restrict__ g,
                             const float* __restrict__ z_hid, float* __restrict__ g_in, int64_t Nc, int64_t n0,
                             int hidden, int act, int need_gin, Drop2 dr) {
  constexpr int C = J2<K>::C;
  int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= Nc) return;
  if (hidden) {
    for (int o = 0; o < out_dim; ++o) {
      float A[C], z[C];
#pragma unroll
      for (int c = 0; c < C; ++c) {
        A[c] = g[((int64_t)c * out_dim + o) * Nc + n];
        z[c] = z_hid[((int64_t)c * out_dim + o) * Nc + n];
      }
      float Z[C];
      act2_adj<K>(act, drop_mask(dr, o, n0 + n), A, z, Z);
#pragma unroll
      for (int c = 0; c < C; ++c) g[((int64_t)c * out_dim + o) * Nc + n] = Z[c];
    }
  }
  if (!need_gin) return;
  for (int i0 = 0; i0 < in_dim; i0 += OB) {
    float acc[C][OB];
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
      for (int j = 0; j < OB; ++j) acc[c][j] = 0.f;
    for (int o = 0; o < out_dim; ++o) {
      float zb[C];
#pragma unroll
      for (int c = 0; c < C; ++c) zb[c] = g[((int64_t)c * out_dim + o) * Nc + n];
#pragma unroll
      for (int j = 0; j < OB; ++j) {
        const float w = (i0 + j < in_dim) ? Wt[(int64_t)o * in_dim + i0 + j] : 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c][j] = fmaf(w, zb[c], acc[c][j]);
      }
    }
#pragma unroll
    for (int j = 0; j < OB; ++j) {
      if (i0 + j >= in_dim) break;
#pragma unroll
      for (int c = 0; c < C; ++c) g_in[((int64_t)c * in_dim + i0 + j) * Nc + n] = acc[c][j];
    }
  }
}

// ---- MFMA layer kernels (hidden width <= 64): one wave per 16-point tile, all C channels ----------------------
// v_mfma_f32_16x16x4_f32 with A = W (16 outputs x 4 inputs), B = jets (4 inputs x 16 points), one accumulator tile per
// (channel, 16 outputs).  Lane l supplies A[l & 15][l >> 4] and B[l >> 4][l & 15] and receives D[4 (l >> 4) + r][l & 15]:
// every lane then holds the same (output, point) of every channel, so the second-order activation (and in the backward
// kernel its adjoint, computed where the lane feeds the B operand) runs in registers.  Same workspace layout as above.
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int K, int OT>   // OT = output tiles of 16
__global__ __launch_bounds__(256) void k2m_fwd_layer(const float* __restrict__ Wt, const float* __restrict__ b,
                                                     int in_dim, int out_dim, const float* __restrict__ a_in,
                                                     float* __restrict__ z_out, float* __restrict__ a_out, int64_t Nc,
                                                     int64_t n0, int hidden, int act, Drop2 dr) {
  constexpr int C = J2<K>::C;
  const int lane = threadIdx.x & 63, col = lane & 15, kq = lane >> 4;
  const int64_t nb = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;
  if (nb >= Nc) return;                      // whole wave
  const int64_t n = nb + col;
  const bool nok = n < Nc;
  f32x4 acc[C][OT];
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int t = 0; t < OT; ++t) acc[c][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < in_dim; k0 += 4) {
    const int kk = k0 + kq;
    const bool kok = kk < in_dim;
    float wv[OT], av[C];
#pragma unroll
    for (int t = 0; t < OT; ++t) {
      const int o = t * 16 + col;
      wv[t] = (kok && o < out_dim) ? Wt[(int64_t)o * in_dim + kk] : 0.f;
    }
#pragma unroll
    for (int c = 0; c < C; ++c) av[c] = (kok && nok) ? a_in[((int64_t)c * in_dim + kk) * Nc + n] : 0.f;
#pragma unroll
    for (int t = 0; t < OT; ++t)
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[t], av[c], acc[c][t], 0, 0, 0);
  }
  if (!nok) return;
#pragma unroll
  for (int t = 0; t < OT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int o = t * 16 + 4 * kq + r;
      if (o >= out_dim) continue;
      float zj[C], out[C];
#pragma unroll
      for (int c = 0; c < C; ++c) zj[c] = acc[c][t][r];
      zj[0] += b[o];
      if (!hidden) {
#pragma unroll
        for (int c = 0; c < C; ++c) a_out[((int64_t)c * out_dim + o) * Nc + n] = zj[c];
        continue;
      }
#pragma unroll
      for (int c = 0; c < C; ++c) z_out[((int64_t)c * out_dim + o) * Nc + n] = zj[c];
      act2_fwd<K>(act, drop_mask(dr, o, n0 + n), zj, out);
#pragma unroll
      for (int c = 0; c < C; ++c) a_out[((int64_t)c * out_dim + o) * Nc + n] = out[c];
    }
}

// g: adjoints of the layer's output jets in, pre-activation adjoints out (hidden layers); g_in = W^T g.
// Each lane converts the (output k0 + (l >> 4), point l & 15) element it feeds as the B operand.
template <int K, int IT>   // IT = input tiles of 16
__global__ __launch_bounds__(256) void k2m_bwd_layer(const float* __restrict__ Wt, int in_dim, int out_dim,
                                                     float* __restrict__ g, const float* __restrict__ z_hid,
                                                     float* __restrict__ g_in, int64_t Nc, int64_t n0, int hidden,
                                                     int act, int need_gin, Drop2 dr) {
  constexpr int C = J2<K>::C;
  const int lane = threadIdx.x & 63, col = lane & 15, kq = lane >> 4;
  const int64_t nb = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;
  if (nb >= Nc) return;                      // whole wave
  const int64_t n = nb + col;
  const bool nok = n < Nc;
  f32x4 acc[C][IT];
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int t = 0; t < IT; ++t) acc[c][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < out_dim; k0 += 4) {
    const int o = k0 + kq;
    const bool ok = o < out_dim && nok;
    float Z[C];
#pragma unroll
    for (int c = 0; c < C; ++c) Z[c] = ok ? g[((int64_t)c * out_dim + o) * Nc + n] : 0.f;
    if (hidden && ok) {
      float A[C], z[C];
#pragma unroll
      for (int c = 0; c < C; ++c) { A[c] = Z[c]; z[c] = z_hid[((int64_t)c * out_dim + o) * Nc + n]; }
      act2_adj<K>(act, drop_mask(dr, o, n0 + n), A, z, Z);
#pragma unroll
      for (int c = 0; c < C; ++c) g[((int64_t)c * out_dim + o) * Nc + n] = Z[c];
    }
    if (!need_gin) continue;
#pragma unroll
    for (int t = 0; t < IT; ++t) {
      const int i = t * 16 + col;
      const float w = (o < out_dim && i < in_dim) ? Wt[(int64_t)o * in_dim + i] : 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w, Z[c], acc[c][t], 0, 0, 0);
    }
  }
  if (!need_gin || !nok) return;
#pragma unroll
  for (int t = 0; t < IT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = t * 16 + 4 * kq + r;
      if (i >= in_dim) continue;
#pragma unroll
      for (int c = 0; c < C; ++c) g_in[((int64_t)c * in_dim + i) * Nc + n] = acc[c][t][r];
    }
}

// dW[o][i] += sum_n sum_c zbar[c][o][n] a_in[c][i][n] ; db[o] += sum_n zbar[0][o][n].
// 16x16 threads own a 16x16 tile of dW; grid.z walks WG_CHUNK-point slices; one channel in LDS at a time.
__global__ void k2_wgrad(const float* __restrict__ zb, const float* __restrict__ a_in, int C, int in_dim,
                         int out_dim, int64_t Nc, float* __restrict__ dW, float* __restrict__ db) {
  __shared__ float zs[16][WG_PTS + 1];
  __shared__ float as[16][WG_PTS + 1];
  const int ti = threadIdx.x & 15, to = threadIdx.x >> 4;
  const int o0 = blockIdx.y * 16, i0 = blockIdx.x * 16;
  const int64_t n_begin = (int64_t)blockIdx.z * WG_CHUNK;
  const int64_t n_end = (n_begin + WG_CHUNK < Nc) ? n_begin + WG_CHUNK : Nc;
  float acc = 0.f, accb = 0.f;
  for (int64_t nb = n_begin; nb < n_end; nb += WG_PTS) {
    for (int c = 0; c < C; ++c) {
      for (int e = threadIdx.x; e < 16 * WG_PTS; e += 256) {
        const int p = e % WG_PTS, f = e / WG_PTS;
        const int64_t n = nb + p;
        const bool ok = n < n_end;
        zs[f][p] = (ok && o0 + f < out_dim) ? zb[((int64_t)c * out_dim + o0 + f) * Nc + n] : 0.f;
        as[f][p] = (ok && i0 + f < in_dim) ? a_in[((int64_t)c * in_dim + i0 + f) * Nc + n] : 0.f;
      }
      __syncthreads();
      for (int p = 0; p < WG_PTS; ++p) acc = fmaf(zs[to][p], as[ti][p], acc);
      if (c == 0 && blockIdx.x == 0 && ti == 0)
        for (int p = 0; p < WG_PTS; ++p) accb += zs[to][p];
      __syncthreads();
    }
  }
  if (o0 + to < out_dim && i0 + ti < in_dim) atomicAdd(&dW[(int64_t)(o0 + to) * in_dim + i0 + ti], acc);
  if (blockIdx.x == 0 && ti == 0 && o0 + to < out_dim) atomicAdd(&db[o0 + to], accb);
}

// The same sums on v_mfma_f32_16x16x4_f32 for layers up to 64 x 64 (pinn_residual2_loss_grad's MFMA path):
//   D[16 outputs x 16 inputs] += A[16 outputs x 4 points] B[4 points x 16 inputs],  A = zbar rows, B = a_in rows.
// Points are contiguous in the workspace rows, so lane (m = lane & 15, q = lane >> 4) loads the four points 4q .. 4q + 3 of
// row m with one 16-byte load, for A and for B alike, and feeds element j of both to k-step j: step j contracts points
// {4q' + j}, the four steps together the tile's 16 points, in an order both operands share.  A wave keeps all OT x IT
// accumulator tiles of the layer (at most 16 tiles = 64 registers) plus OT tiles for db (channel 0 against a constant-one
// B operand), walks its slice of the chunk's points over all C channels, and the four waves of a workgroup are summed in
// LDS before ONE float atomicAdd per element and workgroup (the memory-side atomic units are the scarce
// resource).  Atomics: two runs differ in the last bits, like k2_wgrad.
// Rows are Nc floats apart: when Nc % 4 != 0 they are not 16-byte aligned and every element is loaded on its own, under
// its own bound; with Nc % 4 == 0 a group of four lies wholly inside or wholly outside the chunk.  Points past Nc and
// rows past the layer's dimensions enter as exact zeros.
// The slice (points per wave, a multiple of 16) trades parallelism against atomics: k2m_slice() below.
template <int OT, int IT>
__global__ __launch_bounds__(256) void k2m_wgrad(const float* __restrict__ zb, const float* __restrict__ a_in, int C,
                                                 int in_dim, int out_dim, int64_t Nc, int slice,
                                                 float* __restrict__ dW, float* __restrict__ db) {
  constexpr int NTILE = OT * IT + OT;             // dW tiles, then the db tiles
  __shared__ float red[2][NTILE * 4][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, m = lane & 15, q = lane >> 4;
  const int64_t begin = ((int64_t)blockIdx.x * 4 + wave) * slice;
  const int64_t end = begin + slice < Nc ? begin + slice : Nc;
  const bool vec = (Nc & 3) == 0;
  f32x4 acc[NTILE];
#pragma unroll
  for (int t = 0; t < NTILE; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int64_t nb = begin; nb < end; nb += 16) {
    const int64_t n4 = nb + 4 * q;
    for (int c = 0; c < C; ++c) {
      f32x4 za[OT], aa[IT];
#pragma unroll
      for (int t = 0; t < OT; ++t) {
        const int o = t * 16 + m;
        const float* row = zb + ((int64_t)c * out_dim + o) * Nc;
        za[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (o < out_dim) {
          if (vec) {
            if (n4 < Nc) za[t] = *reinterpret_cast<const f32x4*>(row + n4);
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) if (n4 + j < Nc) za[t][j] = row[n4 + j];
          }
        }
      }
#pragma unroll
      for (int t = 0; t < IT; ++t) {
        const int i = t * 16 + m;
        const float* row = a_in + ((int64_t)c * in_dim + i) * Nc;
        aa[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (i < in_dim) {
          if (vec) {
            if (n4 < Nc) aa[t] = *reinterpret_cast<const f32x4*>(row + n4);
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) if (n4 + j < Nc) aa[t][j] = row[n4 + j];
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int to = 0; to < OT; ++to)
#pragma unroll
          for (int ti = 0; ti < IT; ++ti)
            acc[to * IT + ti] = __builtin_amdgcn_mfma_f32_16x16x4f32(za[to][j], aa[ti][j], acc[to * IT + ti], 0, 0, 0);
      if (c == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int to = 0; to < OT; ++to)
            acc[OT * IT + to] = __builtin_amdgcn_mfma_f32_16x16x4f32(za[to][j], 1.f, acc[OT * IT + to], 0, 0, 0);
      }
    }
  }
  // waves 2, 3 -> LDS; waves 0, 1 add them; waves 0, 1 -> LDS; every thread sums the two copies of its elements
  if (wave >= 2) {
#pragma unroll
    for (int t = 0; t < NTILE; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wave - 2][t * 4 + r][lane] = acc[t][r];
  }
  __syncthreads();
  if (wave < 2) {
#pragma unroll
    for (int t = 0; t < NTILE; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[t][r] += red[wave][t * 4 + r][lane];
  }
  __syncthreads();
  if (wave < 2) {
#pragma unroll
    for (int t = 0; t < NTILE; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wave][t * 4 + r][lane] = acc[t][r];
  }
  __syncthreads();
  // element (t, r) of lane (m', q') is D[4 q' + r][m'] of tile t: output to * 16 + 4 q' + r, input ti * 16 + m'
  for (int e = threadIdx.x; e < NTILE * 4 * 64; e += 256) {
    const int l = e & 63, tr = e >> 6, t = tr >> 2, r = tr & 3;
    const int mm = l & 15, qq = l >> 4;
    const float val = red[0][tr][l] + red[1][tr][l];
    if (t < OT * IT) {
      const int o = (t / IT) * 16 + 4 * qq + r, i = (t % IT) * 16 + mm;
      if (o < out_dim && i < in_dim) atomicAdd(&dW[(int64_t)o * in_dim + i], val);
    } else {
      const int o = (t - OT * IT) * 16 + 4 * qq + r;
      if (mm == 0 && o < out_dim) atomicAdd(&db[o], val);
    }
  }
}

// Residual with the lateral-mixing term on the chunk's output jets (pinn_residual2_loss_grad): one thread per point.
struct Res2Params {
  const float* out;     // lo.out: [channel][output column][point of the chunk]
  float* G;             // lo.g0: the adjoint of every channel and output column (written when want_grad)
  float* fields;        // NULL or (NF, N)
  float* partial;       // rows of NT partial sums, one per workgroup; this launch writes rows row0 + blockIdx.x
  const float* scale;   // device term_scale (want_grad)
  int64_t Nc, n0, N, row0;
  int d_out, want_grad;
  int out_col[PINN_MAX_ROLES];
  int dir_ch[PINN_MAX_DIRS];   // channel of direction role d: 1 + spec.dir_of[d]
  int ch_xx, ch_yy;            // channels of the pairs (x, x) and (y, y), x and y as the DESCRIPTOR's direction indices
  float nu;
};

template <class Res, int K>
__global__ __launch_bounds__(TPB) void k2_residual(const Res2Params P) {
  constexpr int C = J2<K>::C, NR = Res::NR, ND = Res::ND, NT = Res::NT, NF = Res::NF;
  typedef Residual2<Res> R2;
  __shared__ float red[NT][TPB];
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  float f[NF];
#pragma unroll
  for (int t = 0; t < NF; ++t) f[t] = 0.f;
  if (n < P.Nc) {
    const int64_t Nc = P.Nc;
    float v[1 + ND][NR], g[1 + ND][NR], lap[2], glap[2];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int o = P.out_col[r];
      v[0][r] = P.out[(int64_t)o * Nc + n];
#pragma unroll
      for (int d = 0; d < ND; ++d) v[1 + d][r] = P.out[((int64_t)P.dir_ch[d] * P.d_out + o) * Nc + n];
    }
    const int ou = P.out_col[Res::RU], ov = P.out_col[Res::RV];
    lap[0] = P.out[((int64_t)P.ch_xx * P.d_out + ou) * Nc + n] + P.out[((int64_t)P.ch_yy * P.d_out + ou) * Nc + n];
    lap[1] = P.out[((int64_t)P.ch_xx * P.d_out + ov) * Nc + n] + P.out[((int64_t)P.ch_yy * P.d_out + ov) * Nc + n];
    R2::fields(v, lap, P.nu, f);      // (once, outside the branch: the same bits with and without a gradient request)
    if (P.want_grad) R2::adjoint(v, f, P.nu, P.scale, g, glap);
    if (P.fields) {
#pragma unroll
      for (int t = 0; t < NF; ++t) P.fields[(int64_t)t * P.N + P.n0 + n] = f[t];
    }
    if (P.want_grad) {
      // columns that carry no role: zeros in every channel
      for (int o = 0; o < P.d_out; ++o) {
        bool has = false;
#pragma unroll
        for (int r = 0; r < NR; ++r) has = has || P.out_col[r] == o;
        if (has) continue;
#pragma unroll
        for (int c = 0; c < C; ++c) P.G[((int64_t)c * P.d_out + o) * Nc + n] = 0.f;
      }
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const int o = P.out_col[r];
        P.G[(int64_t)o * Nc + n] = g[0][r];
#pragma unroll
        for (int i = 0; i < K; ++i) {       // first-order channel 1 + i: the direction role that rides it, if any
          float a = 0.f;
#pragma unroll
          for (int d = 0; d < ND; ++d) if (P.dir_ch[d] == 1 + i) a = g[1 + d][r];
          P.G[((int64_t)(1 + i) * P.d_out + o) * Nc + n] = a;
        }
        const float gl = r == Res::RU ? glap[0] : r == Res::RV ? glap[1] : 0.f;
#pragma unroll
        for (int c = 1 + K; c < C; ++c) {
          float a = 0.f;
          if (c == P.ch_xx) a += gl;
          if (c == P.ch_yy) a += gl;
          P.G[((int64_t)c * P.d_out + o) * Nc + n] = a;
        }
      }
    }
  }
  // per-block partial sums of the squares, in a fixed order
#pragma unroll
  for (int t = 0; t < NT; ++t) red[t][threadIdx.x] = f[t] * f[t];
  __syncthreads();
  for (int s = TPB / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
#pragma unroll
      for (int t = 0; t < NT; ++t) red[t][threadIdx.x] += red[t][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x < NT) P.partial[(P.row0 + blockIdx.x) * NT + threadIdx.x] = red[threadIdx.x][0];
}

// G[c][o][n] of the chunk from row-major gY (N, d_out), gdY (K, N, d_out), gd2Y (P, N, d_out); NULL = 0
template <int K>
__global__ void k2_seed_adjoint(const float* __restrict__ gY, const float* __restrict__ gdY,
                                const float* __restrict__ gd2Y, int d_out, int64_t N, int64_t Nc, int64_t n0,
                                float* __restrict__ G) {
  constexpr int C = J2<K>::C;
  int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= Nc) return;
  const int64_t gn = n0 + n;
  for (int o = 0; o < d_out; ++o) {
    G[(int64_t)o * Nc + n] = gY ? gY[gn * d_out + o] : 0.f;
#pragma unroll
    for (int c = 1; c < C; ++c) {
      const float* src = c <= K ? gdY : gd2Y;
      const int q = c <= K ? c - 1 : c - 1 - K;
      G[((int64_t)c * d_out + o) * Nc + n] = src ? src[((int64_t)q * N + gn) * d_out + o] : 0.f;
    }
  }
}

template <int K>
__global__ void k2_unseed(const float* __restrict__ out, int d_out, int64_t N, int64_t Nc, int64_t n0,
                          float* __restrict__ Y, float* __restrict__ dY, float* __restrict__ d2Y) {
  constexpr int C = J2<K>::C;
  int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= Nc) return;
  const int64_t gn = n0 + n;
  for (int o = 0; o < d_out; ++o) {
    if (Y) Y[gn * d_out + o] = out[(int64_t)o * Nc + n];
#pragma unroll
    for (int c = 1; c < C; ++c) {
      float* dst = c <= K ? dY : d2Y;
      const int q = c <= K ? c - 1 : c - 1 - K;
      if (dst) dst[((int64_t)q * N + gn) * d_out + o] = out[((int64_t)c * d_out + o) * Nc + n];
    }
  }
}

// ---- workspace ---------------------------------------------------------------------
struct Layout2 {
  int64_t Nc;            // points per chunk
  int64_t act_off[1026]; // post-activation jets a_0 .. a_L (a_0 = the seeds)
  int64_t z_off[1026];   // pre-activation jets of hidden layers 0 .. L-1
  int64_t out, g0, g1, total;
};

int64_t layout_for(const Net& n, int C, int64_t Nc, Layout2* lo) {
  const int maxd = n.W > n.d_in ? (n.W > n.d_out ? n.W : n.d_out) : (n.d_in > n.d_out ? n.d_in : n.d_out);
  int64_t off = 0;
  for (int l = 0; l <= n.L; ++l) {
    if (lo) lo->act_off[l] = off;
    off += align256((int64_t)C * (l == 0 ? n.d_in : n.W) * Nc * 4);
  }
  for (int l = 0; l < n.L; ++l) {
    if (lo) lo->z_off[l] = off;
    off += align256((int64_t)C * n.W * Nc * 4);
  }
  if (lo) lo->out = off;
  off += align256((int64_t)C * n.d_out * Nc * 4);
  if (lo) lo->g0 = off;
  off += align256((int64_t)C * maxd * Nc * 4);
  if (lo) lo->g1 = off;
  off += align256((int64_t)C * maxd * Nc * 4);
  if (lo) { lo->total = off; lo->Nc = Nc; }
  return off;
}

int channels(int k) { return 1 + k + k * (k + 1) / 2; }

bool make_layout2(const Net& n, int64_t N, Layout2* lo) {
  if (n.L + 1 > 1025) return false;
  const int C = channels(n.k);
  const int64_t per_pt = layout_for(n, C, 1, nullptr);   // (an upper bound of the per-point bytes)
  int64_t cap = JET2_WS_BUDGET / per_pt;
  cap = cap < 256 ? 256 : (cap / 256) * 256;
  const int64_t Nc = N < cap ? (N > 0 ? N : 1) : cap;
  layout_for(n, C, Nc, lo);
  return true;
}

inline int tiles16(int dim) { return dim <= 16 ? 1 : dim <= 32 ? 2 : 4; }

template <int K>
void run_fwd_chunk(const Net& n, const float* params, const float* X, int64_t n0, char* ws, const Layout2& lo,
                   int64_t Nc, bool mfma, hipStream_t s) {
  const unsigned grid = (unsigned)((Nc + TPB - 1) / TPB);
  hipLaunchKernelGGL(k2_seed<K>, dim3(grid), dim3(TPB), 0, s, X, n.d_in, Nc, n0, n.dir_col[0], n.dir_col[1],
                     n.dir_col[2], (float*)(ws + lo.act_off[0]));
  for (int l = 0; l <= n.L; ++l) {
    const bool hid = l < n.L;
    const Drop2 dr{n.drop_p > 0.f ? n.drop_thresh : 0u, n.drop_seed, l, 1.f / (1.f - n.drop_p)};
    const float* Wl = params + n.w_off(l);
    const float* bl = params + n.b_off(l);
    const float* ain = (const float*)(ws + lo.act_off[l]);
    float* zo = hid ? (float*)(ws + lo.z_off[l]) : nullptr;
    float* ao = (float*)(ws + (hid ? lo.act_off[l + 1] : lo.out));
    if (mfma) {
      const unsigned gm = (unsigned)((Nc + 63) / 64);
      switch (tiles16(n.out_dim(l))) {
        case 1: hipLaunchKernelGGL((k2m_fwd_layer<K, 1>), dim3(gm), dim3(256), 0, s, Wl, bl, n.in_dim(l), n.out_dim(l), ain, zo, ao, Nc, n0, hid ? 1 : 0, n.act, dr); break;
        case 2: hipLaunchKernelGGL((k2m_fwd_layer<K, 2>), dim3(gm), dim3(256), 0, s, Wl, bl, n.in_dim(l), n.out_dim(l), ain, zo, ao, Nc, n0, hid ? 1 : 0, n.act, dr); break;
        default: hipLaunchKernelGGL((k2m_fwd_layer<K, 4>), dim3(gm), dim3(256), 0, s, Wl, bl, n.in_dim(l), n.out_dim(l), ain, zo, ao, Nc, n0, hid ? 1 : 0, n.act, dr); break;
      }
    } else {
      hipLaunchKernelGGL(k2_fwd_layer<K>, dim3(grid), dim3(TPB), 0, s, Wl, bl, n.in_dim(l), n.out_dim(l), ain, zo, ao,
                         Nc, n0, hid ? 1 : 0, n.act, dr);
    }
  }
}

// Points per wave of k2m_wgrad: the chunk spread over about K2M_GROUPS workgroups of four waves, in whole 16-point tiles,
// between 16 and 128.  Measured on MI355X with fixed slices of 16 / 32 / 64 / 128: the 8 x 64 chunk (23 040
// points, 64 MFMAs per tile and channel) wants the shortest slice, 90.6 / 97.5 / 123.4 / 180.1 ms per 2^20-point call — its
// few workgroups leave SIMDs idle long before the atomics count; 10 x 10 at 2^20 points, chunks of about 180 000 (4 MFMAs per tile and
// channel) wants the longest, 17.9 / 12.1 / 9.2 / 8.3 ms — there every workgroup's flush of atomics is the cost.  The rule
// below is a compromise, not an optimum: it gives the 8 x 64 chunk 16 points per wave (its best) and the 10 x 10 chunks
// 48 (9.9 ms where a fixed 128 measured 8.3).
constexpr int64_t K2M_GROUPS = 1024;
inline int k2m_slice(int64_t Nc) {
  const int64_t tiles = (Nc + 4 * K2M_GROUPS * 16 - 1) / (4 * K2M_GROUPS * 16);
  return (int)(tiles < 1 ? 16 : tiles > 8 ? 128 : tiles * 16);
}

// k2m_wgrad for one layer (both dimensions at most 64)
void launch_k2m_wgrad(const float* zb, const float* a_in, int C, int in_dim, int out_dim, int64_t Nc, float* dW,
                      float* db, hipStream_t s) {
  const int slice = k2m_slice(Nc);
  const dim3 grid((unsigned)((Nc + 4 * slice - 1) / (4 * slice))), block(256);
#define K2M_WG(OTv, ITv) \
  hipLaunchKernelGGL((k2m_wgrad<OTv, ITv>), grid, block, 0, s, zb, a_in, C, in_dim, out_dim, Nc, slice, dW, db)
  switch (tiles16(out_dim) * 8 + tiles16(in_dim)) {
    case 1 * 8 + 1: K2M_WG(1, 1); break;
    case 1 * 8 + 2: K2M_WG(1, 2); break;
    case 1 * 8 + 4: K2M_WG(1, 4); break;
    case 2 * 8 + 1: K2M_WG(2, 1); break;
    case 2 * 8 + 2: K2M_WG(2, 2); break;
    case 2 * 8 + 4: K2M_WG(2, 4); break;
    case 4 * 8 + 1: K2M_WG(4, 1); break;
    case 4 * 8 + 2: K2M_WG(4, 2); break;
    default: K2M_WG(4, 4); break;
  }
#undef K2M_WG
}

// mfma_wgrad: the weight gradient on k2m_wgrad instead of k2_wgrad (pinn_residual2_loss_grad's MFMA path only)
template <int K>
void run_bwd_chunk(const Net& n, const float* params, int64_t n0, char* ws, const Layout2& lo, int64_t Nc,
                   float* grad, bool mfma, hipStream_t s, bool mfma_wgrad = false) {
  constexpr int C = J2<K>::C;
  const unsigned grid = (unsigned)((Nc + TPB - 1) / TPB);
  float* gcur = (float*)(ws + lo.g0);
  float* gnext = (float*)(ws + lo.g1);
  for (int l = n.L; l >= 0; --l) {
    const int in_dim = n.in_dim(l), out_dim = n.out_dim(l);
    const bool hid = l < n.L;
    const Drop2 dr{n.drop_p > 0.f ? n.drop_thresh : 0u, n.drop_seed, l, 1.f / (1.f - n.drop_p)};
    const float* Wl = params + n.w_off(l);
    const float* zh = hid ? (const float*)(ws + lo.z_off[l]) : nullptr;
    const int gin = l > 0 ? 1 : 0;
    if (mfma) {
      const unsigned gm = (unsigned)((Nc + 63) / 64);
      switch (tiles16(in_dim)) {
        case 1: hipLaunchKernelGGL((k2m_bwd_layer<K, 1>), dim3(gm), dim3(256), 0, s, Wl, in_dim, out_dim, gcur, zh, gnext, Nc, n0, hid ? 1 : 0, n.act, gin, dr); break;
        case 2: hipLaunchKernelGGL((k2m_bwd_layer<K, 2>), dim3(gm), dim3(256), 0, s, Wl, in_dim, out_dim, gcur, zh, gnext, Nc, n0, hid ? 1 : 0, n.act, gin, dr); break;
        default: hipLaunchKernelGGL((k2m_bwd_layer<K, 4>), dim3(gm), dim3(256), 0, s, Wl, in_dim, out_dim, gcur, zh, gnext, Nc, n0, hid ? 1 : 0, n.act, gin, dr); break;
      }
    } else {
      hipLaunchKernelGGL(k2_bwd_layer<K>, dim3(grid), dim3(TPB), 0, s, Wl, in_dim, out_dim, gcur, zh, gnext, Nc, n0,
                         hid ? 1 : 0, n.act, gin, dr);
    }
    if (mfma_wgrad) {
      launch_k2m_wgrad(gcur, (const float*)(ws + lo.act_off[l]), C, in_dim, out_dim, Nc, grad + n.w_off(l),
                       grad + n.b_off(l), s);
    } else {
      dim3 wg((in_dim + 15) / 16, (out_dim + 15) / 16, (unsigned)((Nc + WG_CHUNK - 1) / WG_CHUNK));
      hipLaunchKernelGGL(k2_wgrad, wg, dim3(256), 0, s, (const float*)gcur, (const float*)(ws + lo.act_off[l]), C,
                         in_dim, out_dim, Nc, grad + n.w_off(l), grad + n.b_off(l));
    }
    float* t = gcur; gcur = gnext; gnext = t;
  }
}

int prep2(const Net& n, int64_t N, int64_t ws_bytes, void* ws, Layout2* lo) {
  if (!make_layout2(n, N, lo)) { set_error("too many layers for the jet2 kernels"); return PINN_ERR_UNSUPPORTED; }
  return check_workspace(ws, ws_bytes, lo->total);
}

}  // namespace

int64_t jet2_workspace_bytes(const Net& n, int64_t N) {
  Layout2 lo;
  if (!make_layout2(n, N > 0 ? N : 1, &lo)) return -1;
  return lo.total;
}

// the MFMA layer kernels serve fp32 networks whose every layer is at most 64 wide, without dropout
bool jet2_mfma_supports(const Net& n) {
  return n.prec == PINN_PREC_F32 && n.drop_p == 0.f && n.W <= 64 && n.d_in <= 64 && n.d_out <= 64 &&
         (n.act == PINN_ACT_TANH || n.act == PINN_ACT_LEAKY_RELU);
}

#define DISPATCH_K(Kv, CALL)                                             \
  switch (Kv) {                                                          \
    case 1: { constexpr int K = 1; CALL; } break;                        \
    case 2: { constexpr int K = 2; CALL; } break;                        \
    case 3: { constexpr int K = 3; CALL; } break;                        \
    default: set_error("jet2 needs 1 <= k <= %d", PINN_MAX_DIRS); return PINN_ERR_INVALID; \
  }

int jet2_forward(const Net& n, bool mfma, const float* params, const float* X, int64_t N, float* Y, float* dY,
                 float* d2Y, void* ws, int64_t ws_bytes, hipStream_t s) {
  Layout2 lo;
  int rc = prep2(n, N, ws_bytes, ws, &lo);
  if (rc) return rc;
  char* w = (char*)ws;
  DISPATCH_K(n.k, {
    for (int64_t n0 = 0; n0 < N; n0 += lo.Nc) {
      const int64_t Nc = N - n0 < lo.Nc ? N - n0 : lo.Nc;
      run_fwd_chunk<K>(n, params, X, n0, w, lo, Nc, mfma, s);
      hipLaunchKernelGGL(k2_unseed<K>, dim3((unsigned)((Nc + TPB - 1) / TPB)), dim3(TPB), 0, s,
                         (const float*)(w + lo.out), n.d_out, N, Nc, n0, Y, dY, d2Y);
    }
  });
  return check_launch(mfma ? "MFMA forward_jet2" : "generic forward_jet2");
}

int jet2_backward(const Net& n, bool mfma, const float* params, const float* X, int64_t N, const float* gY,
                  const float* gdY, const float* gd2Y, float* grad, void* ws, int64_t ws_bytes, hipStream_t s) {
  Layout2 lo;
  int rc = prep2(n, N, ws_bytes, ws, &lo);
  if (rc) return rc;
  char* w = (char*)ws;
  DISPATCH_K(n.k, {
    for (int64_t n0 = 0; n0 < N; n0 += lo.Nc) {
      const int64_t Nc = N - n0 < lo.Nc ? N - n0 : lo.Nc;
      run_fwd_chunk<K>(n, params, X, n0, w, lo, Nc, mfma, s);
      hipLaunchKernelGGL(k2_seed_adjoint<K>, dim3((unsigned)((Nc + TPB - 1) / TPB)), dim3(TPB), 0, s, gY, gdY, gd2Y,
                         n.d_out, N, Nc, n0, (float*)(w + lo.g0));
      run_bwd_chunk<K>(n, params, n0, w, lo, Nc, grad, mfma, s);
    }
  });
  return check_launch(mfma ? "MFMA jet2_backward" : "generic jet2_backward");
}

// ---- pinn_residual2_loss_grad: forward chunk, k2_residual, backward chunk — no unseed, no seed_adjoint, one forward ----
// Workspace: the jet2 layout, then one row of partial sums per k2_residual workgroup of every chunk.
namespace {
constexpr int RES2_NT = 3;
int64_t residual2_rows(int64_t N, int64_t Nc) {   // workgroups of k2_residual over all chunks (a bound when N % Nc != 0)
  const int64_t chunks = (N + Nc - 1) / Nc;
  return chunks * ((Nc + TPB - 1) / TPB);
}

template <class Res, int K>
void run_residual2(const Net& n, const pinn_residual_spec& sp, float nu, const float* scale, const float* params,
                   const float* X, int64_t N, float* fields, float* grad, char* w, const Layout2& lo, float* partial,
                   bool mfma, hipStream_t s, int64_t* rows) {
  Res2Params P;
  P.out = (const float*)(w + lo.out); P.G = (float*)(w + lo.g0); P.fields = fields; P.partial = partial; P.scale = scale;
  P.N = N; P.d_out = n.d_out; P.want_grad = grad ? 1 : 0; P.nu = nu;
  for (int r = 0; r < PINN_MAX_ROLES; ++r) P.out_col[r] = sp.out_col[r];
  for (int d = 0; d < PINN_MAX_DIRS; ++d) P.dir_ch[d] = 1 + sp.dir_of[d];
  const int ix = sp.dir_of[Res::DX], iy = sp.dir_of[Res::DY];
  P.ch_xx = 1 + K + pair_index(ix, ix, K);
  P.ch_yy = 1 + K + pair_index(iy, iy, K);
  int64_t row0 = 0;
  for (int64_t n0 = 0; n0 < N; n0 += lo.Nc) {
    const int64_t Nc = N - n0 < lo.Nc ? N - n0 : lo.Nc;
    const unsigned grid = (unsigned)((Nc + TPB - 1) / TPB);
    run_fwd_chunk<K>(n, params, X, n0, w, lo, Nc, mfma, s);
    P.Nc = Nc; P.n0 = n0; P.row0 = row0;
    hipLaunchKernelGGL((k2_residual<Res, K>), dim3(grid), dim3(TPB), 0, s, P);
    row0 += grid;
    if (grad) run_bwd_chunk<K>(n, params, n0, w, lo, Nc, grad, mfma, s, mfma);
  }
  *rows = row0;
}
}  // namespace

int64_t residual2_workspace_bytes(const Net& n, int64_t N) {
  Layout2 lo;
  const int64_t Np = N > 0 ? N : 1;
  if (!make_layout2(n, Np, &lo)) return -1;
  return lo.total + align256(residual2_rows(Np, lo.Nc) * RES2_NT * 4);
}

// spec: normalised (check_spec), a residual with a momentum equation, n.k == its number of directions
int residual2_loss_grad(const Net& n, bool mfma, const pinn_residual_spec& spec, float nu, const float* scale,
                        const float* params, const float* X, int64_t N, float* sums, float* fields, float* grad,
                        void* ws, int64_t ws_bytes, hipStream_t s) {
  Layout2 lo;
  if (!make_layout2(n, N, &lo)) { set_error("too many layers for the jet2 kernels"); return PINN_ERR_UNSUPPORTED; }
  const int64_t need = lo.total + align256(residual2_rows(N, lo.Nc) * RES2_NT * 4);
  if (int rc = check_workspace(ws, ws_bytes, need)) return rc;
  char* w = (char*)ws;
  float* partial = (float*)(w + lo.total);
  int64_t rows = 0;
  switch (spec.residual_id) {
    case PINN_RES_NAVIER_STOKES:
      run_residual2<Res2NavierStokes, 3>(n, spec, nu, scale, params, X, N, fields, grad, w, lo, partial, mfma, s, &rows);
      break;
    case PINN_RES_PHYSICS_EQUATION:
      run_residual2<Res2PhysicsEquation, 2>(n, spec, nu, scale, params, X, N, fields, grad, w, lo, partial, mfma, s, &rows);
      break;
    case RES_PE_CORRECTED:
      run_residual2<Res2PhysicsEquationCorrected, 2>(n, spec, nu, scale, params, X, N, fields, grad, w, lo, partial, mfma, s, &rows);
      break;
    default: set_error("residual %d has no second-order term", spec.residual_id); return PINN_ERR_UNSUPPORTED;
  }
  reduce_sums(partial, rows, RES2_NT, 0, RES2_NT, sums, s);
  return check_launch(mfma ? "MFMA residual2_loss_grad" : "generic residual2_loss_grad");
}

}  // namespace pinn
