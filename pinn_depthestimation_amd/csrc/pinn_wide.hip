// pinn_wide.hip — host side of the wide MFMA engine (64 < W <= 256): workspace layout, weight packing, the chunked point
// loop, and per chunk the launch sequence of fp32 mode (one launch per layer and direction, wide_kernel.h) or of bf16
// mode (the chain kernels, chain_kernel.h, with the thin first / last layers around them).  The kernels' instances and
// their launchers: pinn_wide_units.hip, pinn_chain_units.hip (wide_launch.h).
#include "wide_launch.h"
#include "reduce_adam.h"

namespace pinn {

namespace {

int wide_padded_width(int W) { return W <= 128 ? 128 : 256; }

// the shapes the engine's kernels are built for (wide_supports adds what only a launch needs)
bool wide_shape(const Net& n) {
  return n.act == PINN_ACT_TANH && n.W > 64 && n.W <= 256 && n.d_in <= 16 && n.d_out <= 16;
}

struct WGeo { int WP, NTW, PW, PB; };
WGeo wgeo(const Net& n) {
  WGeo g;
  g.WP = wide_padded_width(n.W); g.NTW = g.WP / 16;
  g.PW = g.WP * 16 + (n.L - 1) * g.WP * g.WP + 16 * g.WP;
  g.PB = n.L * g.WP + 16;
  return g;
}
// bytes between the 1 KB pieces of a packed weight slab (k_chain_pack): all slabs' piece i, rounded up to 64 KB, + 4 KB
int64_t chain_plane_bytes(int nh, int NTW) {
  const int64_t slabs = (int64_t)(nh > 0 ? nh : 1) * NTW * 1024;
  return ((slabs + 65535) / 65536) * 65536 + 4096;
}

int cus() { return device_cu_count(); }

// workgroups for `tiles` point tiles at `per_wg` tiles per workgroup and pass, `cap` at the most
int clamp_grid(int64_t tiles, int per_wg, int64_t cap) {
  const int64_t want = (tiles + per_wg - 1) / per_wg;
  return (int)(want < cap ? want : cap);
}

// bf16 mode's output-layer kernel (k_chain_last_fwd: three waves per SIMD fit) runs up to three workgroups per CU, each
// with its own row of loss partial sums
constexpr int SUM_ROWS_PER_CU = 3;
constexpr int64_t ACT_BUDGET_BYTES = (int64_t)6 << 30;   // activation workspace per chunk (fp32 mode)
// bf16 mode (chain kernels): 2L + 1 bf16 jets per chunk, and the weight-gradient kernel flushes its registers
// once per chunk and workgroup — chunks are as large as a 288 GB part comfortably allows
constexpr int64_t CHAIN_BUDGET_BYTES = (int64_t)56 << 30;

struct WLayout {
  int64_t chunk_pts, chunk_tiles, n_chunks;
  int64_t wp, wtp, bp, act, act_stride, gA, gB, gout, sums, total;
  int64_t wf, wtf, jA, jZ, jGL, jG1, jet_stride;   // bf16 mode: packed fragments, chain-layout jets (byte offsets; jet_stride in bytes)
  int grid;
};
WLayout wlayout(const Net& n, const WGeo& g, int64_t N) {
  WLayout w;
  const int K1 = 1 + PINN_MAX_DIRS;
  const bool chain = n.prec == PINN_PREC_BF16;
  // fp32 mode: L jets + 2 adjoint buffers, fp32.  bf16 mode: a_1..a_L, zbar_1..zbar_{L-1}, abar_L, abar_1 in bf16.
  const int64_t per_pt = chain ? (int64_t)K1 * g.WP * 2 * (2 * n.L + 1) + (int64_t)K1 * 16 * 4
                               : (int64_t)K1 * g.WP * 4 * (n.L + 2) + (int64_t)K1 * 16 * 4;
  // whole number of tiles per wave in every full chunk (no tail imbalance): multiple of waves * 16 points
  const int64_t quantum = (int64_t)cus() * WIDE_WAVES * 16;
  int64_t cp = (chain ? CHAIN_BUDGET_BYTES : ACT_BUDGET_BYTES) / per_pt;
  cp = (cp / quantum) * quantum;
  if (cp < quantum) cp = quantum;
  const int64_t npad = ((N + 15) / 16) * 16;
  if (cp > npad) cp = npad;
  w.chunk_pts = cp; w.chunk_tiles = cp / 16; w.n_chunks = (npad + cp - 1) / cp;
  w.grid = cus();
  int64_t off = 0;
  w.wp = off; off += align256((int64_t)g.PW * 4);
  w.wtp = off; off += align256((int64_t)g.PW * 4);
  w.bp = off; off += align256((int64_t)g.PB * 4);
  w.act_stride = align256(w.chunk_tiles * K1 * g.NTW * 256 * 4);
  w.act = w.gA = w.gB = 0;
  w.wf = w.wtf = w.jA = w.jZ = w.jGL = w.jG1 = w.jet_stride = 0;
  if (!chain) {
    w.act = off; off += w.act_stride * n.L;
    w.gA = off; off += w.act_stride;
    w.gB = off; off += w.act_stride;
  } else {
    const int64_t frag = chain_plane_bytes(n.L - 1, g.NTW) * g.NTW;          // hi + lo bf16 per hidden matrix: 2 NS = NTW piece planes
    w.wf = off; off += frag;
    w.wtf = off; off += frag;
    w.jet_stride = align256(w.chunk_tiles * K1 * g.NTW * 256 * 2);
    w.jA = off; off += w.jet_stride * n.L;
    w.jZ = off; off += w.jet_stride * (n.L > 1 ? n.L - 1 : 0);
    w.jGL = off; off += w.jet_stride;
    if (n.L > 1) { w.jG1 = off; off += w.jet_stride; }
    else w.jG1 = w.jGL;                                  // no hidden matrix: abar_1 is abar_L
  }
  w.gout = off; off += align256(w.chunk_tiles * K1 * 256 * 4);
  w.sums = off; off += align256(w.n_chunks * SUM_ROWS_PER_CU * w.grid * MAX_SUMS * 4);   // one row of loss partials per workgroup
  w.total = off;
  return w;
}

__global__ void k_wide_pack(Net n, int WP, const float* __restrict__ params, float* __restrict__ Wp,
                            float* __restrict__ WTp, float* __restrict__ Bp, int PW, int PB) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < PW) {
    int l, rem;
    if (i < WP * 16) { l = 0; rem = i; }
    else { const int j = i - WP * 16; l = 1 + j / (WP * WP); rem = j % (WP * WP); if (l > n.L) l = n.L; }
    const int inP = (l == 0) ? 16 : WP, outP = (l == n.L) ? 16 : WP;
    const int in_d = n.in_dim(l), out_d = n.out_dim(l);
    const int base = i - rem;
    { const int o = rem / inP, c = rem % inP;
      const float v = (o < out_d && c < in_d) ? params[n.w_off(l) + (int64_t)o * in_d + c] : 0.f;
      Wp[i] = v; }
    { const int c = rem / outP, o = rem % outP;
      const float v = (o < out_d && c < in_d) ? params[n.w_off(l) + (int64_t)o * in_d + c] : 0.f;
      WTp[base + rem] = v; }
  }
  if (i < PB) {
    int l = i / WP, o = i % WP;
    if (l >= n.L) { l = n.L; o = i - n.L * WP; }
    Bp[i] = (o < n.out_dim(l)) ? params[n.b_off(l) + o] : 0.f;
  }
}

// Hidden matrices W_1 .. W_{L-1} -> MFMA fragment order for the chain kernels (chain_kernel.h), hi + lo bf16:
//   Wf [li][MT][hl][s][lane][j] = W_l[16 MT + m][n(s, qk, j)]        (forward: rows = output units)
//   WTf[li][MT][hl][s][lane][j] = W_l[n(s, qk, j)][16 MT + m]        (reverse: rows = input units)
// lane = (m = lane & 15, qk = lane >> 4), n(s, qk, j) = 32 s + 16 (j >> 2) + 4 qk + (j & 3): the k index is
// permuted inside each k-step so that two accumulator tiles are the next B operand as they stand.
// A slab (li, MT) is 2 NS pieces of 1 KB ([hi | lo][k-step]); piece i of slab n is stored at element
// i * plane + n * 512: the pieces of one slab are `plane` apart (a multiple of 64 KB plus 4 KB, chain_plane_bytes), so
// that the 32 CUs of an XCD, which read the same slab at about the same time, spread over the L2's channels
// instead of queueing on the few that one contiguous 16 KB region maps to.
__global__ void k_chain_pack(Net n, int NTW, int64_t plane, const float* __restrict__ params, unsigned short* __restrict__ Wf,
                             unsigned short* __restrict__ WTf) {
  const int NS = NTW / 2;
  const int64_t per_layer = (int64_t)NTW * NS * 512;            // (MT, s, lane, j) combinations
  const int64_t total = (int64_t)(n.L - 1) * per_layer;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int li = (int)(e / per_layer);
  int64_t r = e % per_layer;
  const int MT = (int)(r / (NS * 512)); r %= NS * 512;
  const int s = (int)(r / 512); r %= 512;
  const int lane = (int)(r / 8), j = (int)(r % 8);
  const int m = lane & 15, qk = lane >> 4;
  const int row = 16 * MT + m, kk = 32 * s + 16 * (j >> 2) + 4 * qk + (j & 3);
  const int W = n.W;
  const float* Wl = params + n.w_off(li + 1);
  const bool in = row < W && kk < W;
  const float wf = in ? Wl[(int64_t)row * W + kk] : 0.f;
  const float wt = in ? Wl[(int64_t)kk * W + row] : 0.f;
  const int64_t slab = ((int64_t)li * NTW + MT) * 512;
  const int64_t o_hi = (int64_t)s * plane + slab + lane * 8 + j, o_lo = o_hi + (int64_t)NS * plane;
  const __bf16 fh = (__bf16)wf, th = (__bf16)wt;
  Wf[o_hi] = __builtin_bit_cast(unsigned short, fh);
  Wf[o_lo] = __builtin_bit_cast(unsigned short, (__bf16)(wf - (float)fh));
  WTf[o_hi] = __builtin_bit_cast(unsigned short, th);
  WTf[o_lo] = __builtin_bit_cast(unsigned short, (__bf16)(wt - (float)th));
}

// what the chunks of one call share
struct WideCall {
  const Net& n;
  const WGeo& g;
  const WLayout& w;
  char* base;                 // the workspace
  bool grad;
  const LossReq* rq;
  hipStream_t s;
  FusedParams P;
  const float* Wp;            // packed weights, their transposes, biases (k_wide_pack)
  const float* WTp;
  const float* Bp;
  float* gout;                // the output adjoint G of the chunk
  int woff(int l) const { return l == 0 ? 0 : g.WP * 16 + (l - 1) * g.WP * g.WP; }   // layer l inside Wp / WTp
  int nh() const { return n.L - 1; }                                                   // hidden (W x W) matrices
};

template <int NTW>
void pack_weights(const WideCall& c, const float* params) {
  const WGeo& g = c.g;
  const WLayout& w = c.w;
  const int packN = g.PW > g.PB ? g.PW : g.PB;
  hipLaunchKernelGGL(k_wide_pack, dim3((packN + 255) / 256), dim3(256), 0, c.s, c.n, g.WP, params, (float*)(c.base + w.wp),
                     (float*)(c.base + w.wtp), (float*)(c.base + w.bp), g.PW, g.PB);
  if (c.n.prec == PINN_PREC_BF16 && c.nh() > 0) {
    const int64_t total = (int64_t)c.nh() * NTW * (NTW / 2) * 512;
    hipLaunchKernelGGL(k_chain_pack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c.s, c.n, NTW, chain_plane_bytes(c.nh(), NTW) / 2, params,
                       (unsigned short*)(c.base + w.wf), (unsigned short*)(c.base + w.wtf));
  }
}

// ---- fp32 mode: one chunk, one launch per layer and direction.  Lp arrives with the chunk's tiles and sum rows set. ----
template <int NTW>
int fp32_chunk(const WideCall& c, WideLayer Lp, int grid) {
  const Net& n = c.n;
  const WLayout& w = c.w;
  const FusedParams& P = c.P;
  hipStream_t s = c.s;
  const int K1 = n.K1, L = n.L, WP = c.g.WP;
  auto act_l = [&](int l) { return (float*)(c.base + w.act + (int64_t)(l - 1) * w.act_stride); };   // a_l, l = 1..L
  // ---- forward ----
  Lp.W = c.Wp; Lp.b = c.Bp; Lp.out_act = act_l(1);
  if (int rc = launch_wide_fwd<NTW>(WIDE_FIRST, K1, false, P, Lp, grid, s)) return rc;
  for (int l = 1; l < L; ++l) {
    Lp.W = c.Wp + c.woff(l); Lp.b = c.Bp + l * WP; Lp.in_act = act_l(l); Lp.out_act = act_l(l + 1);
    if (int rc = launch_wide_fwd<NTW>(WIDE_HIDDEN, K1, false, P, Lp, grid, s)) return rc;
  }
  Lp.W = c.Wp + c.woff(L); Lp.b = c.Bp + L * WP; Lp.in_act = act_l(L); Lp.out_act = nullptr; Lp.g_out = c.gout;
  if (int rc = launch_wide_fwd<NTW>(WIDE_LAST, K1, c.grad, P, Lp, grid, s)) return rc;
  if (!c.grad) return PINN_OK;
  // ---- reverse sweep (weight gradients: row blocks are waves of a workgroup, one workgroup per CU) ----
  float* grad = c.rq->grad;
  // output layer: dW_L = G . a_L^T ; abar_L = W_L^T G
  Lp.g_in = c.gout; Lp.in_act = act_l(L); Lp.in_d = n.in_dim(L); Lp.out_d = n.out_dim(L);
  Lp.dW = grad + n.w_off(L); Lp.db = grad + n.b_off(L);
  if (int rc = launch_wide_wgrad<NTW>(WIDE_LAST, K1, P, Lp, w.grid, s)) return rc;
  float* gcur = (float*)(c.base + w.gA);
  float* gnext = (float*)(c.base + w.gB);
  Lp.W = c.WTp + c.woff(L); Lp.g_out = gcur;
  if (int rc = launch_wide_bwd<NTW>(WIDE_LAST, K1, P, Lp, grid, s)) return rc;
  for (int l = L - 1; l >= 1; --l) {
    // zbar_l (in place over gcur: one wave per tile) and abar_l = W_l^T zbar_l
    Lp.W = c.WTp + c.woff(l); Lp.g_in = gcur; Lp.in_act = act_l(l + 1); Lp.g_out = gnext;
    if (int rc = launch_wide_bwd<NTW>(WIDE_HIDDEN, K1, P, Lp, grid, s)) return rc;
    Lp.g_in = gcur; Lp.in_act = act_l(l); Lp.in_d = n.in_dim(l); Lp.out_d = n.out_dim(l);
    Lp.dW = grad + n.w_off(l); Lp.db = grad + n.b_off(l);
    if (int rc = launch_wide_wgrad<NTW>(WIDE_HIDDEN, K1, P, Lp, w.grid, s)) return rc;
    float* t = gcur; gcur = gnext; gnext = t;
  }
  Lp.g_in = gcur; Lp.in_act = act_l(1); Lp.g_out = nullptr; Lp.W = nullptr;
  if (int rc = launch_wide_bwd<NTW>(WIDE_FIRST, K1, P, Lp, grid, s)) return rc;
  Lp.g_in = gcur; Lp.in_act = nullptr; Lp.in_d = n.in_dim(0); Lp.out_d = n.out_dim(0);
  Lp.dW = grad + n.w_off(0); Lp.db = grad + n.b_off(0);
  return launch_wide_wgrad<NTW>(WIDE_FIRST, K1, P, Lp, w.grid, s);
}

// ---- diagnostic build only (-DPINN_CHAIN_DIAG, tools/chain_diag.sh; never shipped): the chain kernels' per-phase cycle sums ----
#ifdef PINN_CHAIN_DIAG
unsigned long long* diag_slot(int kernel) {     // 3 kernels x 8 phase sums, then the 8-wave kernels' late wave
  static unsigned long long* dbuf = nullptr;
  if (!dbuf) { (void)hipMalloc((void**)&dbuf, 48 * sizeof(unsigned long long)); }
  return dbuf + 8 * kernel;
}
void diag_report_forward(hipStream_t s) {
  unsigned long long h[8];
  (void)hipStreamSynchronize(s);
  (void)hipMemcpy(h, diag_slot(0), sizeof(h), hipMemcpyDeviceToHost);
  unsigned long long tot = 0; for (int i = 0; i < 8; ++i) tot += h[i];
  fprintf(stderr, "CHAIN_DIAG fwd (no spill): wait_dma %.1f%% barrier %.1f%% step %.1f%% act %.1f%% tile-io %.1f%% | total %llu cycles\n",
          100.0 * h[0] / tot, 100.0 * h[1] / tot, 100.0 * h[2] / tot, 100.0 * h[3] / tot, 100.0 * h[4] / tot, tot);
}
void diag_report_step(hipStream_t s) {
  unsigned long long h[48];
  (void)hipStreamSynchronize(s);
  (void)hipMemcpy(h, diag_slot(0), sizeof(h), hipMemcpyDeviceToHost);
  for (int k8 = 0; k8 < 2; ++k8) {
    const unsigned long long* d = h + (k8 == 0 ? 0 : 24);
    unsigned long long tot = 0; for (int i = 0; i < 8; ++i) tot += d[i];
    fprintf(stderr, "CHAIN_DIAG %s %s wave: wait %.1f%% barrier %.1f%% reads+mfma %.1f%% act %.1f%% copies+stores %.1f%% other %.1f%% tile-io %.1f%% | total %llu cycles\n",
            k8 < 2 ? "fwd8" : "bwd8", (k8 & 1) ? "late" : "early", 100.0 * d[0] / tot, 100.0 * d[1] / tot, 100.0 * d[2] / tot, 100.0 * d[3] / tot, 100.0 * d[4] / tot, 100.0 * d[5] / tot, 100.0 * d[6] / tot, tot);
  }
  const char* nm[3] = {"fwd", "bwd", "wgrad"};
  for (int k = 0; k < 3; ++k) {
    unsigned long long tot = 0; for (int i = 0; i < 8; ++i) tot += h[8 * k + i];
    fprintf(stderr, "CHAIN_DIAG %s: wait_dma %.1f%% barrier %.1f%% step(issue+lds+mfma) %.1f%% act/adjoint %.1f%% tile-io %.1f%% | total %llu cycles\n", nm[k],
            100.0 * h[8 * k] / tot, 100.0 * h[8 * k + 1] / tot, 100.0 * h[8 * k + 2] / tot, 100.0 * h[8 * k + 3] / tot, 100.0 * h[8 * k + 4] / tot, tot);
  }
}
#else
unsigned long long* diag_slot(int) { return nullptr; }
void diag_report_forward(hipStream_t) {}
void diag_report_step(hipStream_t) {}
#endif

// the chain kernels' arguments for one chunk: everything but the per-kernel diagnostic slot and the slice count
template <int NTW>
ChainParams chain_params(const WideCall& c, const WideLayer& Lp) {
  const Net& n = c.n;
  const WLayout& w = c.w;
  ChainParams C;
  memset(&C, 0, sizeof(C));
  C.L = n.L; C.n_tiles = Lp.n_tiles; C.jet_stride = w.jet_stride / 2; C.w_plane = chain_plane_bytes(c.nh(), NTW);
  C.Wf = (const unsigned short*)(c.base + w.wf); C.WTf = (const unsigned short*)(c.base + w.wtf); C.bias = c.Bp;
  C.A = (unsigned short*)(c.base + w.jA); C.Z = (unsigned short*)(c.base + w.jZ);
  C.GL = (unsigned short*)(c.base + w.jGL); C.G1 = (unsigned short*)(c.base + w.jG1);
  C.dW = c.grad ? c.rq->grad : nullptr; C.spill = c.grad ? 1 : 0; C.W = n.W;
  C.w_off1 = n.w_off(1); C.w_per = (int64_t)n.W * n.W + n.W;
  C.X = c.P.X; C.W0 = c.Wp; C.n_points = c.P.N; C.tile0 = Lp.tile0; C.d_in = n.d_in;
  for (int j = 0; j < 3; ++j) C.dir_col[j] = j < n.k ? n.dir_col[j] : 0;
  return C;
}

// ---- bf16 mode: one chunk.  The L - 1 hidden matrices on the three chain kernels (chain_kernel.h); the first layer
// folded into the forward chain kernel and k_chain_first_bwd when d_in <= 3 (every network of the reference), the last
// layer on k_chain_last_fwd and, when d_out <= 4, k_chain_last_bwd; otherwise the thin layers on the per-layer kernels
// (fp32 MFMA on the thin matrices, chain-layout bf16 jets).  Lp arrives with the chunk's tiles and sum rows set. ----
template <int NTW>
int bf16_chunk(const WideCall& c, WideLayer Lp, int grid) {
  const Net& n = c.n;
  const WLayout& w = c.w;
  const FusedParams& P = c.P;
  hipStream_t s = c.s;
  const int K1 = n.K1, L = n.L, nh = c.nh();
  ChainParams C = chain_params<NTW>(c, Lp);
  auto jetA = [&](int l) { return (float*)(c.base + w.jA + (int64_t)(l - 1) * w.jet_stride); };   // a_l, l = 1..L
  const int cgrid = clamp_grid(Lp.n_tiles, CHAIN_WAVES, w.grid);
  const int stream_grid = clamp_grid(Lp.n_tiles, CHAIN_WAVES, 8 * (int64_t)w.grid);   // the two streaming thin-layer kernels
  const bool fold_first = nh > 0 && n.d_in <= 3;
  // ---- forward ----
  Lp.W = c.Wp; Lp.b = c.Bp; Lp.out_act = jetA(1);
  if (!fold_first) { if (int rc = launch_wide_thin<NTW>(THIN_FIRST_FWD, K1, P, Lp, grid, s)) return rc; }
  C.diag = diag_slot(0);
  if (nh > 0) { if (int rc = launch_chain_fwd8<NTW>(K1, fold_first, C, cgrid, s)) return rc; }
  Lp.W = c.Wp + c.woff(L); Lp.b = c.Bp + L * c.g.WP; Lp.in_act = jetA(L); Lp.out_act = nullptr; Lp.g_out = c.gout;
  if (int rc = launch_chain_last_fwd<NTW>(K1, c.grad, P, Lp, clamp_grid(Lp.n_tiles, WIDE_WAVES, (int64_t)SUM_ROWS_PER_CU * w.grid), s)) return rc;
  if (!c.grad) {
    if (nh > 0) diag_report_forward(s);
    return PINN_OK;
  }
  // ---- reverse sweep ----
  float* grad = c.rq->grad;
  // output layer: dW_L = G . a_L^T ; abar_L = W_L^T G (bf16, chain layout) — one streaming kernel when d_out <= 4
  if (n.d_out <= 4) {
    ChainParams F = C;
    F.A = (unsigned short*)jetA(L); F.gout = c.gout; F.WLT = c.WTp + c.woff(L); F.dWL = grad + n.w_off(L); F.d_out = n.d_out;
    if (int rc = launch_chain_last_bwd<NTW>(K1, F, stream_grid, s)) return rc;
  } else {
    Lp.g_in = c.gout; Lp.in_act = jetA(L); Lp.in_d = n.in_dim(L); Lp.out_d = n.out_dim(L);
    Lp.dW = grad + n.w_off(L); Lp.db = grad + n.b_off(L);
    if (int rc = launch_wide_thin<NTW>(THIN_LAST_WGRAD, K1, P, Lp, w.grid, s)) return rc;
    Lp.W = c.WTp + c.woff(L); Lp.g_out = (float*)C.GL;
    if (int rc = launch_wide_thin<NTW>(THIN_LAST_BWD, K1, P, Lp, grid, s)) return rc;
  }
  C.diag = diag_slot(1);
  if (nh > 0) { if (int rc = launch_chain_bwd<NTW>(K1, C, cgrid, s)) return rc; }
  if (fold_first) {
    // first layer: zbar_0 = adjoint(abar_1, a_1) and dW_0, db_0 in one streaming pass (k_chain_first_bwd)
    ChainParams F = C;
    F.A = (unsigned short*)jetA(1); F.dW = grad;
    if (int rc = launch_chain_first_bwd<NTW>(K1, F, stream_grid, s)) return rc;
  } else {
    // first layer: zbar_0 = adjoint(abar_1, a_1), in place over abar_1; dW_0 = zbar_0 . (x, e_j)^T
    Lp.g_in = (float*)C.G1; Lp.in_act = jetA(1); Lp.g_out = nullptr; Lp.W = nullptr;
    if (int rc = launch_wide_thin<NTW>(THIN_FIRST_BWD, K1, P, Lp, grid, s)) return rc;
    Lp.g_in = (float*)C.G1; Lp.in_act = nullptr; Lp.in_d = n.in_dim(0); Lp.out_d = n.out_dim(0);
    Lp.dW = grad + n.w_off(0); Lp.db = grad + n.b_off(0);
    if (int rc = launch_wide_thin<NTW>(THIN_FIRST_WGRAD, K1, P, Lp, w.grid, s)) return rc;
  }
  if (nh > 0) {
    // hidden weight gradients: a workgroup per (layer, slice of the points)
    C.n_slices = w.grid / nh > 0 ? w.grid / nh : 1;
    if ((int64_t)C.n_slices > Lp.n_tiles) C.n_slices = (int)Lp.n_tiles;
    C.diag = diag_slot(2);
    if (int rc = launch_chain_wgrad8<NTW>(K1, C, C.n_slices * nh, s)) return rc;
    diag_report_step(s);
  }
  return PINN_OK;
}

// pack the weights, then chunk by chunk: zero the chunk's partial-sum rows, run it; reduce the rows at the end
template <int NTW>
int run_w(const Net& n, const WGeo& g, bool grad, const LossReq* rq, const float* params, const float* X, int64_t N,
          float* Y, float* dY, char* base, const WLayout& w, hipStream_t s) {
  WideCall c{n, g, w, base, grad, rq, s};
  FusedParams& P = c.P;
  memset(&P, 0, sizeof(P));
  P.d_in = n.d_in; P.d_out = n.d_out; P.L = n.L; P.act = n.act;
  for (int j = 0; j < PINN_MAX_DIRS; ++j) P.dir_col[j] = n.dir_col[j];
  P.N = N; P.X = X; P.Y = Y; P.dY = dY;
  P.n_split = -1;
  P.wg_sums = (float*)(base + w.sums);
  if (rq) set_loss(P, n, *rq);
  c.Wp = (const float*)(base + w.wp);
  c.WTp = (const float*)(base + w.wtp);
  c.Bp = (const float*)(base + w.bp);
  c.gout = (float*)(base + w.gout);
  pack_weights<NTW>(c, params);
  const int64_t total_tiles = (N + 15) / 16;
  const int64_t sum_rows = (int64_t)SUM_ROWS_PER_CU * w.grid;     // per chunk
  for (int64_t ch = 0; ch < w.n_chunks; ++ch) {
    WideLayer Lp;
    memset(&Lp, 0, sizeof(Lp));
    Lp.tile0 = ch * w.chunk_tiles;
    Lp.n_tiles = total_tiles - Lp.tile0 < w.chunk_tiles ? total_tiles - Lp.tile0 : w.chunk_tiles;
    if (Lp.n_tiles <= 0) break;
    Lp.sums_slot = (int)(ch * sum_rows);
    // zero this chunk's rows of the partial-sum table (a smaller grid leaves rows untouched)
    if (hipMemsetAsync(P.wg_sums + (int64_t)Lp.sums_slot * MAX_SUMS, 0, (size_t)sum_rows * MAX_SUMS * 4, s) != hipSuccess) {
      set_error("hipMemsetAsync failed"); return PINN_ERR_LAUNCH;
    }
    const int grid = clamp_grid(Lp.n_tiles, WIDE_WAVES, w.grid);
    if (int rc = n.prec == PINN_PREC_BF16 ? bf16_chunk<NTW>(c, Lp, grid) : fp32_chunk<NTW>(c, Lp, grid)) return rc;
  }
  if (rq) {
    if (P.loss_kind & 1) reduce_sums(P.wg_sums, w.n_chunks * sum_rows, MAX_SUMS, 0, rq->n_terms, rq->sums, s);
    if (P.loss_kind & 2) reduce_sums(P.wg_sums, w.n_chunks * sum_rows, MAX_SUMS, MSE_SUM0, rq->n_cols, rq->mse_sums, s);
  }
  return check_launch("wide reductions");
}

int run(const Net& n, bool grad, const LossReq* rq, const float* params, const float* X, int64_t N, float* Y,
        float* dY, void* ws, int64_t ws_bytes, hipStream_t s) {
  const WGeo g = wgeo(n);
  const WLayout w = wlayout(n, g, N);
  if (int rc = check_workspace(ws, ws_bytes, w.total)) return rc;
  return g.NTW == 8 ? run_w<8>(n, g, grad, rq, params, X, N, Y, dY, (char*)ws, w, s)
                    : run_w<16>(n, g, grad, rq, params, X, N, Y, dY, (char*)ws, w, s);
}

}  // namespace

bool wide_supports(const Net& n) {
  // bf16 mode: k_chain_fwd8 keeps every layer's bias in LDS behind its weight ring; the depth limit is its LDS formula
  if (n.prec == PINN_PREC_BF16 && chain_fwd8_lds_bytes(n.W <= 128 ? 8 : 16, n.L, true) > CHAIN_LDS_LIMIT) return false;
  return wide_shape(n) && n.L >= 1 && (n.K1 == 1 || n.K1 == 3 || n.K1 == 4);
}

int64_t wide_workspace_bytes(const Net& n, int64_t N) {   // for any k: the layout does not depend on it
  if (!wide_shape(n)) return -1;
  return wlayout(n, wgeo(n), N > 0 ? N : 1).total;
}

int wide_forward(const Net& n, const float* params, const float* X, int64_t N, float* Y, float* dY, void* ws,
                 int64_t ws_bytes, hipStream_t s) {
  return run(n, false, nullptr, params, X, N, Y, dY, ws, ws_bytes, s);
}

int wide_loss(const Net& n, const LossReq& rq, const float* params, const float* X, int64_t N, void* ws,
              int64_t ws_bytes, hipStream_t s) {
  return run(n, rq.grad != nullptr, &rq, params, X, N, nullptr, nullptr, ws, ws_bytes, s);
}

}  // namespace pinn
