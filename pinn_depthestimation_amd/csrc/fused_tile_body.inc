  // fused_tile_body.inc — the body of the fused tile kernel (fused_kernel.h), included into k_fused and k_fused_ens.  In scope:
  // the template parameters' names WP, K1, GRAD, LDSACC, ACT, EPI, KRO, DROP and the kernel parameters P.  Everything per
  // workgroup is addressed through blockIdx.x and gridDim.x only.
  constexpr bool PACED = WP >= PACE_MIN_WP;              // fused_kernel.h, PACING
  constexpr int GAP_FWD = PACED ? PACE_GAP : PACE_OFF;
  constexpr bool IO1 = KRO > 0;
  constexpr int KRI = IO1 ? 1 : 4;          // k-steps of the first layer's contraction (d_in <= 4 when IO1)
  constexpr int KRL = IO1 ? KRO : 4;        // k-steps of the output layer's reverse contraction
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int NTH = WP / 16;
  constexpr bool SIN0 = ACT == PINN_ACT_SIN_TANH;                // sine on hidden layer 0 (fused_kernel.h: activate_sin_to, sin_adjoint_to) ...
  constexpr int ACT_H = SIN0 ? PINN_ACT_TANH : ACT;              // ... and this activation on every other hidden layer
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p = lane & 15, q = lane >> 4;
  float* lacc = smem;
  int* locks = reinterpret_cast<int*>(smem + P.lds_acc_floats);
  float* tb = smem + P.lds_acc_floats + MAX_LOCKS + wave * (TB_PER_WAVE * TB_FLOATS);
  float* lsum = smem + P.lds_acc_floats + MAX_LOCKS + FUSED_WAVES * TB_PER_WAVE * TB_FLOATS;
  const int PP = P.PW + P.PB;
  GradSink<LDSACC> sink;
  sink.acc = LDSACC ? lacc : P.wg_grads + (int64_t)blockIdx.x * PP;
  sink.locks = locks;
  if (GRAD) {
    if (LDSACC) {
      for (int i = threadIdx.x; i < PP; i += FUSED_THREADS) lacc[i] = 0.f;
    }
    if (threadIdx.x < MAX_LOCKS) locks[threadIdx.x] = 0;
    __syncthreads();
  }
  float sums[MAX_SUMS];
#pragma unroll
  for (int j = 0; j < MAX_SUMS; ++j) sums[j] = 0.f;

  ScatterMap<K1> sm, sm_mse;
  build_scatter_maps<K1>(P, q, sm, sm_mse);
  // EPI_ADJ numbers the waves WORKGROUP-MAJOR: launched with one workgroup per tile (pinn_fused.hip), only wave 0 of a
  // workgroup has work while n_tiles <= gridDim.x, its adds into the workgroup's gradient copy happen in program order
  // and the result is bit-reproducible from run to run (include/pinn_hip.h, pinn_jet_backward).  Either numbering is a
  // bijection onto [0, nw): the spill slots stay private.
  const int nw = gridDim.x * FUSED_WAVES;
  const int gw = EPI == EPI_ADJ ? wave * (int)gridDim.x + (int)blockIdx.x : (int)blockIdx.x * FUSED_WAVES + wave;
  // restrict-qualified views: weights / biases / inputs are read-only for the whole launch and the
  // spill slot is private to this wave, so loads may be scheduled across the spill stores
  float* __restrict__ scr = P.scratch + (int64_t)gw * P.scratch_per_wave;
  const float* __restrict__ Wp_ = P.Wp;
  const float* __restrict__ WTp_ = P.WTp;
  const float* __restrict__ Bp_ = P.Bp;
  constexpr int SLOT = K1 * NTH * 256;  // floats per spilled layer
  const int L = P.L;

#ifdef PINN_DIAG
  unsigned long long diag[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, tprev = __builtin_amdgcn_s_memtime();
#endif
  auto load_x = [&](int64_t t, f4& x) {
    int64_t pc = t * 16 + p;
    pc = pc < P.N ? pc : P.N - 1;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int f = IO1 ? (r == 0 ? q : 16) : 4 * q + r;      // (IO1: column q in register 0, nothing else)
      x[r] = (f < P.d_in) ? P.X[pc * P.d_in + f] : 0.f;
    }
  };
  f4 xnext;
  load_x(gw < P.n_tiles ? gw : 0, xnext);
  for (int64_t tile = gw; tile < P.n_tiles; tile += nw) {
    PINN_STAMP(11);
    const int64_t pt = tile * 16 + p;
    const bool valid = pt < P.N;
    const int64_t ptc = valid ? pt : P.N - 1;
    DropLane dl;
    if constexpr (DROP) dl.init(P.drop_seed, P.drop_thresh, P.drop_scale, P.drop_keep, pt);
    // (finite_input HERE, where the prefetched inputs are first used, not in load_x: there it makes the wave wait for the load
    // it has just issued — measured 0.7 % of the 8x64 step)
    const f4 xcur = {finite_input(xnext[0]), finite_input(xnext[1]), finite_input(xnext[2]), finite_input(xnext[3])};
    load_x(tile + nw < P.n_tiles ? tile + nw : tile, xnext);
    // ---- layer-0 input jet: features 4q + r of (x, unit tangents) --------------------------
    auto input_jet = [&](f4 (&b)[K1][1]) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = 4 * q + r;                 // PADDED input index (dir_col holds padded indices when IO1)
        b[0][0][r] = xcur[r];
#pragma unroll
        for (int c = 1; c < K1; ++c) b[c][0][r] = (f == P.dir_col[c - 1]) ? 1.f : 0.f;
      }
    };
    f4 b0[K1][1];
    input_jet(b0);
    // ---- forward chain: weights streamed block-by-block (gemm_stream), activations written straight
    // into the next GEMM's B operand: nothing is copied between layers ------------------------------
    f4 a[K1][NTH];
    f4 ws[NTH];   // the weight block the next GEMM starts with
    {
      f4 w0[NTH][1];
      load_w<1, NTH>(Wp_, w0, p, q);
      load_wblk<NTH>(Wp_ + w_off_p<WP>(L > 1 ? 1 : L), 0, ws, p, q);
      f4 bias[NTH];
      load_bias<NTH>(Bp_ + b_off_p<WP>(0), bias, q);
      f4 acc0[K1][NTH];
      zero_tiles<NTH, K1>(acc0);
      gemm_chain<1, NTH, K1, KRI>(w0, b0, acc0);
      PINN_STAMP(0);
      if constexpr (SIN0) activate_sin_to<NTH, K1>(acc0, bias, a, Wp_, P.X + ptc * P.d_in, P.d_in, q);
      else activate_to<ACT, NTH, K1, DROP>(acc0, bias, a, &dl, 0, q);
    }
    PINN_STAMP(1);
    for (int l = 1; l < L; ++l) {
      f4 bias[NTH];
      f4 nx[K1][NTH];
      zero_tiles<NTH, K1>(nx);
      // a_l (this GEMM's B operand) is spilled and the layer's bias requested from INSIDE the GEMM (see gemm_stream); a_L is
      // never spilled
      const SpillOps<NTH, K1, GRAD> sp{scr + (l - 1) * SLOT, a, lane};
      const BiasOps<NTH> lb{Bp_ + b_off_p<WP>(l), bias, q};
      gemm_stream<NTH, NTH, K1, SpillOps<NTH, K1, GRAD>, BiasOps<NTH>, GAP_FWD>(Wp_ + w_off_p<WP>(l), Wp_ + w_off_p<WP>(l + 1), ws, a, nx, p, q, sp, lb);
      PINN_STAMP(0);
      activate_to<ACT_H, NTH, K1, DROP>(nx, bias, a, &dl, l, q);
      PINN_STAMP(1);
    }
    f4 G[K1][1];
    f4 out[K1][1];
    if constexpr (EPI == EPI_ADJ) {
      // the output adjoint does not depend on the outputs: no output GEMM; the caller's adjoints are requested here,
      // behind the forward chain (held across it they would spill at width 64) and in front of the two weight loads
      // below, and first used by the output layer's weight gradient
      load_adjoint<K1>(P, G, pt, valid, q);
      load_wblk<NTH>(WTp_ + w_off_p<WP>(L > 1 ? L - 1 : 0), 0, ws, p, q);
    } else {
      f4 bias_o[1];
      zero_tiles<1, K1>(out);
      // (the block fetched behind the output GEMM is W_{L-1}^T's first: the reverse sweep starts there)
      const BiasOps<1> lb{Bp_ + b_off_p<WP>(L), bias_o, q};
      gemm_stream<NTH, 1, K1, NoOps, BiasOps<1>, GAP_FWD>(Wp_ + w_off_p<WP>(L), WTp_ + w_off_p<WP>(L > 1 ? L - 1 : 0), ws, a, out, p, q, NoOps(), lb);
      out[0][0] += bias_o[0];
    }
    // reverse-sweep operands whose latency the residual evaluation below hides
    f4 wtl[NTH][1];
    f4 ai[K1][NTH];
    if constexpr (GRAD) load_w<1, NTH>(WTp_ + w_off_p<WP>(L), wtl, p, q);

    // ---- outputs / loss -----------------------------------------------------------------------
    if constexpr (EPI == EPI_FIELD) field_epilogue<K1>(P, out, pt, ptc, valid, p, q);
    else if constexpr (EPI == EPI_FIELD_PEC) field_tile<ResPhysicsEquationCorrected, K1>(P, out, pt, valid, false, p, q);
    else if constexpr (EPI == EPI_FIELD_WAVE) field_tile<ResPhysicsEquationWave, K1>(P, out, pt, valid, false, p, q);
    else if constexpr (EPI == EPI_COEF) coef_epilogue<K1, GRAD>(P, out, G, sums, sm, tb, valid, p, q);
    else if constexpr (EPI == EPI_WEIGHTED) weighted_epilogue<K1, GRAD>(P, out, G, sums, sm, tb, pt, ptc, valid, p, q);
    else if constexpr (EPI != EPI_ADJ) loss_epilogue<K1, GRAD, (WP < 64 || EPI == EPI_PEC || EPI == EPI_WAVE), EPI>(P, out, G, sums, sm, sm_mse, tb, pt, ptc, valid, p, q);

    PINN_STAMP(2);
    // ---- reverse sweep ------------------------------------------------------------------------
    // State entering iteration l: z = zbar of hidden layer l, ai = a_l (its load in flight), ws =
    // first block of W_l^T.  The iteration runs  abar_l = W_l^T z  (a_l lands meanwhile), then
    // dW_l = z (x) a_l, then z <- adjoint(abar_l, a_l) = zbar of layer l-1, and only then re-uses
    // ai's registers for a_{l-1}: each spilled layer is read once, into the registers it is used
    // from, and there are no loop-carried copies.
    if constexpr (GRAD) {
      weight_grad<1, NTH, K1, false, PACED>(sink, L, w_off_p<WP>(L), P.PW + b_off_p<WP>(L), G, a, tb, lane);
      f4 z[K1][NTH];
      {
        f4 g[K1][NTH];
        zero_tiles<NTH, K1>(g);
        gemm_chain<1, NTH, K1, KRL>(wtl, G, g);
        if constexpr (SIN0) {   // L == 1: the output layer's adjoint feeds the sine adjoint directly
          if (L == 1) { f4 b1[K1][1]; input_jet(b1); sin_adjoint_to<NTH, K1, KRI>(Wp_, Bp_ + b_off_p<WP>(0), b1, g, z, p, q, P.X + ptc * P.d_in, P.d_in); }
          else activate_adjoint_to<ACT_H, NTH, K1, DROP>(g, a, z, &dl, L - 1, q);
        } else activate_adjoint_to<ACT, NTH, K1, DROP>(g, a, z, &dl, L - 1, q);
      }
      for (int l = L - 1; l >= 1; --l) {
        PINN_STAMP(3);
        f4 g2[K1][NTH];
        zero_tiles<NTH, K1>(g2);
        // a_l is requested from inside the GEMM (see gemm_stream: behind block 1's weight loads, in one run — PACE_OFF) and used
        // by the weight gradient after it
        const UnspillOps<NTH, K1> ld{scr + (l - 1) * SLOT, ai, lane};
        gemm_stream<NTH, NTH, K1, UnspillOps<NTH, K1>, NoOps, PACE_OFF>(WTp_ + w_off_p<WP>(l), WTp_ + w_off_p<WP>(l >= 2 ? l - 1 : 1), ws, z, g2, p, q, ld);
        PINN_STAMP(6);
        weight_grad<NTH, NTH, K1, false, PACED>(sink, l, w_off_p<WP>(l), P.PW + b_off_p<WP>(l), z, ai, tb, lane);
        PINN_STAMP(5);
        if constexpr (SIN0) {   // l == 1: the adjoint of layer 0, the sine, from a recomputed z_0
          if (l == 1) { f4 b1[K1][1]; input_jet(b1); sin_adjoint_to<NTH, K1, KRI>(Wp_, Bp_ + b_off_p<WP>(0), b1, g2, z, p, q, P.X + ptc * P.d_in, P.d_in); }
          else activate_adjoint_to<ACT_H, NTH, K1, DROP>(g2, ai, z, &dl, l - 1, q);
        } else activate_adjoint_to<ACT, NTH, K1, DROP>(g2, ai, z, &dl, l - 1, q);
        PINN_STAMP(4);
      }
      {  // layer 0: z = zbar_0, input = (x, unit tangents)
        f4 b1[K1][1];
        input_jet(b1);   // recomputed rather than kept live across the whole tile; with UNIT_A weight_grad reads the coordinates only
        // (UNIT_A for the LDS-copy instances only: with it, clang 22 crashes in its 'Rewrite AGPR-Copy-MFMA' pass on the
        // width-64 LeakyReLU instance that keeps its gradient copy in global memory)
        weight_grad<NTH, 1, K1, LDSACC, PACED>(sink, 0, 0, P.PW + b_off_p<WP>(0), z, b1, tb, lane, P.dir_col);
      }
    }
    PINN_STAMP(7);
  }
#ifdef PINN_DIAG
  if (blockIdx.x == 0 && threadIdx.x == 0 && GRAD) {
    unsigned long long tot = 0;
    for (int i = 0; i < 12; ++i) tot += diag[i];
    printf("DIAG cycles/wave: fwd_gemm %llu fwd_act+spill %llu out+residual %llu | unspill_wait %llu adjoint %llu wgrad(transp+mfma+flush) %llu bwd_gemm %llu first/last-layer %llu loop-top %llu | total %llu\n",
           diag[0], diag[1], diag[2], diag[3], diag[4], diag[5], diag[6], diag[7], diag[11], tot);
  }
#endif

  if constexpr (EPI == EPI_FIELD || EPI == EPI_FIELD_PEC || EPI == EPI_FIELD_WAVE) return;   // nothing to reduce: the fields are already where they belong
  // ---- per-workgroup reductions ------------------------------------------------------------------
#pragma unroll
  for (int j = 0; j < MAX_SUMS; ++j) {
    float v = sums[j];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0) lsum[wave * MAX_SUMS + j] = v;
  }
  __syncthreads();
  if (threadIdx.x < MAX_SUMS) {
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < FUSED_WAVES; ++w) v += lsum[w * MAX_SUMS + threadIdx.x];
    P.wg_sums[(int64_t)blockIdx.x * MAX_SUMS + threadIdx.x] = v;
  }
  if (GRAD && LDSACC) {
    float* dst = P.wg_grads + (int64_t)blockIdx.x * PP;
    for (int i = threadIdx.x; i < PP; i += FUSED_THREADS) dst[i] = lacc[i];
  }
