// residuals.h — per-point PDE residual fields and their adjoints, written on the
// forward-mode jet (y, dy/dx_j) of the network outputs.
//
// The reference obtains every partial derivative with torch.autograd.grad
// (physics.py:6-15) and the parameter gradient with a second reverse pass
// (train.py:191).  All of its PDEs are first order in the inputs, so here the
// residual is a pointwise function r(y, dy) of the jet and its adjoint
// (dr/dy, dr/ddy) is written out by hand.  Each struct cites the lines it
// restates.  v[c][r]: c = 0 value, c = 1+d the derivative along direction role
// d; r = output role.  g has the same shape and receives
// sum_t scale[t] * d(field_t^2)/dv.
//
// Each PDE states its field expressions ONCE and its adjoint ONCE, as __host__ __device__ functions (the *_point entries
// of pinn_abi.hip run them on the host, where tests hold them to fp64 without a GPU):
//   fields(v, closure, f)                 the signed fields
//   adjoint(v, rc, rx, ry, g)             g <- rc dfc/dv + rx dfx/dv + ry dfy/dv  (rc, rx, ry: 2 scale[t] f[t] in eval)
//   eval<GRAD>(v, closure, scale, g, sq)  fields, their squares and, with GRAD, the adjoint
// and everything else is derived from them: the coefficient structs pass a run-time closure constant to the same
// functions, the second-order structs add only which roles carry the Laplacian.  `closure` is the
// residual's own small Closure type — what it needs beside the jet — so that every caller has one call shape.
// Three pairs remain, each marked THE ONLY PAIR with its reason: the field lines of Navier_Stokes and of physics_equation
// under a second rounding contract, and the corrected physics_equation's adjoint inside its eval.
// In an eval, rc, rx, ry are NAMED before the adjoint call, in that order: the order instructions reach the optimiser in
// decides which product of a sum of two is fused into the multiply-add, i.e. the last bits (tools/residual_parity.py).
#pragma once
#include <hip/hip_runtime.h>

namespace pinn {

struct NoClosure {};

// physics.py:50-88  Navier_Stokes(t, x, y, h, z, u, v)
// roles: outputs h=0 z=1 u=2 v=3; directions t=0 x=1 y=2
// The breaking constant CB = 3/16 g gamma_b^2 (physics.py:76-78) is an argument of the shared functions (*_cb): this struct
// passes the compile-time constant formed in double, ResNavierStokesCoef the fp32 run-time value.
struct ResNavierStokes {
  static constexpr int NR = 4, ND = 3, NT = 3, NF = 3;
  typedef NoClosure Closure;
  static constexpr float CB0 = (float)(3.0 / 16.0 * 9.81 * (0.78 * 0.78));   // physics.py:76-78
  // the signed fields f = (fc, fm_x, fm_y)
  __host__ __device__ static inline void fields_cb(const float (&v)[1 + ND][NR], float CB, float (&f)[NF]) {
    const float h = v[0][0], z = v[0][1], u = v[0][2], w = v[0][3];
    const float z_t = v[1][1], u_t = v[1][2], w_t = v[1][3];
    const float h_x = v[2][0], z_x = v[2][1], u_x = v[2][2], w_x = v[2][3];
    const float h_y = v[3][0], z_y = v[3][1], u_y = v[3][2], w_y = v[3][3];
    const float G = 9.81f;                                      // physics.py:75
    const float H = h + z;                  // total depth h+z (physics.py:64-68)
    const float Hx = h_x + z_x, Hy = h_y + z_y;
    const float hu_x = Hx * u + H * u_x;    // d((h+z)u)/dx  physics.py:67
    const float hv_y = Hy * w + H * w_y;    // d((h+z)v)/dy  physics.py:68
    const float Fbr_x = CB * Hx * H, Fbr_y = CB * Hy * H;       // physics.py:77-78
    f[0] = z_t + hu_x + hv_y;                                // physics.py:81
    f[1] = u_t + u * u_x + w * u_y + G * z_x + Fbr_x;        // physics.py:82
    f[2] = w_t + u * w_x + w * w_y + G * z_y + Fbr_y;        // physics.py:83
  }
  // THE ONLY PAIR: fields_cb's lines once more under contract(off), for ResNavierStokesCoef.  Its fields must round the same
  // way in every instance (the forward-only sums equal the gradient call's bit for bit), the plain fields keep the
  // contraction the compiler chooses (switching them off would change the bits of every plain kernel), and the pragma is
  // lexical — it does not follow an inlined callee — so two rounding contracts are two statements.  Change both or neither.
  __host__ __device__ static inline void fields_cb_strict(const float (&v)[1 + ND][NR], float CB, float (&f)[NF]) {
#pragma clang fp contract(off)
    const float h = v[0][0], z = v[0][1], u = v[0][2], w = v[0][3];
    const float z_t = v[1][1], u_t = v[1][2], w_t = v[1][3];
    const float h_x = v[2][0], z_x = v[2][1], u_x = v[2][2], w_x = v[2][3];
    const float h_y = v[3][0], z_y = v[3][1], u_y = v[3][2], w_y = v[3][3];
    const float G = 9.81f;
    const float H = h + z;
    const float Hx = h_x + z_x, Hy = h_y + z_y;
    const float hu_x = Hx * u + H * u_x;
    const float hv_y = Hy * w + H * w_y;
    const float Fbr_x = CB * Hx * H, Fbr_y = CB * Hy * H;
    f[0] = z_t + hu_x + hv_y;
    f[1] = u_t + u * u_x + w * u_y + G * z_x + Fbr_x;
    f[2] = w_t + u * w_x + w * w_y + G * z_y + Fbr_y;
  }
  // g <- rc dfc/dv + rx dfm_x/dv + ry dfm_y/dv
  __host__ __device__ static inline void adjoint_cb(const float (&v)[1 + ND][NR], float CB, float rc, float rx, float ry,
                                                    float (&g)[1 + ND][NR]) {
    const float h = v[0][0], z = v[0][1], u = v[0][2], w = v[0][3];
    const float h_x = v[2][0], z_x = v[2][1], u_x = v[2][2], w_x = v[2][3];
    const float h_y = v[3][0], z_y = v[3][1], u_y = v[3][2], w_y = v[3][3];
    const float G = 9.81f;
    const float H = h + z;
    const float Hx = h_x + z_x, Hy = h_y + z_y;
    const float gh = rc * (u_x + w_y) + CB * (rx * Hx + ry * Hy);
    g[0][0] = gh; g[0][1] = gh;
    g[0][2] = rc * Hx + rx * u_x + ry * w_x;
    g[0][3] = rc * Hy + rx * u_y + ry * w_y;
    g[1][0] = 0.f; g[1][1] = rc; g[1][2] = rx; g[1][3] = ry;
    const float ghx = rc * u + rx * CB * H;
    g[2][0] = ghx; g[2][1] = ghx + rx * G;
    g[2][2] = rc * H + rx * u; g[2][3] = ry * u;
    const float ghy = rc * w + ry * CB * H;
    g[3][0] = ghy; g[3][1] = ghy + ry * G;
    g[3][2] = rx * w; g[3][3] = rc * H + ry * w;
  }
  __host__ __device__ static inline void fields(const float (&v)[1 + ND][NR], const Closure&, float (&f)[NF]) { fields_cb(v, CB0, f); }
  __host__ __device__ static inline void adjoint(const float (&v)[1 + ND][NR], float rc, float rx, float ry,
                                                 float (&g)[1 + ND][NR]) {
    adjoint_cb(v, CB0, rc, rx, ry, g);
  }
  template <bool GRAD>
  __host__ __device__ static inline void eval(const float (&v)[1 + ND][NR], const Closure& cl, const float* scale,
                                              float (&g)[1 + ND][NR], float (&sq)[NT]) {
    float f[NF];
    fields(v, cl, f);
    sq[0] = f[0] * f[0]; sq[1] = f[1] * f[1]; sq[2] = f[2] * f[2];   // physics.py:86
    if (GRAD) {
      const float rc = 2.f * scale[0] * f[0], rx = 2.f * scale[1] * f[1], ry = 2.f * scale[2] * f[2];
      adjoint(v, rc, rx, ry, g);
    }
  }
};

// physics.py:91-120  physics_equation(x, y, h, U, V, eta_mean, Hrms, k)
// roles: outputs h=0 U=1 V=2 eta_mean=3 Hrms=4 k=5; directions x=0 y=1.
// Bug-compatible with physics.py:106: E = 1/8**rho*g*Hrms**2 == 0.0, so the
// radiation-stress terms Sxx_x, Syy_y contribute exactly 0 to loss and gradient
// and Hrms, k receive zero adjoints.
// The friction constant RC = rho Cd (physics.py:102-103) is an argument of the shared functions (*_rc): this struct passes
// the compile-time constant formed in double, ResPhysicsEquationCoef the fp32 run-time value.
struct ResPhysicsEquation {
  static constexpr int NR = 6, ND = 2, NT = 3, NF = 3;
  typedef NoClosure Closure;
  static constexpr float RC0 = (float)(1025 * 0.002);     // rho*Cd  physics.py:102-103
  // the signed fields f = (fc, fx, fy)
  __host__ __device__ static inline void fields_rc(const float (&v)[1 + ND][NR], float RC, float (&f)[NF]) {
    const float h = v[0][0], U = v[0][1], V = v[0][2], eta = v[0][3];
    const float U_x = v[1][1], V_x = v[1][2], e_x = v[1][3];
    const float U_y = v[2][1], V_y = v[2][2], e_y = v[2][3];
    const float G = 9.81f, RHO = 1025.f;
    const float tbx = (RC * U) * fabsf(U);       // tau_bx  physics.py:102
    const float tby = (RC * V) * fabsf(V);       // tau_by  physics.py:103
    const float D = 1.0f / (RHO * (eta + h));    // physics.py:114-115
    f[0] = U_x + V_y;                                        // physics.py:113
    f[1] = U * U_x + V * U_y + G * e_x + D * tbx;            // physics.py:114 (Sxx_x+Sxy_y == 0)
    f[2] = U * V_x + V * V_y + G * e_y + D * tby;            // physics.py:115
  }
  // THE ONLY PAIR: fields_rc's lines once more under contract(off), for ResPhysicsEquationCoef — as
  // ResNavierStokes::fields_cb_strict, for the same reasons.  Change both or neither.
  __host__ __device__ static inline void fields_rc_strict(const float (&v)[1 + ND][NR], float RC, float (&f)[NF]) {
#pragma clang fp contract(off)
    const float h = v[0][0], U = v[0][1], V = v[0][2], eta = v[0][3];
    const float U_x = v[1][1], V_x = v[1][2], e_x = v[1][3];
    const float U_y = v[2][1], V_y = v[2][2], e_y = v[2][3];
    const float G = 9.81f, RHO = 1025.f;
    const float tbx = (RC * U) * fabsf(U);
    const float tby = (RC * V) * fabsf(V);
    const float D = 1.0f / (RHO * (eta + h));
    f[0] = U_x + V_y;
    f[1] = U * U_x + V * U_y + G * e_x + D * tbx;
    f[2] = U * V_x + V * V_y + G * e_y + D * tby;
  }
  // g <- rc dfc/dv + rx dfx/dv + ry dfy/dv; zero on Hrms, k and on every derivative the fields do not read
  __host__ __device__ static inline void adjoint_rc(const float (&v)[1 + ND][NR], float RC, float rc, float rx, float ry,
                                                    float (&g)[1 + ND][NR]) {
    const float h = v[0][0], U = v[0][1], V = v[0][2], eta = v[0][3];
    const float U_x = v[1][1], V_x = v[1][2];
    const float U_y = v[2][1], V_y = v[2][2];
    const float G = 9.81f, RHO = 1025.f;
    const float tbx = (RC * U) * fabsf(U);
    const float tby = (RC * V) * fabsf(V);
    const float D = 1.0f / (RHO * (eta + h));
#pragma unroll
    for (int c = 0; c < 1 + ND; ++c)
#pragma unroll
      for (int r = 0; r < NR; ++r) g[c][r] = 0.f;
    const float dD = -RHO * D * D;             // d D / d(eta+h)
    const float gS = dD * (rx * tbx + ry * tby);
    g[0][0] = gS; g[0][3] = gS;
    g[0][1] = rx * (U_x + D * RC * 2.f * fabsf(U)) + ry * V_x;
    g[0][2] = rx * U_y + ry * (V_y + D * RC * 2.f * fabsf(V));
    g[1][1] = rc + rx * U;   // d/dU_x
    g[1][2] = ry * U;        // d/dV_x
    g[1][3] = rx * G;        // d/deta_x
    g[2][1] = rx * V;        // d/dU_y
    g[2][2] = rc + ry * V;   // d/dV_y
    g[2][3] = ry * G;        // d/deta_y
  }
  __host__ __device__ static inline void fields(const float (&v)[1 + ND][NR], const Closure&, float (&f)[NF]) { fields_rc(v, RC0, f); }
  __host__ __device__ static inline void adjoint(const float (&v)[1 + ND][NR], float rc, float rx, float ry,
                                                 float (&g)[1 + ND][NR]) {
    adjoint_rc(v, RC0, rc, rx, ry, g);
  }
  // THE NaN CARRIER, in this eval only — never in the coefficient or the second-order form, whose callers and tests know
  // exact zeros there.  The zero adjoint of Hrms and k is written 0 * |rx + ry|: +0 at every finite point, NaN where the
  // point's momentum fields are not finite, so that the gradient of the two output biases is NaN at a NaN point as the
  // reference's is (0.0 * nan; tests/test_nonfinite_gpu.py).  It is a NaN carrier only, not physics.py's expression: there
  // E = 0.0 * Hrms**2 also makes fx and fy NaN when Hrms or k ALONE is not finite, which these kernels' forward does not.
  template <bool GRAD>
  __host__ __device__ static inline void eval(const float (&v)[1 + ND][NR], const Closure& cl, const float* scale,
                                              float (&g)[1 + ND][NR], float (&sq)[NT]) {
    float f[NF];
    fields(v, cl, f);
    sq[0] = f[0] * f[0]; sq[1] = f[1] * f[1]; sq[2] = f[2] * f[2];   // physics.py:118
    if (GRAD) {
      const float rc = 2.f * scale[0] * f[0], rx = 2.f * scale[1] * f[1], ry = 2.f * scale[2] * f[2];
      adjoint(v, rc, rx, ry, g);
      g[0][4] = g[0][5] = 0.f * fabsf(rx + ry);
    }
  }
};

// physics_equation with the radiation stress physics.py:106-109 evidently meant (the package's
// physics.physics_equation(..., corrected=True)): E = rho g Hrms^2 / 8, Sxx = E (2n + 1/2), Syy = E n, n = kh / sinh 2kh.
// Same roles and directions as ResPhysicsEquation; selected by pinn_residual_spec.flags bit 0, never by an id of its own.
//   fx = U U_x + V U_y + G eta_x + D (tbx + d Sxx / dx),   fy likewise with d Syy / dy
struct ResPhysicsEquationCorrected {
  static constexpr int NR = 6, ND = 2, NT = 3, NF = 3;
  typedef NoClosure Closure;
  // n(s) = s / sinh 2s with n1 = dn/ds = (S - 2sC) / S^2 and n2 = d2n/ds2 = 4 (s S^2 - C S + 2s) / S^3 (S = sinh 2s,
  // C = cosh 2s).  Formed from t = exp(-2|s|): 1/S = 2t / (1 - t^2), C/S = (1 + t^2) / (1 - t^2) — nothing overflows,
  // however large |s| (t underflows to 0 and with it n, n1, n2) — and by parity (n, n2 even, n1 odd).  Below |s| = 1/4
  // both closed forms cancel (1 - 2s C/S ~ -4/3 s^2), so there the Taylor series of 2s / sinh 2s through s^12 takes
  // over: first dropped term of n2 is 1e-8 at the threshold; the closed n2 loses a factor 30 (3e-6) just above it.
  // At s = 0 the limits (1/2, 0, -2/3).
  __host__ __device__ static inline void ratio(float s, float& n, float& n1, float& n2) {
    const float a = fabsf(s);
    if (a < 0.25f) {
      constexpr float A1 = (float)(-1.0 / 3.0), A2 = (float)(7.0 / 45.0), A3 = (float)(-62.0 / 945.0),
                      A4 = (float)(127.0 / 4725.0), A5 = (float)(-146.0 / 13365.0), A6 = (float)(2828954.0 / 638512875.0);
      const float u = s * s;
      n = fmaf(fmaf(fmaf(fmaf(fmaf(fmaf(A6, u, A5), u, A4), u, A3), u, A2), u, A1), u, 0.5f);
      n1 = s * fmaf(fmaf(fmaf(fmaf(fmaf(12.f * A6, u, 10.f * A5), u, 8.f * A4), u, 6.f * A3), u, 4.f * A2), u, 2.f * A1);
      n2 = fmaf(fmaf(fmaf(fmaf(fmaf(132.f * A6, u, 90.f * A5), u, 56.f * A4), u, 30.f * A3), u, 12.f * A2), u, 2.f * A1);
    } else {
      const float t = expf(-2.f * a), t2 = t * t;
      const float id = 1.0f / (1.f - t2);
      const float iS = 2.f * t * id, ct = (1.f + t2) * id;      // 1 / sinh 2a, coth 2a
      n = a * iS;
      const float m1 = iS * (1.f - 2.f * a * ct);
      n1 = s < 0.f ? -m1 : m1;
      n2 = 4.f * iS * (a - ct + 2.f * a * (iS * iS));
    }
  }
  // everything the fields and the adjoint share
  struct Mid { float D, tbx, tby, E, n, n1, n2, s_x, s_y, E_x, E_y, Sx, Sy; };
  __host__ __device__ static inline Mid mid(const float (&v)[1 + ND][NR]) {
    const float h = v[0][0], U = v[0][1], V = v[0][2], eta = v[0][3], R = v[0][4], K = v[0][5];
    const float h_x = v[1][0], R_x = v[1][4], K_x = v[1][5];
    const float h_y = v[2][0], R_y = v[2][4], K_y = v[2][5];
    const float RHO = 1025.f;
    const float RC = (float)(1025 * 0.002);
    const float C_E = (float)(1025 * 9.81 / 8.0);     // rho g / 8
    Mid m;
    m.tbx = (RC * U) * fabsf(U);
    m.tby = (RC * V) * fabsf(V);
    m.D = 1.0f / (RHO * (eta + h));
    m.E = C_E * R * R;
    m.E_x = 2.f * C_E * R * R_x; m.E_y = 2.f * C_E * R * R_y;
    m.s_x = K_x * h + K * h_x; m.s_y = K_y * h + K * h_y;
    ratio(K * h, m.n, m.n1, m.n2);
    m.Sx = m.E_x * (2.f * m.n + 0.5f) + 2.f * m.E * m.n1 * m.s_x;   // d Sxx / dx
    m.Sy = m.E_y * m.n + m.E * m.n1 * m.s_y;                        // d Syy / dy
    return m;
  }
  __host__ __device__ static inline void fields(const float (&v)[1 + ND][NR], const Closure&, float (&f)[NF]) {
    const float U = v[0][1], V = v[0][2];
    const float U_x = v[1][1], V_x = v[1][2], e_x = v[1][3];
    const float U_y = v[2][1], V_y = v[2][2], e_y = v[2][3];
    const float G = 9.81f;
    const Mid m = mid(v);
    f[0] = U_x + V_y;
    f[1] = U * U_x + V * U_y + G * e_x + m.D * (m.tbx + m.Sx);
    f[2] = U * V_x + V * V_y + G * e_y + m.D * (m.tby + m.Sy);
  }
  // The adjoint on given (rc, rx, ry), for Residual2<> — eval's lines below once more: THE ONLY PAIR of this struct, kept
  // because eval written as a call of this function does not compile to the parent's code (the sum g[0][1] has its two
  // products fused the other way round and the gradient's last bits differ: DESIGN.md 2.20).  Change both or neither.
  __host__ __device__ static inline void adjoint(const float (&v)[1 + ND][NR], float rc, float rx, float ry,
                                                 float (&g)[1 + ND][NR]) {
    const float h = v[0][0], U = v[0][1], V = v[0][2], R = v[0][4], K = v[0][5];
    const float h_x = v[1][0], U_x = v[1][1], V_x = v[1][2], R_x = v[1][4], K_x = v[1][5];
    const float h_y = v[2][0], U_y = v[2][1], V_y = v[2][2], R_y = v[2][4], K_y = v[2][5];
    const float G = 9.81f, RHO = 1025.f;
    const float RC = (float)(1025 * 0.002);
    const float C_E = (float)(1025 * 9.81 / 8.0);
    const Mid m = mid(v);
    const float ax = rx * m.D, ay = ry * m.D;
    const float dD = -RHO * m.D * m.D;             // d D / d(eta+h)
    const float gS = dD * (rx * (m.tbx + m.Sx) + ry * (m.tby + m.Sy));
    const float ds = ax * (2.f * m.E_x * m.n1 + 2.f * m.E * m.n2 * m.s_x) + ay * (m.E_y * m.n1 + m.E * m.n2 * m.s_y);   // adjoint of s = kh
    const float gsx = 2.f * ax * m.E * m.n1, gsy = ay * m.E * m.n1;   // adjoints of s_x, s_y
    const float nn = 2.f * m.n + 0.5f;
    g[0][0] = gS + ds * K + gsx * K_x + gsy * K_y;
    g[0][1] = rx * (U_x + m.D * RC * 2.f * fabsf(U)) + ry * V_x;
    g[0][2] = rx * U_y + ry * (V_y + m.D * RC * 2.f * fabsf(V));
    g[0][3] = gS;
    g[0][4] = ax * (2.f * C_E * R_x * nn + 4.f * C_E * R * m.n1 * m.s_x) + ay * (2.f * C_E * R_y * m.n + 2.f * C_E * R * m.n1 * m.s_y);
    g[0][5] = ds * h + gsx * h_x + gsy * h_y;
    g[1][0] = gsx * K;       // d/dh_x
    g[1][1] = rc + rx * U;   // d/dU_x
    g[1][2] = ry * U;        // d/dV_x
    g[1][3] = rx * G;        // d/deta_x
    g[1][4] = 2.f * ax * C_E * R * nn;   // d/dHrms_x
    g[1][5] = gsx * h;       // d/dk_x
    g[2][0] = gsy * K;
    g[2][1] = rx * V;
    g[2][2] = rc + ry * V;
    g[2][3] = ry * G;
    g[2][4] = 2.f * ay * C_E * R * m.n;
    g[2][5] = gsy * h;
  }
  template <bool GRAD>
  __host__ __device__ static inline void eval(const float (&v)[1 + ND][NR], const Closure& cl, const float* scale,
                                              float (&g)[1 + ND][NR], float (&sq)[NT]) {
    float f[NF];
    fields(v, cl, f);
    sq[0] = f[0] * f[0]; sq[1] = f[1] * f[1]; sq[2] = f[2] * f[2];
    if (GRAD) {
      const float h = v[0][0], U = v[0][1], V = v[0][2], R = v[0][4], K = v[0][5];
      const float h_x = v[1][0], U_x = v[1][1], V_x = v[1][2], R_x = v[1][4], K_x = v[1][5];
      const float h_y = v[2][0], U_y = v[2][1], V_y = v[2][2], R_y = v[2][4], K_y = v[2][5];
      const float G = 9.81f, RHO = 1025.f;
      const float RC = (float)(1025 * 0.002);
      const float C_E = (float)(1025 * 9.81 / 8.0);
      const Mid m = mid(v);
      const float rc = 2.f * scale[0] * f[0], rx = 2.f * scale[1] * f[1], ry = 2.f * scale[2] * f[2];
      const float ax = rx * m.D, ay = ry * m.D;
      const float dD = -RHO * m.D * m.D;             // d D / d(eta+h)
      const float gS = dD * (rx * (m.tbx + m.Sx) + ry * (m.tby + m.Sy));
      const float ds = ax * (2.f * m.E_x * m.n1 + 2.f * m.E * m.n2 * m.s_x) + ay * (m.E_y * m.n1 + m.E * m.n2 * m.s_y);   // adjoint of s = kh
      const float gsx = 2.f * ax * m.E * m.n1, gsy = ay * m.E * m.n1;   // adjoints of s_x, s_y
      const float nn = 2.f * m.n + 0.5f;
      g[0][0] = gS + ds * K + gsx * K_x + gsy * K_y;
      g[0][1] = rx * (U_x + m.D * RC * 2.f * fabsf(U)) + ry * V_x;
      g[0][2] = rx * U_y + ry * (V_y + m.D * RC * 2.f * fabsf(V));
      g[0][3] = gS;
      g[0][4] = ax * (2.f * C_E * R_x * nn + 4.f * C_E * R * m.n1 * m.s_x) + ay * (2.f * C_E * R_y * m.n + 2.f * C_E * R * m.n1 * m.s_y);
      g[0][5] = ds * h + gsx * h_x + gsy * h_y;
      g[1][0] = gsx * K;       // d/dh_x
      g[1][1] = rc + rx * U;   // d/dU_x
      g[1][2] = ry * U;        // d/dV_x
      g[1][3] = rx * G;        // d/deta_x
      g[1][4] = 2.f * ax * C_E * R * nn;   // d/dHrms_x
      g[1][5] = gsx * h;       // d/dk_x
      g[2][0] = gsy * K;
      g[2][1] = rx * V;
      g[2][2] = rc + ry * V;
      g[2][3] = ry * G;
      g[2][4] = 2.f * ay * C_E * R * m.n;
      g[2][5] = gsy * h;
    }
  }
};

// The corrected physics_equation closed by the two wave equations that tie k and Hrms to the depth (the package's
// physics.physics_equation(..., corrected=True, wave_omega=, wave_gamma=)); selected by pinn_residual_spec.flags bit 1 on top
// of bit 0, never by an id of its own.  Same roles (h, U, V, eta, R = Hrms, K = k) and directions (x, y); five terms:
//   0..2  ResPhysicsEquationCorrected's fc, fx, fy (its functions are called, not restated)
//   3     f_d = G K tanh(s) / omega^2 - 1,  s = K h                       linear dispersion, dimensionless
//   4     f_E = d/dx (R^2 c_g) + eps,  c_g = (omega / K) (1/2 + n(s))     wave-energy flux balance divided by rho g / 8
//         eps = (3 sqrt(pi) / 2) (omega / 2 pi) R^5 / (gamma^2 h^3) [1 - (1 + q^2)^(-5/2)],  q = R / (gamma h)
//         (Thornton & Guza 1983 with B = 1); expanded: f_E = 2 R R_x c_g + R^2 omega [n1 s_x / K - (1/2 + n) K_x / K^2] + eps
// Waves travel along +x, as the residual's Sxy = 0 has it.  n, n1, n2 are ratio()'s.  tanh s and sech^2 s come from the same
// t = exp(-2|s|) — tanh = (1 - t) / (1 + t), sech^2 = 4t / (1 + t)^2, nothing overflows — and below ratio()'s threshold
// |s| = 1/4, where 1 - t cancels, from the Taylor series of tanh through s^11 (first dropped term 2e-10 relative there).
// No guards beyond that: K = 0 or h = 0 give non-finite values, which propagate as everywhere else; K > 0, h > 0,
// omega > 0 and gamma > 0 are the caller's to ensure (the C-ABI checks omega and gamma).
struct ResPhysicsEquationWave {
  typedef ResPhysicsEquationCorrected R1;
  static constexpr int NR = 6, ND = 2, NT = 5, NF = 5;
  struct Closure { float omega, gamma; };   // pinn_residual_spec.param[0..1]
  __host__ __device__ static inline void tanh_sech2(float s, float& T, float& S2) {
    const float a = fabsf(s);
    if (a < 0.25f) {
      constexpr float B1 = (float)(-1.0 / 3.0), B2 = (float)(2.0 / 15.0), B3 = (float)(-17.0 / 315.0),
                      B4 = (float)(62.0 / 2835.0), B5 = (float)(-1382.0 / 155925.0);
      const float u = s * s;
      T = s * fmaf(fmaf(fmaf(fmaf(fmaf(B5, u, B4), u, B3), u, B2), u, B1), u, 1.f);
      S2 = fmaf(-T, T, 1.f);
    } else {
      const float t = expf(-2.f * a);
      const float id = 1.0f / (1.f + t);
      const float m = (1.f - t) * id;
      T = s < 0.f ? -m : m;
      S2 = 4.f * t * (id * id);
    }
  }
  // everything fields and eval share of terms 3 and 4
  struct Mid { float fd, fE, Kd, T, S2, A, n1, n2, ik, s_x, Pk, cg, eps_R, eps_h; };
  __host__ __device__ static inline Mid mid(const float (&v)[1 + ND][NR], float omega, float gamma) {
    const float h = v[0][0], R = v[0][4], K = v[0][5];
    const float h_x = v[1][0], R_x = v[1][4], K_x = v[1][5];
    const float G = 9.81f;
    const float C_EPS = (float)(0.75 / 1.7724538509055160273);   // (3 sqrt(pi) / 2) / (2 pi)
    Mid m;
    const float s = K * h;
    float n;
    R1::ratio(s, n, m.n1, m.n2);
    tanh_sech2(s, m.T, m.S2);
    m.Kd = G / (omega * omega);
    m.fd = m.Kd * K * m.T - 1.f;
    m.ik = 1.0f / K;
    m.A = 0.5f + n;
    m.cg = omega * m.A * m.ik;
    m.s_x = K_x * h + K * h_x;
    m.Pk = m.n1 * m.s_x * m.ik - m.A * K_x * (m.ik * m.ik);
    // breaking: B = 1 - u^(-5/2), u = 1 + q^2, as (1 - r)(1 + r + r^2 + r^3 + r^4) with r = u^(-1/2) and 1 - r =
    // q^2 r^2 / (1 + r): no cancellation at small q; Bp = dB/dq = 5 q u^(-7/2)
    const float ih = 1.0f / h, ig = 1.0f / gamma;
    const float q = R * ig * ih;
    const float r = 1.0f / sqrtf(1.f + q * q), r2 = r * r;
    const float B = (q * q) * r2 / (1.f + r) * (1.f + r + r2 + r2 * r + r2 * r2);
    const float Bp = 5.f * q * (r2 * r2 * r2 * r);
    const float c0 = C_EPS * omega * (ig * ig) * (ih * ih * ih);
    const float R4 = (R * R) * (R * R);
    const float eps = c0 * R4 * R * B;
    m.eps_R = c0 * R4 * (5.f * B + q * Bp);
    m.eps_h = -c0 * R4 * R * ih * (3.f * B + q * Bp);
    m.fE = 2.f * R * R_x * m.cg + (R * R) * omega * m.Pk + eps;
    return m;
  }
  __host__ __device__ static inline void fields(const float (&v)[1 + ND][NR], const Closure& cl, float (&f)[NF]) {
    float f3[R1::NF];
    R1::fields(v, R1::Closure(), f3);
    const Mid m = mid(v, cl.omega, cl.gamma);
    f[0] = f3[0]; f[1] = f3[1]; f[2] = f3[2];
    f[3] = m.fd; f[4] = m.fE;
  }
  template <bool GRAD>
  __host__ __device__ static inline void eval(const float (&v)[1 + ND][NR], const Closure& cl, const float* scale,
                                              float (&g)[1 + ND][NR], float (&sq)[NT]) {
    const float omega = cl.omega;
    float sq3[R1::NT];
    R1::template eval<GRAD>(v, R1::Closure(), scale, g, sq3);      // terms 0..2 and, with GRAD, all of g
    const Mid m = mid(v, omega, cl.gamma);
    sq[0] = sq3[0]; sq[1] = sq3[1]; sq[2] = sq3[2];
    sq[3] = m.fd * m.fd; sq[4] = m.fE * m.fE;
    if (GRAD) {
      const float h = v[0][0], R = v[0][4], K = v[0][5];
      const float h_x = v[1][0], R_x = v[1][4], K_x = v[1][5];
      const float rd = 2.f * scale[3] * m.fd, rE = 2.f * scale[4] * m.fE;
      const float R2w = (R * R) * omega;
      const float ds = omega * m.ik * (2.f * R * R_x * m.n1 + (R * R) * (m.n2 * m.s_x - m.n1 * K_x * m.ik));   // d f_E / d s
      const float gsx = R2w * m.n1 * m.ik;                                                                      // d f_E / d s_x
      const float dK = -omega * (m.ik * m.ik) * (2.f * R * R_x * m.A + (R * R) * (m.n1 * m.s_x - 2.f * m.A * K_x * m.ik));   // through 1 / K
      g[0][0] += rd * m.Kd * (K * K) * m.S2 + rE * (ds * K + gsx * K_x + m.eps_h);
      g[0][4] += rE * (2.f * R_x * m.cg + 2.f * R * omega * m.Pk + m.eps_R);
      g[0][5] += rd * m.Kd * (m.T + (K * h) * m.S2) + rE * (ds * h + gsx * h_x + dK);
      g[1][0] += rE * gsx * K;                                   // d/dh_x
      g[1][4] += rE * 2.f * R * m.cg;                            // d/dHrms_x
      g[1][5] += rE * (gsx * h - R2w * m.A * (m.ik * m.ik));     // d/dk_x
    }
  }
};

// physics.py:37-47 continuity_ftemp(x, y, h, U, V); physics.py:18-33 continuity_only
// roles: outputs h=0 U=1 V=2; directions x=0 y=1.
// fc = d(hU)/dx + d(hV)/dy.  continuity_only (anchor_on) adds (h - anchor)^2 on the points
// with x < threshold (physics.py:26-28); `masked` says whether this point is one.
struct ResContinuity {
  static constexpr int NR = 3, ND = 2, NT = 3, NF = 2;
  struct Closure { bool anchor_on, masked; float anchor; };
  // f = (fc, da): da = h - anchor on the masked points of continuity_only, 0 elsewhere and for continuity_ftemp
  __host__ __device__ static inline void fields(const float (&v)[1 + ND][NR], const Closure& cl, float (&f)[NF]) {
    const float h = v[0][0], U = v[0][1], V = v[0][2];
    const float h_x = v[1][0], U_x = v[1][1];
    const float h_y = v[2][0], V_y = v[2][2];
    f[0] = h_x * U + h * U_x + h_y * V + h * V_y;                        // physics.py:20-23,39-42
    f[1] = (cl.anchor_on && cl.masked) ? (h - cl.anchor) : 0.f;          // physics.py:27-28
  }
  // sq = (fc^2, da^2, 1 on a masked point of continuity_only: the count the anchor's mean divides by)
  template <bool GRAD>
  __host__ __device__ static inline void eval(const float (&v)[1 + ND][NR], const Closure& cl, const float* scale,
                                              float (&g)[1 + ND][NR], float (&sq)[NT]) {
    float f[NF];
    fields(v, cl, f);
    const float fc = f[0], da = f[1];
    sq[0] = fc * fc;
    sq[1] = da * da;
    sq[2] = (cl.anchor_on && cl.masked) ? 1.f : 0.f;
    if (GRAD) {
      const float h = v[0][0], U = v[0][1], V = v[0][2];
      const float h_x = v[1][0], U_x = v[1][1];
      const float h_y = v[2][0], V_y = v[2][2];
      const float rc = 2.f * scale[0] * fc;
#pragma unroll
      for (int c = 0; c < 1 + ND; ++c)
#pragma unroll
        for (int r = 0; r < NR; ++r) g[c][r] = 0.f;
      g[0][0] = rc * (U_x + V_y) + (cl.anchor_on ? 2.f * scale[1] * da : 0.f);
      g[0][1] = rc * h_x;
      g[0][2] = rc * h_y;
      g[1][0] = rc * U; g[1][1] = rc * h;
      g[2][0] = rc * V; g[2][2] = rc * h;
    }
  }
};

// ---- runtime closure coefficients (pinn_residual_coef_loss_grad) -----------------------------------------------------
// Navier_Stokes and the plain physics_equation with their one physical closure read from an array instead of the literal
// above: coef[0] = gamma_b (physics.py:76, default 0.78) resp. Cd (physics.py:99, default 0.002).  NC coefficients;
// gc[j] <- d/d coef[j] sum_t scale[t] field_t^2 at this point (0 without GRAD).  The formulas are the plain structs' own
// functions with CB resp. RC formed in fp32 at run time (there: in double at compile time), so at the defaults the two
// agree to rounding, not bit for bit; the fields and their squares are formed under contract(off) (fields_*_strict above).
struct ResNavierStokesCoef {
  typedef ResNavierStokes P;
  static constexpr int NR = P::NR, ND = P::ND, NT = P::NT, NF = P::NF, NC = 1;
  static constexpr float DEFAULTS[NC] = {0.78f};
  __host__ __device__ static inline float cb(const float* coef) {
    const float gb = coef[0];
    return (float)(3.0 / 16.0 * 9.81) * (gb * gb);   // physics.py:76-78
  }
  __host__ __device__ static inline void fields(const float (&v)[1 + ND][NR], const float* coef, float (&f)[NF]) {
    P::fields_cb_strict(v, cb(coef), f);
  }
  template <bool GRAD>
  __host__ __device__ static inline void eval(const float (&v)[1 + ND][NR], const float* coef, const float* scale,
                                              float (&g)[1 + ND][NR], float (&sq)[NT], float (&gc)[NC]) {
    float f[NF];
    fields(v, coef, f);
    {
#pragma clang fp contract(off)   // (no fusing of a square into the caller's running sum either)
      sq[0] = f[0] * f[0]; sq[1] = f[1] * f[1]; sq[2] = f[2] * f[2];
    }
    gc[0] = 0.f;
    if (GRAD) {
      const float H = v[0][0] + v[0][1], Hx = v[2][0] + v[2][1], Hy = v[3][0] + v[3][1];
      const float rc = 2.f * scale[0] * f[0], rx = 2.f * scale[1] * f[1], ry = 2.f * scale[2] * f[2];
      P::adjoint_cb(v, cb(coef), rc, rx, ry, g);
      gc[0] = (rx * Hx * H + ry * Hy * H) * ((float)(3.0 / 8.0 * 9.81) * coef[0]);   // d CB / d gamma_b = 3/8 g gamma_b
    }
  }
};

struct ResPhysicsEquationCoef {   // the plain residual (E == 0, physics.py:106); the corrected stress has no coefficient form
  typedef ResPhysicsEquation P;
  static constexpr int NR = P::NR, ND = P::ND, NT = P::NT, NF = P::NF, NC = 1;
  static constexpr float DEFAULTS[NC] = {0.002f};
  __host__ __device__ static inline float rho_cd(const float* coef) { return 1025.f * coef[0]; }   // physics.py:102-103
  __host__ __device__ static inline void fields(const float (&v)[1 + ND][NR], const float* coef, float (&f)[NF]) {
    P::fields_rc_strict(v, rho_cd(coef), f);
  }
  template <bool GRAD>
  __host__ __device__ static inline void eval(const float (&v)[1 + ND][NR], const float* coef, const float* scale,
                                              float (&g)[1 + ND][NR], float (&sq)[NT], float (&gc)[NC]) {
    float f[NF];
    fields(v, coef, f);
    {
#pragma clang fp contract(off)   // (no fusing of a square into the caller's running sum either)
      sq[0] = f[0] * f[0]; sq[1] = f[1] * f[1]; sq[2] = f[2] * f[2];
    }
    gc[0] = 0.f;
    if (GRAD) {
      const float h = v[0][0], U = v[0][1], V = v[0][2], eta = v[0][3];
      const float RHO = 1025.f;
      const float D = 1.0f / (RHO * (eta + h));
      const float rc = 2.f * scale[0] * f[0], rx = 2.f * scale[1] * f[1], ry = 2.f * scale[2] * f[2];
      P::adjoint_rc(v, rho_cd(coef), rc, rx, ry, g);
      gc[0] = D * RHO * (rx * (U * fabsf(U)) + ry * (V * fabsf(V)));   // d tau_b / d Cd = rho U|U|
    }
  }
};

// ---- second order: lateral mixing nu * lap(U) in the momentum equations --------------------------------------------
// The momentum fields of Navier_Stokes and physics_equation (plain and corrected) with the eddy-viscosity closure
//   fm_x -> fm_x - nu (u_xx + u_yy),   fm_y -> fm_y - nu (v_xx + v_yy)        (fc unchanged)
// written on the first-order jet v[1 + ND][NR] plus the two Laplacians lap = (L_u, L_v) of the momentum roles: the
// caller forms them from whatever pair layout it carries.  Adjoint: the first-order one with rx = 2 scale[1] fx and
// ry = 2 scale[2] fy of the SHIFTED fields, and glap = (-nu rx, -nu ry), which the caller puts on the (x, x) and (y, y)
// pairs of role u and of role v; every other second-order adjoint is zero.
// Each base IS its first-order struct — its fields and its adjoint(rc, rx, ry), so without ResPhysicsEquation::eval's NaN
// carrier — and adds only which roles carry the momentum and which directions are x and y.
struct Res2NavierStokes : ResNavierStokes { static constexpr int RU = 2, RV = 3, DX = 1, DY = 2; };
struct Res2PhysicsEquation : ResPhysicsEquation { static constexpr int RU = 1, RV = 2, DX = 0, DY = 1; };
struct Res2PhysicsEquationCorrected : ResPhysicsEquationCorrected { static constexpr int RU = 1, RV = 2, DX = 0, DY = 1; };

// f <- the shifted fields; with GRAD also g <- sum_t scale[t] d(f_t^2) / dv and glap <- (-nu rx, -nu ry)
template <class B>
struct Residual2 {
  static constexpr int NR = B::NR, ND = B::ND, NT = B::NT, NF = B::NF;
  __host__ __device__ static inline void fields(const float (&v)[1 + ND][NR], const float (&lap)[2], float nu,
                                                float (&f)[NF]) {
    B::fields(v, typename B::Closure(), f);
    f[1] = f[1] - nu * lap[0];
    f[2] = f[2] - nu * lap[1];
  }
  template <bool GRAD>
  __host__ __device__ static inline void eval(const float (&v)[1 + ND][NR], const float (&lap)[2], float nu,
                                              const float* scale, float (&f)[NF], float (&g)[1 + ND][NR],
                                              float (&glap)[2]) {
    fields(v, lap, nu, f);
    if (GRAD) adjoint(v, f, nu, scale, g, glap);
  }
  // the adjoint from fields already formed (k2_residual: one copy of the field arithmetic, with or without a gradient)
  __host__ __device__ static inline void adjoint(const float (&v)[1 + ND][NR], const float (&f)[NF], float nu,
                                                 const float* scale, float (&g)[1 + ND][NR], float (&glap)[2]) {
    const float rc = 2.f * scale[0] * f[0], rx = 2.f * scale[1] * f[1], ry = 2.f * scale[2] * f[2];
    B::adjoint(v, rc, rx, ry, g);
    glap[0] = -nu * rx;
    glap[1] = -nu * ry;
  }
};

// ---- inputs ---------------------------------------------------------------------------------------------------------------
// An input of +-inf as +-FLT_MAX, everything else (NaN included) unchanged: what the MFMA kernels hand X to layer 0 through.
// Their hidden layers are padded to a multiple of 16 units with zero weights, and 0 * inf = NaN in a padded unit of layer 0
// would spread to every real unit of layer 1 (0 * NaN), although the network itself saturates: tanh(w * inf) = +-1 and the
// row is finite (oracle, generic and wide engine; tests/test_nonfinite_gpu.py).  w * FLT_MAX saturates tanh_f32 the same way
// for every normal w; a NaN must NOT be caught here (fmin / fmax / med3 would drop it).  In integers, without a compare (the
// width-64 kernels spill scalar registers already, and a compare's mask is one more): t = 0 for an infinity and 1 otherwise,
// and bits + t - 1 steps an infinity down to the largest finite pattern of its sign and leaves everything else alone.
__device__ __forceinline__ float finite_input(float x) {
  const unsigned b = __float_as_uint(x);
  const unsigned t = min((b & 0x7fffffffu) ^ 0x7f800000u, 1u);
  return __uint_as_float(b + t - 1u);
}

// ---- activations (dnn.py:18-21) ------------------------------------------------
// tanh: odd minimax polynomial below 0.625, the exponential form above.  Measured over all 2^32 inputs against fp64
// (tests/test_devmath_gpu.py): relative error <= 7.61e-8 below 0.625 (subnormals included), absolute error
// <= 9.70e-8 everywhere (asserted: 1.0e-7 and 1.5e-7); monotonic from one bit pattern to the next; |tanh_f32| <= 1, so that
// s = 1 - a^2 >= 0 in every caller; +-inf -> +-1, NaN -> NaN.  The sign goes on LAST, on whichever branch was taken: both
// branches are sign-symmetric in magnitude, so tanh_f32(-x) = -tanh_f32(x) bit for bit, -0 included (the polynomial alone
// gives fma(-0, -0, -0) = +0 there).
__device__ inline float tanh_f32(float x) {
  const float ax = fabsf(x);
  const float x2 = x * x;
  float p = -5.70498872745e-3f;
  p = fmaf(p, x2, 2.06390887954e-2f);
  p = fmaf(p, x2, -5.37397155531e-2f);
  p = fmaf(p, x2, 1.33314422036e-1f);
  p = fmaf(p, x2, -3.33332819422e-1f);
  const float small = fmaf(p * x2, x, x);
  // 1 - 2/(exp(2|x|)+1); exp2 argument clamps naturally (inf -> 1)
  const float e = __expf(2.f * ax);
  const float big = fmaf(-2.f, __builtin_amdgcn_rcpf(e + 1.f), 1.f);   // v_rcp_f32: 1 ulp
  return copysignf(ax < 0.625f ? small : big, x);
}

// Two tanh_f32 evaluations on one register pair, every fp32 operation written on the pair (v_pk_mul_f32 / v_pk_fma_f32 /
// v_pk_add_f32): per element the same operations in the same order as tanh_f32, so each half is bitwise tanh_f32 of its
// input (all 2^32 patterns through either half: tests/test_devmath_gpu.py).  The one liberty: |x| is taken BEHIND the
// doubling and the multiply by log2(e) instead of in front of them — both are sign-symmetric, the magnitudes are the same
// bits — so that these two run packed (packed fp32 has no |.| modifier; v_exp_f32 has).  __expf(y) is
// v_exp_f32(y * log2(e)) with exactly this constant (0x3fb8aa3b).
typedef float f2 __attribute__((ext_vector_type(2)));
__device__ inline f2 tanh_f32x2(f2 x) {
  const f2 x2 = x * x;
  f2 p = f2{-5.70498872745e-3f, -5.70498872745e-3f};
  p = __builtin_elementwise_fma(p, x2, f2{2.06390887954e-2f, 2.06390887954e-2f});
  p = __builtin_elementwise_fma(p, x2, f2{-5.37397155531e-2f, -5.37397155531e-2f});
  p = __builtin_elementwise_fma(p, x2, f2{1.33314422036e-1f, 1.33314422036e-1f});
  p = __builtin_elementwise_fma(p, x2, f2{-3.33332819422e-1f, -3.33332819422e-1f});
  const f2 small = __builtin_elementwise_fma(p * x2, x, x);
  const f2 t = (x + x) * f2{0x1.715476p+0f, 0x1.715476p+0f};                    // +-(2|x|) log2(e)
  const f2 e = f2{__builtin_amdgcn_exp2f(fabsf(t[0])), __builtin_amdgcn_exp2f(fabsf(t[1]))};
  const f2 d = e + f2{1.f, 1.f};
  const f2 r = f2{__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])};
  const f2 big = __builtin_elementwise_fma(f2{-2.f, -2.f}, r, f2{1.f, 1.f});
  return f2{copysignf(fabsf(x[0]) < 0.625f ? small[0] : big[0], x[0]),
            copysignf(fabsf(x[1]) < 0.625f ? small[1] : big[1], x[1])};
}

// sin z and cos z together for the sine first layer (PINN_ACT_SIN_TANH), from z in DOUBLE.  A Fourier layer's arguments reach
// tens to a few hundred, where (a) the hardware sine (v_sin_f32 / __sinf, input in revolutions) has lost most of its bits and
// (b) an fp32 z itself is the largest error there is: one rounding of z = 8 is 5e-7 of sin z, of z = 256 it is 1.5e-5, whatever
// evaluates the sine afterwards (measured on a one-point Navier_Stokes sum of a 3 -> 10 -> 4 network: 3.3e-6 relative with z_0
// formed by the fp32 fmaf chain, 2.9e-7 with z_0 exact).  So the callers form z_0 = W_0 x + b_0 in double — the products of
// fp32 numbers are exact there — and the reduction r = z - k pi/2 is one double fused multiply-add; then the Cephes
// single-precision minimax polynomials on |r| <= pi/4 in fp32 and the quadrant swap.  No table, no branch, no scratch.
// Two roundings are carried along exactly, rl = the double r minus its fp32 rounding and res = (1 - w) - h for
// w = fl(1 - h), h = r^2 / 2, and
//   sin(r + rl) = r + [r^3 ps + rl],   cos(r + rl) = w + [res + r^4 pc - rl r]
// add the small bracket to the large term in one final rounding (with r, 1 - h and the result each rounded the figure is
// 9.25e-8).  Every product is an operand of an explicit fmaf or stands alone, so no contraction can change a rounding: the
// numpy restatement in tests/devmath_util.py is this function bit for bit.  Absolute error <= 7e-8 for both against fp64,
// measured 5.5e-8, on every fp32 z with |z| <= 1024, on doubles up to 2^16 and beside every quadrant
// boundary k pi/2 up to k = 2^20.  Beyond 2^26 the double pi/2's own error (6.1e-17 k) grows into it; from |z| = 2^31 on the
// quadrant count leaves int and the result is meaningless (|sn|, |cs| <= 1 holds up to 2^30).  NaN and +-inf give NaN.
__device__ inline void sincos_f64arg(double z, float& sn, float& cs) {
  const double k = rint(z * 0.63661977236758134308);
  const double rd = fma(-k, 1.57079632679489661923, z);
  const float r = (float)rd;
  const float rl = (float)(rd - (double)r);
  const float r2 = r * r;
  float ps = -1.9515295891e-4f;
  ps = fmaf(ps, r2, 8.3321608736e-3f);
  ps = fmaf(ps, r2, -1.6666654611e-1f);
  const float s = r + fmaf(ps * r2, r, rl);
  float pc = 2.443315711809948e-5f;
  pc = fmaf(pc, r2, -1.388731625493765e-3f);
  pc = fmaf(pc, r2, 4.166664568298827e-2f);
  const float h = 0.5f * r2, w = 1.f - h, res = (1.f - w) - h;
  const float c = w + fmaf(-rl, r, fmaf(pc * r2, r2, res));
  const int n = (int)k;
  const float s1 = (n & 1) ? c : s, c1 = (n & 1) ? s : c;
  sn = (n & 2) ? -s1 : s1;
  cs = ((n + 1) & 2) ? -c1 : c1;
}
// z_0 of one unit in double: b + sum_i w[i] x[i], d_in terms (w: the unit's row of W_0, x: the point's row of X)
__device__ inline double sin_layer_z(const float* __restrict__ w, float b, const float* __restrict__ x, int d_in) {
  double z = (double)b;
  for (int i = 0; i < d_in; ++i) z = fma((double)w[i], (double)x[i], z);
  return z;
}

// ---- point weights (pinn_residual_weighted_loss_grad) ---------------------------------------------------------------------
// The value of x behind a barrier the optimiser cannot see through.  The weighted kernels form the fields that go into the
// sums (and into the optional field store) from opaque copies of the jet and take them out through it again: that piece of
// arithmetic then has no operand in common with the adjoint's, so it is contracted into fused multiply-adds the same way in
// the forward-only and in the gradient instance, and a forward-only call returns the gradient call's term sums bit for bit.
// (Measured without it: eval<false> and eval<true> of ResNavierStokes rounded fc differently in the generic kernel.)
__device__ __forceinline__ float opaque(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(x));
#endif
  return x;
}
// the signed fields f[NF] of one point from its jet v, through the barrier on both sides
template <class RES>
__device__ __forceinline__ void isolated_fields(const float (&v)[1 + RES::ND][RES::NR], const typename RES::Closure& cl,
                                                float (&f)[RES::NF]) {
  float vb[1 + RES::ND][RES::NR];
#pragma unroll
  for (int c = 0; c <= RES::ND; ++c)
#pragma unroll
    for (int r = 0; r < RES::NR; ++r) vb[c][r] = opaque(v[c][r]);
  RES::fields(vb, cl, f);
#pragma unroll
  for (int t = 0; t < RES::NF; ++t) f[t] = opaque(f[t]);
}

}  // namespace pinn
