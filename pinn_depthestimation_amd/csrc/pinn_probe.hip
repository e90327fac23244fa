// pinn_probe.hip — TEST-ONLY probe of the hand-written device math (libpinn_probe.so, never linked into libpinn_hip.so).
//
// It includes the kernel headers and calls their helpers AS THEY STAND — tanh_f32, tanh_f32x2, sincos_f64arg, sin_layer_z
// (residuals.h), tanh_bf (chain_kernel.h), to_bf16x4 / from_bf16x4 (wide_kernel.h) — so that tests/test_devmath_gpu.py can
// hold each one's accuracy claim over ALL fp32 bit patterns against the device library's fp64 functions.  Three exports
// (bound by ctypes in tests/devmath_util.py; every pointer is a HOST pointer, the probe stages the data itself):
//   probe_eval(fn, x, n, y)                   the helper element-wise on caller data
//   probe_ref (fn, x, n, y64)                 the fp64 reference the scans use, on the same data
//   probe_scan(fn, first_bits, count, table)  helper and reference at `count` consecutive fp32 bit patterns, reduced on the
//                                             device to one row per (sign, exponent) binade
// Nothing here is part of the product ABI (include/pinn_hip.h).
#include <vector>
#include "chain_kernel.h"

namespace {
using namespace pinn;

enum : int { FN_TANH_F32 = 0, FN_TANH_F32X2 = 1, FN_TANH_BF = 2, FN_SINCOS = 3, FN_TO_BF16 = 4, FN_FROM_BF16 = 5, FN_SIN_Z = 6, FN_COUNT = 7 };

// ---- table rows: 16 unsigned 64-bit slots per (sign, exponent) binade; the maxima are fp64 values >= 0 kept as their bits
// (for such values the order of the bits is the order of the values, and a NaN error sorts above everything: it cannot hide)
constexpr int ROW = 16;                      // (512 rows: pattern >> 23)
constexpr int S_COUNT = 0;                    // patterns visited
constexpr int S_ABS = 1, S_ABS_AT = 2;        // max |helper - ref| over finite inputs (sincos: of the sine) and where
constexpr int S_REL = 3, S_REL_AT = 4;        // max |helper - ref| / |ref| (tanh_f32: over |x| < 0.625 only, the claim's domain)
constexpr int S_AUX = 5, S_AUX_AT = 6;        // sincos: max abs error of the cosine; tanh_f32: largest backward step |f(prev)| - |f(x)|
constexpr int S_COUNT2 = 7;                   // tanh_f32x2: patterns visited by the second half
constexpr int S_VIOL = 8;                     // 8 counters of broken invariants, meaning per function (tests/devmath_util.py)
constexpr int CHUNK_LOG2 = 16, CHUNK = 1 << CHUNK_LOG2, THREADS = 256;   // patterns per workgroup: inside ONE binade (2^23)

__device__ __forceinline__ float f_of(unsigned b) { return __uint_as_float(b); }
__device__ __forceinline__ unsigned b_of(float f) { return __float_as_uint(f); }
__device__ __forceinline__ bool nan_bits(unsigned b) { return (b & 0x7fffffffu) > 0x7f800000u; }
__device__ __forceinline__ bool inf_bits(unsigned b) { return (b & 0x7fffffffu) == 0x7f800000u; }
// plain integer round-to-nearest-even of an fp32 pattern to bf16 (the caller keeps NaN out)
__host__ __device__ inline unsigned bf16_rne(unsigned b) { return (b + 0x7fffu + ((b >> 16) & 1u)) >> 16; }

struct Acc {
  unsigned long long count = 0, count2 = 0, m_abs = 0, m_rel = 0, m_aux = 0;
  unsigned a_abs = 0, a_rel = 0, a_aux = 0;
  unsigned viol[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  __device__ __forceinline__ static void up(unsigned long long& m, unsigned& at, double e, unsigned bits) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(e) & 0x7fffffffffffffffull;
    if (b > m) { m = b; at = bits; }
  }
};

template <int FN>
__device__ __forceinline__ void visit(unsigned bits, Acc& A) {
  const float x = f_of(bits);
  const bool isn = nan_bits(bits), isi = inf_bits(bits);
  if constexpr (FN == FN_TANH_F32) {
    A.count += 1;
    const float y = tanh_f32(x);
    if (isn) { A.viol[4] += !nan_bits(b_of(y)); return; }
    A.viol[0] += b_of(tanh_f32(-x)) != (b_of(y) ^ 0x80000000u);
    A.viol[1] += !(fabsf(y) <= 1.f);
    if ((bits & 0x7fffffffu) == 0) A.viol[2] += b_of(y) != bits;
    if (isi) { A.viol[3] += b_of(y) != ((bits & 0x80000000u) | 0x3f800000u); return; }
    const double r = tanh((double)x), e = fabs((double)y - r);
    Acc::up(A.m_abs, A.a_abs, e, bits);
    if (fabsf(x) < 0.625f && r != 0.0) Acc::up(A.m_rel, A.a_rel, e / fabs(r), bits);
    if ((bits & 0x7fffffffu) != 0) {      // the neighbour one pattern closer to zero must not be larger in magnitude
      const double back = (double)fabsf(tanh_f32(f_of(bits - 1))) - (double)fabsf(y);
      if (back > 0.0) Acc::up(A.m_aux, A.a_aux, back, bits);
    }
  } else if constexpr (FN == FN_TANH_F32X2) {
    A.count += 1; A.count2 += 1;
    const unsigned other = __brev(bits);          // the second half walks the whole domain too, in bit-reversed order
    const f2 v = tanh_f32x2(f2{x, f_of(other)});
    const unsigned w0 = b_of(tanh_f32(x)), w1 = b_of(tanh_f32(f_of(other)));
    A.viol[0] += !(b_of(v[0]) == w0 || (nan_bits(b_of(v[0])) && nan_bits(w0)));
    A.viol[1] += !(b_of(v[1]) == w1 || (nan_bits(b_of(v[1])) && nan_bits(w1)));
  } else if constexpr (FN == FN_TANH_BF) {
    A.count += 1;
    const float y = tanh_bf(x);
    if (isn) { A.viol[4] += !nan_bits(b_of(y)); return; }
    A.viol[1] += !(fabsf(y) <= 1.f);
    if (isi) { A.viol[3] += !(y == copysignf(1.f, x)); return; }
    const double r = tanh((double)x), e = fabs((double)y - r);
    Acc::up(A.m_abs, A.a_abs, e, bits);
    if (r != 0.0) Acc::up(A.m_rel, A.a_rel, e / fabs(r), bits);
  } else if constexpr (FN == FN_SINCOS) {
    A.count += 1;
    float sn, cs;
    sincos_f64arg((double)x, sn, cs);
    if (isn || isi) { A.viol[4] += !(nan_bits(b_of(sn)) && nan_bits(b_of(cs))); return; }
    A.viol[1] += !(fabsf(sn) <= 1.f && fabsf(cs) <= 1.f);
    Acc::up(A.m_abs, A.a_abs, fabs((double)sn - sin((double)x)), bits);
    Acc::up(A.m_aux, A.a_aux, fabs((double)cs - cos((double)x)), bits);
  }
}

// to_bf16x4 / from_bf16x4 on the four patterns 4g .. 4g + 3, one per vector lane
__device__ __forceinline__ void visit_bf16(unsigned bits4, Acc& A) {
  const f4 v = {f_of(bits4), f_of(bits4 + 1), f_of(bits4 + 2), f_of(bits4 + 3)};
  const bf16x4 h = to_bf16x4(v);
  const f4 back = from_bf16x4(h);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned b = bits4 + j, hj = (unsigned)(unsigned short)h[j];
    A.count += 1;
    if (nan_bits(b)) A.viol[4] += !((hj & 0x7fffu) > 0x7f80u);      // a NaN stays a NaN; its payload is not compared
    else A.viol[0] += hj != bf16_rne(b);
    A.viol[1] += b_of(back[j]) != (hj << 16);
  }
}

template <int FN>
__global__ __launch_bounds__(THREADS) void k_scan(unsigned long long first, unsigned long long* __restrict__ wg_rows) {
  __shared__ unsigned long long row[ROW];
  const unsigned start = (unsigned)(first + (unsigned long long)blockIdx.x * CHUNK);
  if (threadIdx.x < ROW) row[threadIdx.x] = 0;
  __syncthreads();
  Acc A;
  if constexpr (FN == FN_TO_BF16) {
    for (unsigned i = threadIdx.x * 4; i < (unsigned)CHUNK; i += THREADS * 4) visit_bf16(start + i, A);
  } else {
    for (unsigned i = threadIdx.x; i < (unsigned)CHUNK; i += THREADS) visit<FN>(start + i, A);
  }
  // integer atomics on the workgroup's LDS row only; the rows of different workgroups are folded on the host
  atomicAdd(&row[S_COUNT], A.count);
  if (A.count2) atomicAdd(&row[S_COUNT2], A.count2);
  atomicMax(&row[S_ABS], A.m_abs);
  atomicMax(&row[S_REL], A.m_rel);
  atomicMax(&row[S_AUX], A.m_aux);
#pragma unroll
  for (int j = 0; j < 8; ++j) if (A.viol[j]) atomicAdd(&row[S_VIOL + j], (unsigned long long)A.viol[j]);
  __syncthreads();
  // whoever holds a maximum names its pattern (equal maxima: any of them)
  if (A.m_abs && A.m_abs == row[S_ABS]) row[S_ABS_AT] = A.a_abs;
  if (A.m_rel && A.m_rel == row[S_REL]) row[S_REL_AT] = A.a_rel;
  if (A.m_aux && A.m_aux == row[S_AUX]) row[S_AUX_AT] = A.a_aux;
  __syncthreads();
  if (threadIdx.x < ROW) wg_rows[(size_t)blockIdx.x * ROW + threadIdx.x] = row[threadIdx.x];
}

__global__ void k_eval(int fn, const void* __restrict__ xv, long long n, void* __restrict__ yv) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* xf = (const float*)xv;
  float* yf = (float*)yv;
  switch (fn) {
    case FN_TANH_F32: yf[i] = tanh_f32(xf[i]); break;
    case FN_TANH_F32X2: {   // pair (x[i], x[n-1-i]): y[i] <- first half, y[n+i] <- second half
      const f2 v = tanh_f32x2(f2{xf[i], xf[n - 1 - i]});
      yf[i] = v[0]; yf[n + i] = v[1];
    } break;
    case FN_TANH_BF: yf[i] = tanh_bf(xf[i]); break;
    case FN_SINCOS: {
      float sn, cs;
      sincos_f64arg(((const double*)xv)[i], sn, cs);
      yf[2 * i] = sn; yf[2 * i + 1] = cs;
    } break;
    case FN_TO_BF16: {      // the value sits in vector lane i & 3
      f4 v = {0.f, 0.f, 0.f, 0.f};
      v[i & 3] = xf[i];
      ((unsigned*)yv)[i] = (unsigned)(unsigned short)to_bf16x4(v)[i & 3];
    } break;
    case FN_FROM_BF16: {
      bf16x4 h = {0, 0, 0, 0};
      h[i & 3] = (short)(unsigned short)((const unsigned*)xv)[i];
      yf[i] = from_bf16x4(h)[i & 3];
    } break;
    case FN_SIN_Z: {        // records of 18 floats: w[8], x[8], b, d_in
      const float* r = xf + 18 * i;
      ((double*)yv)[i] = sin_layer_z(r, r[16], r + 8, (int)r[17]);
    } break;
  }
}

__global__ void k_ref(int fn, const void* __restrict__ xv, long long n, double* __restrict__ y) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  switch (fn) {
    case FN_TANH_F32: case FN_TANH_F32X2: case FN_TANH_BF: y[i] = tanh((double)((const float*)xv)[i]); break;
    case FN_SINCOS: { const double z = ((const double*)xv)[i]; y[2 * i] = sin(z); y[2 * i + 1] = cos(z); } break;
    case FN_TO_BF16: y[i] = (double)bf16_rne(((const unsigned*)xv)[i]); break;
    case FN_FROM_BF16: y[i] = (double)((((const unsigned*)xv)[i] & 0xffffu) << 16); break;
  }
}

size_t in_bytes(int fn, long long n) {
  return fn == FN_SINCOS ? 8 * (size_t)n : fn == FN_SIN_Z ? 72 * (size_t)n : 4 * (size_t)n;
}

// stage x, run, fetch y; every step checked, the two buffers always released
template <class L>
int staged(const void* x, size_t xb, void* y, size_t yb, L launch) {
  void *dx = nullptr, *dy = nullptr;
  int rc = 0;
  if (hipMalloc(&dx, xb ? xb : 1) != hipSuccess || hipMalloc(&dy, yb ? yb : 1) != hipSuccess) rc = -10;
  if (!rc && xb && hipMemcpy(dx, x, xb, hipMemcpyHostToDevice) != hipSuccess) rc = -11;
  if (!rc) {
    launch(dx, dy);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = -12;
  }
  if (!rc && yb && hipMemcpy(y, dy, yb, hipMemcpyDeviceToHost) != hipSuccess) rc = -13;
  if (dx) (void)hipFree(dx);
  if (dy) (void)hipFree(dy);
  return rc;
}
}  // namespace

extern "C" {

int probe_eval(int fn, const void* x, long long n, void* y) {
  if (fn < 0 || fn >= FN_COUNT || n < 0 || (n > 0 && (!x || !y))) return -1;
  if (n == 0) return 0;
  const size_t yb = (fn == FN_TANH_F32X2 || fn == FN_SINCOS || fn == FN_SIN_Z) ? 8 * (size_t)n : 4 * (size_t)n;
  return staged(x, in_bytes(fn, n), y, yb, [&](void* dx, void* dy) {
    hipLaunchKernelGGL(k_eval, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, fn, (const void*)dx, n, dy);
  });
}

int probe_ref(int fn, const void* x, long long n, double* y64) {
  if (fn < 0 || fn >= FN_SIN_Z || n < 0 || (n > 0 && (!x || !y64))) return -1;
  if (n == 0) return 0;
  const size_t yb = (fn == FN_SINCOS ? 16 : 8) * (size_t)n;
  return staged(x, in_bytes(fn, n), y64, yb, [&](void* dx, void* dy) {
    hipLaunchKernelGGL(k_ref, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, fn, (const void*)dx, n, (double*)dy);
  });
}

// table: N_BINADES rows of ROW slots, row = pattern >> 23; ACCUMULATED into (the caller zeroes it once and sends its slices).
// first_bits and count are multiples of 2^16, count at most 2^28 per call, the slice inside [0, 2^32).
int probe_scan(int fn, unsigned long long first_bits, unsigned long long count, unsigned long long* table) {
  if (fn < 0 || fn > FN_TO_BF16 || !table) return -1;
  if ((first_bits | count) & (CHUNK - 1) || count > (1ull << 28) || first_bits + count > (1ull << 32)) return -2;
  if (count == 0) return 0;
  const unsigned n_wg = (unsigned)(count >> CHUNK_LOG2);
  std::vector<unsigned long long> rows((size_t)n_wg * ROW);
  const int rc = staged(nullptr, 0, rows.data(), rows.size() * 8, [&](void*, void* dy) {
    unsigned long long* out = (unsigned long long*)dy;
    switch (fn) {
      case FN_TANH_F32: hipLaunchKernelGGL(k_scan<FN_TANH_F32>, dim3(n_wg), dim3(THREADS), 0, 0, first_bits, out); break;
      case FN_TANH_F32X2: hipLaunchKernelGGL(k_scan<FN_TANH_F32X2>, dim3(n_wg), dim3(THREADS), 0, 0, first_bits, out); break;
      case FN_TANH_BF: hipLaunchKernelGGL(k_scan<FN_TANH_BF>, dim3(n_wg), dim3(THREADS), 0, 0, first_bits, out); break;
      case FN_SINCOS: hipLaunchKernelGGL(k_scan<FN_SINCOS>, dim3(n_wg), dim3(THREADS), 0, 0, first_bits, out); break;
      default: hipLaunchKernelGGL(k_scan<FN_TO_BF16>, dim3(n_wg), dim3(THREADS), 0, 0, first_bits, out); break;
    }
  });
  if (rc) return rc;
  for (unsigned w = 0; w < n_wg; ++w) {
    const unsigned long long* r = &rows[(size_t)w * ROW];
    unsigned long long* t = table + (size_t)((first_bits + ((unsigned long long)w << CHUNK_LOG2)) >> 23) * ROW;
    t[S_COUNT] += r[S_COUNT];
    t[S_COUNT2] += r[S_COUNT2];
    for (int j = 0; j < 8; ++j) t[S_VIOL + j] += r[S_VIOL + j];
    for (int s : {S_ABS, S_REL, S_AUX})
      if (r[s] > t[s]) { t[s] = r[s]; t[s + 1] = r[s + 1]; }
  }
  return 0;
}

}  // extern "C"
