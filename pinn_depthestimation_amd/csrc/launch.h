// launch.h — the library's one launch helper and its K1 dispatch, shared by the fused engine (fused_launch.h) and the wide
// and chain engines (wide_launch.h).  Host only: nothing here is seen by a kernel.
#pragma once
#include <type_traits>
#include "common.h"

namespace pinn {

// raise the kernel's dynamic-LDS limit if need be, launch with the kernel's arguments `args`, report a failed launch under `what`
template <class K, class... Args>
int launch_kernel(K kern, dim3 grid, int threads, size_t lds_bytes, hipStream_t s, const char* what, const Args&... args) {
  if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds_bytes)) return rc;
  hipLaunchKernelGGL(kern, grid, dim3(threads), lds_bytes, s, args...);
  return check_launch(what);
}

// f(std::integral_constant<int, K>) for the K of KS that equals K1; NO_INSTANCE if none does
constexpr int NO_INSTANCE = -(1 << 20);
template <int... KS, class F>
int with_k1(int K1, F f) {
  int rc = NO_INSTANCE;
  (void)((K1 == KS && (rc = f(std::integral_constant<int, KS>{}), true)) || ...);
  return rc;
}

}  // namespace pinn
