// pinn_fused_sin_w64_g4.hip — ONE instance of the fused tile kernel, alone in its translation unit: sine first layer, padded
// width 64, K1 = 4, gradient pass with the workgroup's gradient copy in global memory.  With -amdgpu-mfma-vgpr-form (the switch
// of the other width-64 translation units, Makefile) clang 22 crashes on it in its 'Rewrite AGPR-Copy-MFMA' pass
// (eliminateSpillsOfReassignedVGPRs) once the GEMM streams and the weight gradient issue their memory and LDS instructions
// from slots between the MFMAs (fused_kernel.h) — whatever the slot spacing, and with the pacing of this instance switched
// off as well: the same pass and the same family (width 64, K1 = 4, global gradient copy) as the two crashes recorded in
// DESIGN 3.3.  Built without the switch the instance keeps 208 bytes per lane in scratch memory (244 before, with it); its
// eight siblings stay in pinn_fused_sin_w64.hip and keep the switch (without it one of them would start to spill).
#include "fused_kernel.h"

namespace pinn {
template __global__ void k_fused<64, 4, true, false, PINN_ACT_SIN_TANH, EPI_GENERIC>(const FusedParams);
}  // namespace pinn
