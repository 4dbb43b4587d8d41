// Placement probe for the mixed-width decode GEMM grid (gemm.hip gemm_tile_mixed_kernel): the
// same launch shape (256 threads and 72 KiB of LDS per workgroup, so two fit a CU; `nwide` wide
// column tiles first in launch order, the narrow ones after them), each workgroup streaming its
// rows of a row-major [N, K] bf16 weight once, as the GEMM's weight DMA does. Every workgroup
// records where it ran: rec[blockIdx] = {XCC id, HW_ID bits (SE / SH / CU), width, 0}.
#include <hip/hip_runtime.h>

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int kLdsBytes = 72 * 1024;

extern "C" __global__ void __launch_bounds__(256)
placement(const u32x4* __restrict__ w, int K, int nwide, int wide, int narrow, int4* __restrict__ rec,
          unsigned* __restrict__ sink) {
  __shared__ unsigned lds[kLdsBytes / 4];
  const int b = blockIdx.x;
  const bool is_wide = b < nwide;
  const int width = is_wide ? wide : narrow;
  const int n0 = is_wide ? b * wide : nwide * wide + (b - nwide) * narrow;
  unsigned xcc, hw;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
  const long ld16 = K / 8;                       // 16-byte chunks per row
  const int per_step = width * 8;                // chunks of a [width x 64] K step
  unsigned acc = 0;
  for (int k0 = 0; k0 < K / 64; ++k0)
    for (int c = threadIdx.x; c < per_step; c += 256) {
      const u32x4 v = __builtin_nontemporal_load(w + (long)(n0 + (c >> 3)) * ld16 + k0 * 8 + (c & 7));
      acc ^= v.x ^ v.y ^ v.z ^ v.w;
    }
  lds[(threadIdx.x + acc) % (kLdsBytes / 4)] = acc;   // keeps the loads and the LDS footprint live
  __syncthreads();
  if (lds[threadIdx.x] == 0x9e3779b9u) sink[b] = acc;  // practically never
  if (threadIdx.x == 0) rec[b] = int4{(int)(xcc & 15), (int)((hw >> 8) & 0xff), width, 0};
}
