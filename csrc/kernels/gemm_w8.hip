// FP8 e4m3 weight-only ("W8A16") linear layers: quantise, native decode GEMM, dequantise.
//
//   code[n, k] = RNE_e4m3fn(w[n, k] / scale[n]),  scale[n] = absmax(w[n, :]) / 448  (1 if zero)
//   Y[m, n]    = scale[n] * sum_k X[m, k] * float(code[n, k])            (f32 accumulation)
//
// The format is OCP e4m3fn (torch.float8_e4m3fn, the KV cache's format: bfly_kv.h). e4m3 has 3
// mantissa bits, so widening a code to bf16 is exact and the GEMM runs the same bf16 MFMAs as
// gemm.hip on half the weight bytes; the per-row scale multiplies the f32 accumulators.
//
//  * quant_fp8_rows_kernel: one workgroup per weight row: absmax, scale, codes.
//  * wq_gemm_kernel<W8Fmt, MT, 2> (up to kW8NativeMaxRows rows, in 64-row tiles): the decode
//    GEMM skeleton of gemm_wq.inc on 128-wide K chunks, a 16-B load being 16 codes.
//    K permutation: a 16-B weight load of lane group g = lane >> 4 covers k = 64 q + 16 g + j
//    (j < 16) of the chunk, so one load instruction reads 64 contiguous bytes per row; MFMA
//    step (q, s) takes j = 8 s .. 8 s + 7 and reads the X fragment at the same k.
//  * gemm_wq_reduce_kernel: the split-K slab reduce of every weight-only format.
//  * dequant_fp8_kernel: codes (x scale) -> bf16 [N, K]. Prefill and every row count above
//    kW8NativeMaxRows widen the BARE codes into a scratch (exact in bf16), run the bf16 GEMMs of
//    gemm.hip on it and apply scale[n] (and SwiGLU) to the result in w8_scale_cols_kernel: the
//    scale multiplies the accumulated sum, as in the native kernel, where a scratch of
//    bf16(code * scale) would add a 2^-9 rounding to every weight.
#include "bfly_common.h"

#include <cstdio>
#include <cstdlib>
#include "bfly_kernels.h"
#include "bfly_kv.h"

namespace bfly {

#include "gemm_wq.inc"

// The native kernel tiles M over blockIdx.z in 64-row steps, re-streaming the codes per tile;
// row counts above this limit take the dequantise route (ops.linear_w8). Measured on the four
// Llama-3-70B projections (tools/w8_bench.py --route, profiles/w8): row-tiled native against
// dequantise at 128 rows 61 / 45 / 253 / 127 us against 90 / 72 / 473 / 229 us (QKV, O, gate/up,
// down), at 256 rows 106 / 72 / 483 / 229 against 102 / 84 / 520 / 273, at 512 rows
// 179 / 115 / 928 / 430 against 127 / 108 / 629 / 323.
constexpr int kW8NativeMaxRows = 256;

// ---------------------------------------------------------------------------------------
// Quantise / dequantise
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
quant_fp8_rows_kernel(const bf16* __restrict__ w, long ldw, int K, fp8_t* __restrict__ code,
                      float* __restrict__ scale) {
  __shared__ float red[4];
  const long n = blockIdx.x;
  const bf16* row = w + n * ldw;
  fp8_t* crow = code + n * (long)K;
  const bool vec = (K % 8 == 0) && (ldw % 8 == 0);
  float amax = 0.f;
  if (vec) {
    for (int k = threadIdx.x * 8; k < K; k += 256 * 8) {
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(row + k);
#pragma unroll
      for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(bf2f(v[j])));
    }
  } else {
    for (int k = threadIdx.x; k < K; k += 256) amax = fmaxf(amax, fabsf(bf2f(row[k])));
  }
  amax = wave_max(amax);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = amax;
  __syncthreads();
  amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  // absmax / 448 in double: the library is built with -ffast-math, under which an f32
  // division by a constant may become a multiply by its rounded reciprocal. The double
  // quotient (or product) rounds to the correctly rounded f32 quotient: amax has 8
  // significant bits, so amax / 7 is exact or has a period-3 binary expansion and is never
  // within 2^-50 of an f32 rounding tie.
  const float sc = amax > 0.f ? (float)((double)amax / 448.0) : 1.f;
  if (threadIdx.x == 0) scale[n] = sc;
  if (vec) {
    for (int k = threadIdx.x * 8; k < K; k += 256 * 8) {
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(row + k);
      u32x2 o;
      o[0] = fp8_pack4(bf2f(v[0]) / sc, bf2f(v[1]) / sc, bf2f(v[2]) / sc, bf2f(v[3]) / sc);
      o[1] = fp8_pack4(bf2f(v[4]) / sc, bf2f(v[5]) / sc, bf2f(v[6]) / sc, bf2f(v[7]) / sc);
      *reinterpret_cast<u32x2*>(crow + k) = o;
    }
  } else {
    for (int k = threadIdx.x; k < K; k += 256)
      crow[k] = (fp8_t)(fp8_pack4(bf2f(row[k]) / sc, 0.f, 0.f, 0.f) & 0xff);
  }
}

// out[n, k] = bf16(float(code[n, k]) * scale[n]); 16 codes per lane when K % 16 == 0.
// scale == nullptr: the bare codes, which bf16 holds exactly.
__global__ void __launch_bounds__(256)
dequant_fp8_kernel(const fp8_t* __restrict__ code, const float* __restrict__ scale, long N, int K,
                   bf16* __restrict__ out, long ldo) {
  if (K % 16 == 0) {
    const int per_row = K / 16;
    const long total = N * per_row;
    for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
      const long n = e / per_row;
      const int k = (int)(e % per_row) * 16;
      const u32x4 c = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(code + n * K + k));
      const float sc = scale ? scale[n] : 1.f;
      bf16x8 lo = KV<fp8_t>::widen(u32x2{c[0], c[1]});
      bf16x8 hi = KV<fp8_t>::widen(u32x2{c[2], c[3]});
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        lo[j] = f2bf(bf2f(lo[j]) * sc);
        hi[j] = f2bf(bf2f(hi[j]) * sc);
      }
      bf16* o = out + n * ldo + k;
      *reinterpret_cast<bf16x8*>(o) = lo;
      *reinterpret_cast<bf16x8*>(o + 8) = hi;
    }
  } else {
    const long total = N * K;
    for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
      const long n = e / K;
      const int k = (int)(e % K);
      const f32x2 f = __builtin_amdgcn_cvt_pk_f32_fp8((int)code[e], false);
      out[n * ldo + k] = f2bf(f[0] * (scale ? scale[n] : 1.f));
    }
  }
}

// The dequantise route's epilogue: y[M, N] = X . code^T from a bf16 GEMM over the bare codes
// -> out = (y * scale[n]), or its SwiGLU over the 16-row gate/up interleave. 8 output columns
// per lane; in place (out == y) for the plain epilogue.
__global__ void __launch_bounds__(256)
w8_scale_cols_kernel(const bf16* __restrict__ y, long ldy, const float* __restrict__ scale, int M, int N,
                     int epi, bf16* __restrict__ out, long ldo) {
  const int nout = epi == EPI_SILU ? N / 2 : N;
  const int per_row = nout / 8;
  const long total = (long)M * per_row;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long m = e / per_row;
    const int f = (int)(e % per_row) * 8;
    const int n = epi == EPI_SILU ? (f >> 4) * 32 + (f & 15) : f;
    const bf16x8 a = *reinterpret_cast<const bf16x8*>(y + m * ldy + n);
    const f32x4 s0 = *reinterpret_cast<const f32x4*>(scale + n);
    const f32x4 s1 = *reinterpret_cast<const f32x4*>(scale + n + 4);
    bf16x8 o;
    if (epi == EPI_SILU) {
      const bf16x8 b = *reinterpret_cast<const bf16x8*>(y + m * ldy + n + 16);
      const f32x4 u0 = *reinterpret_cast<const f32x4*>(scale + n + 16);
      const f32x4 u1 = *reinterpret_cast<const f32x4*>(scale + n + 20);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        o[j] = f2bf(silu(bf2f(a[j]) * s0[j]) * (bf2f(b[j]) * u0[j]));
        o[j + 4] = f2bf(silu(bf2f(a[j + 4]) * s1[j]) * (bf2f(b[j + 4]) * u1[j]));
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        o[j] = f2bf(bf2f(a[j]) * s0[j]);
        o[j + 4] = f2bf(bf2f(a[j + 4]) * s1[j]);
      }
    }
    *reinterpret_cast<bf16x8*>(out + m * ldo + f) = o;
  }
}

// ---------------------------------------------------------------------------------------
// Native decode GEMM
// ---------------------------------------------------------------------------------------
// The FP8 side of gemm_wq.inc's skeleton: chunks of 128 k, two 16-B loads per (chunk, row).
struct W8Fmt {
  static constexpr int Q = 1, kMaxRows = kW8NativeMaxRows, kLoads = 2, kSteps = 2;
  static constexpr bool kRowScale = true;
  using Scale = float;
  struct Regs { u32x4 c[2]; };   // codes k = 64 q + 16 g + j (j < 16) of the chunk

  static __device__ __forceinline__ int pitch(int K) { return K; }   // K code bytes per row

  template <int NT>
  static __device__ __forceinline__ void load(const uint8_t* __restrict__ W, const float*, long K, int n0,
                                              int kc, int lane, Regs (&a)[NT]) {
    const int g = lane >> 4, r = lane & 15;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const uint8_t* p = W + (long)(n0 + 16 * t + r) * K + (long)kc * kWqSub + 16 * g;
#pragma unroll
      for (int q = 0; q < 2; ++q)
        a[t].c[q] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p + 64 * q));
    }
  }

  static __device__ __forceinline__ int koff(int q, int s, int g) { return 64 * q + 16 * g + 8 * s; }
  static __device__ __forceinline__ float scale(const Regs&, int, int) { return 1.f; }   // unused
  static __device__ __forceinline__ bf16x8 frag(const Regs& a, int q, int s, float) {
    return KV<fp8_t>::widen(u32x2{a.c[q][2 * s], a.c[q][2 * s + 1]});
  }

  // 128 weight rows per workgroup (256-row workgroups measured no faster on any Llama-3-70B
  // projection at 1 - 64 rows, profiles/w8). Split K while the grid has at most 320 workgroups
  // (1.25 per CU), keeping >= 4 chunks per split: 70B QKV / O / down split 8 ways, gate/up (448
  // workgroups) not at all, which was the fastest split of each in the sweep.
  static int splitk(int, int, int blocks, int nchunks) {
    int sk = 1;
    while (blocks * sk <= 320 && nchunks >= 8 * sk && sk < 16) sk *= 2;
    return sk;
  }
};

// Sum the (already scaled) split-K slabs [SK][M][N] in a fixed order and apply the epilogue.
// Format-neutral: a slab holds final f32 sums (a format's scales are already in them), so
// every weight-only GEMM reduces through this kernel.
__global__ void __launch_bounds__(256)
gemm_wq_reduce_kernel(const float* __restrict__ part, int SK, int M, int N, int epi,
                      bf16* __restrict__ out, long ldo) {
  const int nout = epi == EPI_SILU ? N / 2 : N;
  const long total = (long)M * (nout / 4);
  const long slab = (long)M * N;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const int m = (int)(e / (nout / 4)), f = (int)(e % (nout / 4)) * 4;
    bf16x4 o;
    if (epi == EPI_SILU) {
      const long gi = (long)m * N + (f >> 4) * 32 + (f & 15);
      f32x4 gs = {0.f, 0.f, 0.f, 0.f}, us = {0.f, 0.f, 0.f, 0.f};
      for (int s = 0; s < SK; ++s) {
        gs += *reinterpret_cast<const f32x4*>(part + s * slab + gi);
        us += *reinterpret_cast<const f32x4*>(part + s * slab + gi + 16);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = f2bf(silu(gs[i]) * us[i]);
    } else {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      for (int s = 0; s < SK; ++s) v += *reinterpret_cast<const f32x4*>(part + s * slab + (long)m * N + f);
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = f2bf(v[i]);
    }
    *reinterpret_cast<bf16x4*>(out + (long)m * ldo + f) = o;
  }
}

// ---------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------
void launch_gemm_wq_reduce(const float* part, int sk, int M, int N, int epi, bf16* out, long ldo,
                           hipStream_t stream) {
  const long total = (long)M * ((epi == EPI_SILU ? N / 2 : N) / 4);
  if (total <= 0) return;
  gemm_wq_reduce_kernel<<<wq_grid(total, 4096), 256, 0, stream>>>(part, sk, M, N, epi, out, ldo);
}

int gemm_w8_check(int M, int N, int K, int epi) { return wq_check<W8Fmt>(M, N, K, epi); }
int gemm_w8_splitk(int M, int N, int K, int epi) { return wq_splitk<W8Fmt>(M, N, K, epi); }
size_t gemm_w8_workspace_bytes(int M, int N, int K) { return wq_workspace_bytes<W8Fmt>(M, N, K); }

int launch_gemm_w8(const bf16* X, long ldx, const uint8_t* W, const float* scale, int M, int N, int K,
                   int epi, bf16* out, long ldo, float* ws, size_t ws_bytes, hipStream_t stream,
                   bool any_m, int force_sk) {
  return wq_launch<W8Fmt>(X, ldx, W, scale, M, N, K, epi, out, ldo, ws, ws_bytes, stream, any_m, force_sk);
}

void launch_quant_fp8_rows(const bf16* w, long ldw, long N, int K, uint8_t* code, float* scale,
                           hipStream_t stream) {
  if (N <= 0 || K <= 0) return;
  quant_fp8_rows_kernel<<<(unsigned)N, 256, 0, stream>>>(w, ldw, K, code, scale);
}

void launch_dequant_fp8(const uint8_t* code, const float* scale, long N, int K, bf16* out, long ldo,
                        hipStream_t stream) {
  if (N <= 0 || K <= 0) return;
  const long total = K % 16 == 0 ? N * (K / 16) : N * (long)K;
  dequant_fp8_kernel<<<wq_grid(total), 256, 0, stream>>>(code, scale, N, K, out, ldo);
}

void launch_w8_scale_cols(const bf16* y, long ldy, const float* scale, int M, int N, int epi, bf16* out,
                          long ldo, hipStream_t stream) {
  if (M <= 0 || N <= 0) return;
  const long total = (long)M * ((epi == EPI_SILU ? N / 2 : N) / 8);
  w8_scale_cols_kernel<<<wq_grid(total), 256, 0, stream>>>(y, ldy, scale, M, N, epi, out, ldo);
}

}  // namespace bfly
