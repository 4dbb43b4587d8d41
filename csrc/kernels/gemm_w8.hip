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
//  * gemm_w8_kernel (up to kW8NativeMaxRows rows, in 64-row tiles): a workgroup of 4 waves
//    owns 64*NT (NT = 2) weight rows and one K range (split-K over blockIdx.y, f32 slabs +
//    gemm_w8_reduce_kernel). Each wave streams its
//    16*NT rows straight into VGPRs with non-temporal 16-B loads (16 codes), five 128-wide
//    K chunks ahead, and widens them in registers. The X rows of a chunk are shared by the 4
//    waves, so they are staged once per workgroup through a double-buffered LDS tile (X from L2
//    per wave would exceed the weight bytes at 64 rows). W is the MFMA A operand, as in
//    gemm_skinny_kernel: a lane holds 4 consecutive n of one token row.
//    K permutation: a 16-B weight load of lane group g = lane >> 4 covers k = 64 q + 16 g + j
//    (j < 16) of the chunk, so one load instruction reads 64 contiguous bytes per row; MFMA
//    step (q, s) takes j = 8 s .. 8 s + 7 and reads the X fragment at the same k.
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

constexpr int kW8Threads = 256;
constexpr int kW8Chunk = 128;        // K elements per pipeline step
constexpr int kW8XPitch = 272;       // bytes per X row in LDS: 256 + 16 (rows 4 banks apart)
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
template <int NT>
__device__ __forceinline__ void w8_load(const fp8_t* __restrict__ W, long K, int n0, int kc,
                                        int lane, u32x4 (&a)[NT][2]) {
  const int g = lane >> 4, r = lane & 15;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const fp8_t* p = W + (long)(n0 + 16 * t + r) * K + (long)kc * kW8Chunk + 16 * g;
#pragma unroll
    for (int q = 0; q < 2; ++q)
      a[t][q] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p + 64 * q));
  }
}

// The workgroup's 256 threads copy MT x 16 rows x 128 k of X: thread -> (row tid / 16, 16-B
// column tid % 16), one 256-B row per 16 lanes.
template <int MT>
__device__ __forceinline__ void w8_x_load(const bf16* __restrict__ X, long ldx, int m0, int M,
                                          int kc, bf16x8 (&xr)[MT]) {
  const int row = threadIdx.x >> 4, kb = threadIdx.x & 15;
#pragma unroll
  for (int p = 0; p < MT; ++p) {
    int m = m0 + 16 * p + row;
    m = m < M ? m : M - 1;
    xr[p] = *reinterpret_cast<const bf16x8*>(X + (long)m * ldx + (long)kc * kW8Chunk + 8 * kb);
  }
}

template <int MT>
__device__ __forceinline__ void w8_x_store(unsigned char* buf, const bf16x8 (&xr)[MT]) {
  const int row = threadIdx.x >> 4, kb = threadIdx.x & 15;
#pragma unroll
  for (int p = 0; p < MT; ++p)
    *reinterpret_cast<bf16x8*>(buf + (16 * p + row) * kW8XPitch + 16 * kb) = xr[p];
}

template <int MT, int NT>
__device__ __forceinline__ void w8_mma(const u32x4 (&a)[NT][2], const unsigned char* buf, int lane,
                                       f32x4 (&acc)[NT][MT]) {
  const int g = lane >> 4, r = lane & 15;
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8 b[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        b[mt] = *reinterpret_cast<const bf16x8*>(buf + (16 * mt + r) * kW8XPitch +
                                                 2 * (64 * q + 16 * g + 8 * s));
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const bf16x8 wa = KV<fp8_t>::widen(u32x2{a[t][q][2 * s], a[t][q][2 * s + 1]});
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[t][mt] = mfma16(wa, b[mt], acc[t][mt]);
      }
    }
}

template <int MT, int NT>
__global__ void __launch_bounds__(kW8Threads)
gemm_w8_kernel(const bf16* __restrict__ X, long ldx, const fp8_t* __restrict__ W,
               const float* __restrict__ scale, int M, int N, int K, int epi,
               bf16* __restrict__ out, long ldo, float* __restrict__ part) {
  constexpr int kBuf = MT * 16 * kW8XPitch;
  __shared__ __attribute__((aligned(16))) unsigned char xs[2 * kBuf];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int n0 = blockIdx.x * 64 * NT + wid * 16 * NT;
  const int m0 = blockIdx.z * 64;
  const int nchunks = K / kW8Chunk;
  const int S = gridDim.y;
  const int c0 = (int)(((long)nchunks * blockIdx.y) / S);
  const int c1 = (int)(((long)nchunks * (blockIdx.y + 1)) / S);

  f32x4 acc[NT][MT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[t][mt] = f32x4{0.f, 0.f, 0.f, 0.f};

  // A ring of R weight register sets: chunk s is consumed while s + 1 .. s + R - 1 are in flight
  // (R - 1 chunks of 16 NT rows x 128 B per wave cover the HBM latency with one workgroup per
  // CU). X goes L2 -> registers -> LDS: loaded three steps ahead, stored into the other LDS
  // buffer one step ahead. Every ring index below is a compile-time constant after unrolling
  // (runtime-indexed register arrays would go to scratch); the step count is uniform over the
  // workgroup, so every barrier is too. X loads are issued before the W loads of a step: memory
  // returns in order, and the X store of step s must not wait for the newest weights.
  constexpr int R = 6;
  u32x4 a[R][NT][2];
  bf16x8 xr[2][MT];
  const int n = c1 - c0;
  if (n > 0) w8_x_load<MT>(X, ldx, m0, M, c0, xr[0]);
  if (n > 1) w8_x_load<MT>(X, ldx, m0, M, c0 + 1, xr[1]);
#pragma unroll
  for (int j = 0; j < R - 1; ++j)
    if (j < n) w8_load<NT>(W, K, n0, c0 + j, lane, a[j]);
  if (n > 0) w8_x_store<MT>(xs, xr[0]);
  if (n > 2) w8_x_load<MT>(X, ldx, m0, M, c0 + 2, xr[0]);
  __syncthreads();
  for (int i = 0; i < n; i += R) {
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int s = i + j;                 // R is even: s and j have the same parity
      if (s >= n) break;
      if (s + 1 < n) w8_x_store<MT>(xs + ((j + 1) & 1) * kBuf, xr[(j + 1) & 1]);
      if (s + 3 < n) w8_x_load<MT>(X, ldx, m0, M, c0 + s + 3, xr[(j + 1) & 1]);
      if (s + R - 1 < n) w8_load<NT>(W, K, n0, c0 + s + R - 1, lane, a[(j + R - 1) % R]);
      w8_mma<MT, NT>(a[j], xs + (j & 1) * kBuf, lane, acc);
      __syncthreads();
    }
  }

  // Epilogue: lane (g, r) holds n = n0 + 16 t + 4 g + i (i < 4) of token row m0 + 16 mt + r.
  const int g = lane >> 4, r = lane & 15;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const f32x4 sc = *reinterpret_cast<const f32x4*>(scale + n0 + 16 * t + 4 * g);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[t][mt] *= sc;
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int m = m0 + 16 * mt + r;
    if (m >= M) continue;
    if (part) {
#pragma unroll
      for (int t = 0; t < NT; ++t)
        *reinterpret_cast<f32x4*>(part + ((long)blockIdx.y * M + m) * N + n0 + 16 * t + 4 * g) = acc[t][mt];
    } else if (epi == EPI_SILU) {
#pragma unroll
      for (int t = 0; t < NT; t += 2) {   // gate tile t, up tile t + 1: same lane, same i
        bf16x4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = f2bf(silu(acc[t][mt][i]) * acc[t + 1][mt][i]);
        *reinterpret_cast<bf16x4*>(out + (long)m * ldo + n0 / 2 + 8 * t + 4 * g) = o;
      }
    } else {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        bf16x4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = f2bf(acc[t][mt][i]);
        *reinterpret_cast<bf16x4*>(out + (long)m * ldo + n0 + 16 * t + 4 * g) = o;
      }
    }
  }
}

// Sum the (already scaled) split-K slabs [SK][M][N] in a fixed order and apply the epilogue.
__global__ void __launch_bounds__(256)
gemm_w8_reduce_kernel(const float* __restrict__ part, int SK, int M, int N, int epi,
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
void launch_gemm_w8_reduce(const float* part, int sk, int M, int N, int epi, bf16* out, long ldo,
                           hipStream_t stream) {
  const long total = (long)M * ((epi == EPI_SILU ? N / 2 : N) / 4);
  if (total <= 0) return;
  long grid = (total + 255) / 256;
  if (grid > 4096) grid = 4096;
  gemm_w8_reduce_kernel<<<(int)grid, 256, 0, stream>>>(part, sk, M, N, epi, out, ldo);
}

struct W8Plan { int mt, nt, sk; };

// Shape contract: N % 128 == 0, K % 128 == 0, epilogue none / SiLU. (`any_m`: skip the row limit.)
static bool w8_plan(int M, int N, int K, int epi, W8Plan& p, bool any_m = false) {
  if (M <= 0 || N <= 0 || K <= 0 || N % 128 != 0 || K % kW8Chunk != 0) return false;
  if (epi != EPI_NONE && epi != EPI_SILU) return false;
  if (!any_m && M > kW8NativeMaxRows) return false;
  p.mt = M >= 64 ? 4 : (M + 15) / 16;
  const int ztiles = (M + 63) / 64;
  const int nchunks = K / kW8Chunk;
  // 128 weight rows per workgroup (256-row workgroups measured no faster on any Llama-3-70B
  // projection at 1 - 64 rows, profiles/w8). Split K while the grid has at most 320 workgroups
  // (1.25 per CU), keeping >= 4 chunks per split: 70B QKV / O / down split 8 ways, gate/up (448
  // workgroups) not at all, which was the fastest split of each in the sweep.
  p.nt = 2;
  const int blocks = N / (64 * p.nt) * ztiles;
  int sk = 1;
  while (blocks * sk <= 320 && nchunks >= 8 * sk && sk < 16) sk *= 2;
  p.sk = sk;
  return true;
}

int gemm_w8_check(int M, int N, int K, int epi) {
  if (M <= 0) return 0;
  W8Plan p;
  return w8_plan(M, N, K, epi, p) ? 0 : -1;
}

int gemm_w8_splitk(int M, int N, int K, int epi) {
  W8Plan p;
  return w8_plan(M, N, K, epi, p, true) ? p.sk : 0;
}

size_t gemm_w8_workspace_bytes(int M, int N, int K) {
  W8Plan p;
  if (!w8_plan(M, N, K, EPI_NONE, p, true) || p.sk <= 1) return 0;
  return (size_t)p.sk * M * N * sizeof(float);
}

template <int MT, int NT>
static void run_w8(const bf16* X, long ldx, const fp8_t* W, const float* scale, int M, int N, int K,
                   int epi, bf16* out, long ldo, float* part, int sk, hipStream_t stream) {
  dim3 grid(N / (64 * NT), sk, (M + 63) / 64);
  gemm_w8_kernel<MT, NT><<<grid, kW8Threads, 0, stream>>>(X, ldx, W, scale, M, N, K, epi, out, ldo, part);
}

int launch_gemm_w8(const bf16* X, long ldx, const uint8_t* W, const float* scale, int M, int N, int K,
                   int epi, bf16* out, long ldo, float* ws, size_t ws_bytes, hipStream_t stream,
                   bool any_m, int force_sk) {
  if (M <= 0) return 0;
  W8Plan p;
  if (!w8_plan(M, N, K, epi, p, any_m)) return -1;
  if (force_sk > 0) {   // measurements (tools/w8_bench.py): another split than the heuristic's
    p.sk = force_sk;
    if (p.sk > K / kW8Chunk) return -2;
    if (p.sk > 1 && (ws == nullptr || ws_bytes < (size_t)p.sk * M * N * sizeof(float))) return -3;
  }
  if (p.sk > 1 && (ws == nullptr || ws_bytes < (size_t)p.sk * M * N * sizeof(float))) p.sk = 1;
  float* part = p.sk > 1 ? ws : nullptr;
#define W8_CASE(MT_, NT_)                                                                         \
  if (p.mt == MT_ && p.nt == NT_)                                                                 \
    run_w8<MT_, NT_>(X, ldx, W, scale, M, N, K, epi, out, ldo, part, p.sk, stream);
  W8_CASE(1, 2) W8_CASE(2, 2) W8_CASE(3, 2) W8_CASE(4, 2)
#undef W8_CASE
  if (part) launch_gemm_w8_reduce(part, p.sk, M, N, epi, out, ldo, stream);
  return 0;
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
  long grid = (total + 255) / 256;
  if (grid > 16384) grid = 16384;
  dequant_fp8_kernel<<<(int)grid, 256, 0, stream>>>(code, scale, N, K, out, ldo);
}

void launch_w8_scale_cols(const bf16* y, long ldy, const float* scale, int M, int N, int epi, bf16* out,
                          long ldo, hipStream_t stream) {
  if (M <= 0 || N <= 0) return;
  const long total = (long)M * ((epi == EPI_SILU ? N / 2 : N) / 8);
  long grid = (total + 255) / 256;
  if (grid > 16384) grid = 16384;
  w8_scale_cols_kernel<<<(int)grid, 256, 0, stream>>>(y, ldy, scale, M, N, epi, out, ldo);
}

}  // namespace bfly
