// OCP MXFP4 weight-only ("W4A16") linear layers: quantise, native decode GEMM, dequantise.
//
//   block b of row n: k = 32 b .. 32 b + 31, amax = max |w[n, k]|
//   E          = clamp(floor(log2(amax)) - 2, -125, 125)   (0 for an all-zero block)
//   scale[n,b] = uint8(E + 127)                            (e8m0)
//   code[n,k]  = RNE_e2m1(w[n, k] / 2^E), saturating at +-6; grid {0, .5, 1, 1.5, 2, 3, 4, 6},
//                bit 3 the sign; element 2 i in the low nibble of byte i, 2 i + 1 in the high one
//   Y[m, n]    = sum_k X[m, k] * value(code[n, k]) * 2^E   (f32 accumulation, one rounding)
//
// A dequantised weight has two significant bits and, with E clamped, a normal bf16 exponent: it
// is exact in bf16. So the GEMM is gemm.hip's bf16 GEMM on the dequantised matrix, with no scale
// left for the accumulators or the result, and every step of the quantiser is exact too (the
// exponent comes from the bf16 bits, the division is a multiplication by a power of two).
//
//  * quant_mxfp4_kernel: one lane per 32-element block: amax, scale byte, 16 B of codes.
//  * dequant_mxfp4_kernel: one lane per block: a 16-B code load, one scale byte, 64 B of bf16.
//  * wq_gemm_kernel<W4Fmt<Q>, MT, 2> (up to kW4NativeMaxRows rows, in 64-row tiles): the decode
//    GEMM skeleton of gemm_wq.inc (split-K slabs reduced by gemm_wq_reduce_kernel). A 16-B load
//    is 32 codes = one scale block; they are converted in registers with
//    v_cvt_scalef32_pk_bf16_fp4 (two codes and their scale -> two bf16 per instruction).
//    A chunk is Q sub-chunks of 128 k (Q = 2 when K % 256 == 0, else 1): per row, Q loads 64 B
//    apart, so a load instruction reads 64 contiguous bytes per row and a chunk 64 Q.
//    K permutation: lane group g = lane >> 4 loads block g of sub-chunk q, k = 128 q + 32 g + j
//    (j < 32); MFMA step (q, s), s < 4, takes the lane's codes j = 8 s .. 8 s + 7 (dword s) and
//    reads the X fragment at the same k. The four scale bytes of a (row, sub-chunk) are one
//    aligned dword: loaded once per lane, byte g extracted, 2^E formed as byte << 23.
#include "bfly_common.h"

#include "bfly_kernels.h"

namespace bfly {

#include "gemm_wq.inc"   // a sub-chunk (kWqSub = 128 k) is 4 scale blocks, 64 code bytes

// The native kernel tiles M over blockIdx.z in 64-row steps, re-streaming the codes per tile;
// row counts above this limit dequantise into the arena scratch and run the bf16 GEMM
// (ops.linear_w4). tools/w4_bench.py --route compares the two routes (profiles/w4).
constexpr int kW4NativeMaxRows = 256;

// 2^(biased - 127) for biased in 1 .. 254. The quantiser writes scale bytes 2 .. 252 only; 0
// would give 0 and 255 infinity where the format means 2^-127 and NaN, so those are invalid input.
__device__ __forceinline__ float pow2_bits(int biased) { return __uint_as_float((uint32_t)biased << 23); }

// ---------------------------------------------------------------------------------------
// Quantise / dequantise
// ---------------------------------------------------------------------------------------
// |w| / 2^E of one bf16 (15 magnitude bits `h`), exactly. A subnormal bf16 (m * 2^-133) goes
// through an integer conversion so that the result does not depend on the f32 denormal mode;
// above E = -7 it would be below 2^-120 and quantises to zero.
__device__ __forceinline__ float w4_scaled(uint32_t h, int E, float inv) {
  if (h >> 7) return __uint_as_float(h << 16) * inv;
  return E <= -7 ? (float)h * pow2_bits(-6 - E) : 0.f;
}

// RNE onto the e2m1 grid as a count of passed midpoints; a tie goes to the even code, so the
// midpoints below an even code are inclusive. Saturates at 6 (code 7).
__device__ __forceinline__ uint32_t w4_code(float t) {
  return (uint32_t)(t > .25f) + (uint32_t)(t >= .75f) + (uint32_t)(t > 1.25f) + (uint32_t)(t >= 1.75f) +
         (uint32_t)(t > 2.5f) + (uint32_t)(t >= 3.5f) + (uint32_t)(t > 5.f);
}

__global__ void __launch_bounds__(256)
quant_mxfp4_kernel(const bf16* __restrict__ w, long ldw, long N, int K, uint8_t* __restrict__ code,
                   uint8_t* __restrict__ scale) {
  const int nb = K / 32;
  const long total = N * nb;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long n = e / nb;
    const int b = (int)(e % nb);
    const u32x4* src = reinterpret_cast<const u32x4*>(w + n * ldw + 32 * b);
    u32x4 v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = src[i];
    uint32_t amax = 0;   // magnitude bits order like the values
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t lo = v[i][j] & 0x7fffu, hi = (v[i][j] >> 16) & 0x7fffu;
        amax = amax > lo ? amax : lo;
        amax = amax > hi ? amax : hi;
      }
    int E = (int)(amax >> 7) - 129;   // exponent field - 127 = floor(log2), minus e2m1's largest exponent
    E = E < -125 ? -125 : (E > 125 ? 125 : E);
    if (amax == 0) E = 0;
    const float inv = pow2_bits(127 - E);
    u32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      uint32_t word = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {   // dword j of v[i]: elements 8 i + 2 j (low half) and + 1
        const uint32_t d = v[i][j];
        const uint32_t c0 = w4_code(w4_scaled(d & 0x7fffu, E, inv)) | ((d >> 12) & 8u);
        const uint32_t c1 = w4_code(w4_scaled((d >> 16) & 0x7fffu, E, inv)) | ((d >> 28) & 8u);
        word |= (c0 | (c1 << 4)) << (8 * j);
      }
      o[i] = word;
    }
    *reinterpret_cast<u32x4*>(code + n * (long)(K / 2) + 16 * b) = o;
    scale[n * nb + b] = (uint8_t)(E + 127);
  }
}

// the eight codes of one dword, scaled: element 2 i + h is nibble h of byte i
__device__ __forceinline__ bf16x8 w4_widen(uint32_t c, float s) {
  const bf16x2 p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, s, 0);
  const bf16x2 p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, s, 1);
  const bf16x2 p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, s, 2);
  const bf16x2 p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, s, 3);
  return bf16x8{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
}

__global__ void __launch_bounds__(256)
dequant_mxfp4_kernel(const uint8_t* __restrict__ code, const uint8_t* __restrict__ scale, long N, int K,
                     bf16* __restrict__ out, long ldo) {
  const int nb = K / 32;
  const long total = N * nb;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long n = e / nb;
    const int b = (int)(e % nb);
    const u32x4 c = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(code + n * (long)(K / 2) + 16 * b));
    const float s = pow2_bits(scale[n * nb + b]);
    bf16* o = out + n * ldo + 32 * b;
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<bf16x8*>(o + 8 * i) = w4_widen(c[i], s);
  }
}

// ---------------------------------------------------------------------------------------
// Native decode GEMM
// ---------------------------------------------------------------------------------------
// The MXFP4 side of gemm_wq.inc's skeleton: chunks of Q sub-chunks.
template <int Q_> struct W4Fmt {
  static constexpr int Q = Q_, kMaxRows = kW4NativeMaxRows, kLoads = Q, kSteps = 4;
  static constexpr bool kRowScale = false;   // the block scales go into the fragments
  using Scale = uint8_t;
  struct Regs {
    u32x4 c[Q];      // 32 codes of block g of each sub-chunk
    uint32_t s[Q];   // the sub-chunk's four scale bytes
  };

  struct Pitch { long Kb, Ks; };   // K / 2 code bytes and K / 32 scale bytes per row
  static __device__ __forceinline__ Pitch pitch(int K) { return {K / 2, K / 32}; }

  // kc counts chunks of Q sub-chunks
  template <int NT>
  static __device__ __forceinline__ void load(const uint8_t* __restrict__ W, const uint8_t* __restrict__ S, Pitch pitch,
                                              int n0, int kc, int lane, Regs (&a)[NT]) {
    const long Kb = pitch.Kb, Ks = pitch.Ks;
    const int g = lane >> 4, r = lane & 15;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const long row = n0 + 16 * t + r;
      const uint8_t* p = W + row * Kb + (long)kc * (64 * Q) + 16 * g;
      const uint8_t* ps = S + row * Ks + (long)kc * (4 * Q);
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        a[t].c[q] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p + 64 * q));
        a[t].s[q] = *reinterpret_cast<const uint32_t*>(ps + 4 * q);
      }
    }
  }

  static __device__ __forceinline__ int koff(int q, int s, int g) { return 128 * q + 32 * g + 8 * s; }
  static __device__ __forceinline__ float scale(const Regs& a, int q, int g) {
    return pow2_bits((a.s[q] >> (8 * g)) & 0xffu);
  }
  static __device__ __forceinline__ bf16x8 frag(const Regs& a, int q, int s, float sc) {
    return w4_widen(a.c[q][s], sc);
  }

  // gemm_w8's rule: split K while the grid has at most 320 workgroups (1.25 per CU), keeping
  // >= 8 sub-chunks (1024 k) per split: 70B QKV / O / down split 8 ways, gate/up not at all
  // (in the sweep 8 ways was fastest for QKV and down at 1 and 16 rows; O ties at 4 and 8 ways at
  // 1 row and is 7 % faster at 4 ways at 16 rows, which this rule leaves on the table).
  // A full 64-row tile writes 4 - 64 times the slab bytes of a decode batch of 1 - 16 rows, and
  // there the fastest split of the sweep (profiles/w4) was the largest one that keeps the grid
  // within one workgroup per CU (256): QKV 2, O and down 4.
  static int splitk(int mt, int ztiles, int blocks, int nsub) {
    int sk = 1;
    if (mt == 4 && ztiles == 1)
      while (blocks * sk * 2 <= 256 && nsub >= 16 * sk && sk < 16) sk *= 2;
    else
      while (blocks * sk <= 320 && nsub >= 8 * sk && sk < 16) sk *= 2;
    return sk;
  }
};

// ---------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------
// (the plan is the same for either Q)
int gemm_w4_check(int M, int N, int K, int epi) { return wq_check<W4Fmt<1>>(M, N, K, epi); }
int gemm_w4_splitk(int M, int N, int K, int epi) { return wq_splitk<W4Fmt<1>>(M, N, K, epi); }
size_t gemm_w4_workspace_bytes(int M, int N, int K) { return wq_workspace_bytes<W4Fmt<1>>(M, N, K); }

int launch_gemm_w4(const bf16* X, long ldx, const uint8_t* W, const uint8_t* scale, int M, int N, int K, int epi,
                   bf16* out, long ldo, float* ws, size_t ws_bytes, hipStream_t stream, bool any_m, int force_sk) {
  // 256-k chunks wherever K allows: 1.07-1.33x faster than 128-k ones on the 70B projections
  // (profiles/w4, measured with a switch that this file no longer has)
  return K % (2 * kWqSub) == 0
             ? wq_launch<W4Fmt<2>>(X, ldx, W, scale, M, N, K, epi, out, ldo, ws, ws_bytes, stream, any_m, force_sk)
             : wq_launch<W4Fmt<1>>(X, ldx, W, scale, M, N, K, epi, out, ldo, ws, ws_bytes, stream, any_m, force_sk);
}

void launch_quant_mxfp4(const bf16* w, long ldw, long N, int K, uint8_t* code, uint8_t* scale,
                        hipStream_t stream) {
  if (N <= 0 || K <= 0) return;
  quant_mxfp4_kernel<<<wq_grid(N * (K / 32)), 256, 0, stream>>>(w, ldw, N, K, code, scale);
}

void launch_dequant_mxfp4(const uint8_t* code, const uint8_t* scale, long N, int K, bf16* out, long ldo,
                          hipStream_t stream) {
  if (N <= 0 || K <= 0) return;
  dequant_mxfp4_kernel<<<wq_grid(N * (K / 32)), 256, 0, stream>>>(code, scale, N, K, out, ldo);
}

}  // namespace bfly
