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
//  * gemm_w4_kernel (up to kW4NativeMaxRows rows, in 64-row tiles): gemm_w8_kernel's skeleton.
//    A workgroup of 4 waves owns 64*NT (NT = 2) weight rows and one K range (split-K over
//    blockIdx.y, f32 slabs + the shared slab reduce of gemm_w8.hip). Each wave streams its 16*NT
//    rows into VGPRs with non-temporal 16-B loads (32 codes = one scale block), five K chunks
//    ahead, and converts them in registers with v_cvt_scalef32_pk_bf16_fp4 (two codes and their
//    scale -> two bf16 per instruction). The X rows of a chunk are staged once per workgroup
//    through a double-buffered padded LDS tile. W is the MFMA A operand.
//    A chunk is Q sub-chunks of 128 k (Q = 2 when K % 256 == 0, else 1): per row, Q loads 64 B
//    apart, so a load instruction reads 64 contiguous bytes per row and a chunk 64 Q.
//    K permutation: lane group g = lane >> 4 loads block g of sub-chunk q, k = 128 q + 32 g + j
//    (j < 32); MFMA step (q, s), s < 4, takes the lane's codes j = 8 s .. 8 s + 7 (dword s) and
//    reads the X fragment at the same k. The four scale bytes of a (row, sub-chunk) are one
//    aligned dword: loaded once per lane, byte g extracted, 2^E formed as byte << 23.
#include "bfly_common.h"

#include "bfly_kernels.h"

namespace bfly {

constexpr int kW4Threads = 256;
constexpr int kW4Sub = 128;          // K elements of a sub-chunk: 4 scale blocks, 64 code bytes
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
template <int Q> struct W4Regs {
  u32x4 c[Q];      // 32 codes of block g of each sub-chunk
  uint32_t s[Q];   // the sub-chunk's four scale bytes
};

// kc counts chunks of Q sub-chunks; `Kb` = K / 2 code bytes and `Ks` = K / 32 scale bytes per row
template <int NT, int Q>
__device__ __forceinline__ void w4_load(const uint8_t* __restrict__ W, const uint8_t* __restrict__ S, long Kb,
                                        long Ks, int n0, int kc, int lane, W4Regs<Q> (&a)[NT]) {
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

// The workgroup's 256 threads copy MT x 16 rows x 128 Q k of X: 16 Q lanes per row (one 16-B
// column each), 16 / Q rows per pass.
template <int MT, int Q>
__device__ __forceinline__ void w4_x_load(const bf16* __restrict__ X, long ldx, int m0, int M, int kc,
                                          bf16x8 (&xr)[MT * Q]) {
  const int row = threadIdx.x / (16 * Q), kb = threadIdx.x % (16 * Q);
#pragma unroll
  for (int p = 0; p < MT * Q; ++p) {
    int m = m0 + (16 / Q) * p + row;
    m = m < M ? m : M - 1;
    xr[p] = *reinterpret_cast<const bf16x8*>(X + (long)m * ldx + (long)kc * (kW4Sub * Q) + 8 * kb);
  }
}

template <int MT, int Q>
__device__ __forceinline__ void w4_x_store(unsigned char* buf, const bf16x8 (&xr)[MT * Q]) {
  constexpr int kPitch = 256 * Q + 16;   // bytes per X row in LDS (rows 4 banks apart)
  const int row = threadIdx.x / (16 * Q), kb = threadIdx.x % (16 * Q);
#pragma unroll
  for (int p = 0; p < MT * Q; ++p)
    *reinterpret_cast<bf16x8*>(buf + ((16 / Q) * p + row) * kPitch + 16 * kb) = xr[p];
}

template <int MT, int NT, int Q>
__device__ __forceinline__ void w4_mma(const W4Regs<Q> (&a)[NT], const unsigned char* buf, int lane,
                                       f32x4 (&acc)[NT][MT]) {
  constexpr int kPitch = 256 * Q + 16;
  const int g = lane >> 4, r = lane & 15;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    float sc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) sc[t] = pow2_bits((a[t].s[q] >> (8 * g)) & 0xffu);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      bf16x8 b[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        b[mt] = *reinterpret_cast<const bf16x8*>(buf + (16 * mt + r) * kPitch + 2 * (128 * q + 32 * g + 8 * s));
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const bf16x8 wa = w4_widen(a[t].c[q][s], sc[t]);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[t][mt] = mfma16(wa, b[mt], acc[t][mt]);
      }
    }
  }
}

template <int MT, int NT, int Q>
__global__ void __launch_bounds__(kW4Threads)
gemm_w4_kernel(const bf16* __restrict__ X, long ldx, const uint8_t* __restrict__ W,
               const uint8_t* __restrict__ S, int M, int N, int K, int epi, bf16* __restrict__ out, long ldo,
               float* __restrict__ part) {
  constexpr int kBuf = MT * 16 * (256 * Q + 16);
  __shared__ __attribute__((aligned(16))) unsigned char xs[2 * kBuf];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int n0 = blockIdx.x * 64 * NT + wid * 16 * NT;
  const int m0 = blockIdx.z * 64;
  const long Kb = K / 2, Ks = K / 32;
  const int nchunks = K / (kW4Sub * Q);
  const int SK = gridDim.y;
  const int c0 = (int)(((long)nchunks * blockIdx.y) / SK);
  const int c1 = (int)(((long)nchunks * (blockIdx.y + 1)) / SK);

  f32x4 acc[NT][MT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[t][mt] = f32x4{0.f, 0.f, 0.f, 0.f};

  // gemm_w8_kernel's pipeline: a ring of R weight register sets (chunk s consumed while
  // s + 1 .. s + R - 1 are in flight), X loaded three steps ahead and stored into the other LDS
  // buffer one step ahead. Every ring index is a compile-time constant after unrolling; the
  // step count is uniform over the workgroup, so every barrier is too.
  constexpr int R = 6;
  W4Regs<Q> a[R][NT];
  bf16x8 xr[2][MT * Q];
  const int n = c1 - c0;
  if (n > 0) w4_x_load<MT, Q>(X, ldx, m0, M, c0, xr[0]);
  if (n > 1) w4_x_load<MT, Q>(X, ldx, m0, M, c0 + 1, xr[1]);
#pragma unroll
  for (int j = 0; j < R - 1; ++j)
    if (j < n) w4_load<NT, Q>(W, S, Kb, Ks, n0, c0 + j, lane, a[j]);
  if (n > 0) w4_x_store<MT, Q>(xs, xr[0]);
  if (n > 2) w4_x_load<MT, Q>(X, ldx, m0, M, c0 + 2, xr[0]);
  __syncthreads();
  for (int i = 0; i < n; i += R) {
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int s = i + j;                 // R is even: s and j have the same parity
      if (s >= n) break;
      if (s + 1 < n) w4_x_store<MT, Q>(xs + ((j + 1) & 1) * kBuf, xr[(j + 1) & 1]);
      if (s + 3 < n) w4_x_load<MT, Q>(X, ldx, m0, M, c0 + s + 3, xr[(j + 1) & 1]);
      if (s + R - 1 < n) w4_load<NT, Q>(W, S, Kb, Ks, n0, c0 + s + R - 1, lane, a[(j + R - 1) % R]);
      w4_mma<MT, NT, Q>(a[j], xs + (j & 1) * kBuf, lane, acc);
      __syncthreads();
    }
  }

  // Epilogue: lane (g, r) holds n = n0 + 16 t + 4 g + i (i < 4) of token row m0 + 16 mt + r.
  const int g = lane >> 4, r = lane & 15;
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

// ---------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------
struct W4Plan { int mt, nt, q, sk; };

// Shape contract: N % 128 == 0, K % 128 == 0, epilogue none / SiLU. (`any_m`: skip the row limit.)
static bool w4_plan(int M, int N, int K, int epi, W4Plan& p, bool any_m = false) {
  if (M <= 0 || N <= 0 || K <= 0 || N % 128 != 0 || K % kW4Sub != 0) return false;
  if (epi != EPI_NONE && epi != EPI_SILU) return false;
  if (!any_m && M > kW4NativeMaxRows) return false;
  p.mt = M >= 64 ? 4 : (M + 15) / 16;
  p.nt = 2;
  // 256-k chunks wherever K allows: 1.07-1.33x faster than 128-k ones on the 70B projections
  // (profiles/w4, measured with a switch that this file no longer has)
  p.q = K % (2 * kW4Sub) == 0 ? 2 : 1;
  const int ztiles = (M + 63) / 64;
  const int nsub = K / kW4Sub;
  // gemm_w8's rule: split K while the grid has at most 320 workgroups (1.25 per CU), keeping
  // >= 8 sub-chunks (1024 k) per split: 70B QKV / O / down split 8 ways, gate/up not at all
  // (in the sweep 8 ways was fastest for QKV and down at 1 and 16 rows; O ties at 4 and 8 ways at
  // 1 row and is 7 % faster at 4 ways at 16 rows, which this rule leaves on the table).
  // A full 64-row tile writes 4 - 64 times the slab bytes of a decode batch of 1 - 16 rows, and
  // there the fastest split of the sweep (profiles/w4) was the largest one that keeps the grid
  // within one workgroup per CU (256): QKV 2, O and down 4.
  const int blocks = N / (64 * p.nt) * ztiles;
  int sk = 1;
  if (p.mt == 4 && ztiles == 1)
    while (blocks * sk * 2 <= 256 && nsub >= 16 * sk && sk < 16) sk *= 2;
  else
    while (blocks * sk <= 320 && nsub >= 8 * sk && sk < 16) sk *= 2;
  p.sk = sk;
  return true;
}

int gemm_w4_check(int M, int N, int K, int epi) {
  if (M <= 0) return 0;
  W4Plan p;
  return w4_plan(M, N, K, epi, p) ? 0 : -1;
}

int gemm_w4_splitk(int M, int N, int K, int epi) {
  W4Plan p;
  return w4_plan(M, N, K, epi, p, true) ? p.sk : 0;
}

size_t gemm_w4_workspace_bytes(int M, int N, int K) {
  W4Plan p;
  if (!w4_plan(M, N, K, EPI_NONE, p, true) || p.sk <= 1) return 0;
  return (size_t)p.sk * M * N * sizeof(float);
}

template <int MT, int NT, int Q>
static void run_w4(const bf16* X, long ldx, const uint8_t* W, const uint8_t* S, int M, int N, int K, int epi,
                   bf16* out, long ldo, float* part, int sk, hipStream_t stream) {
  dim3 grid(N / (64 * NT), sk, (M + 63) / 64);
  gemm_w4_kernel<MT, NT, Q><<<grid, kW4Threads, 0, stream>>>(X, ldx, W, S, M, N, K, epi, out, ldo, part);
}

int launch_gemm_w4(const bf16* X, long ldx, const uint8_t* W, const uint8_t* scale, int M, int N, int K, int epi,
                   bf16* out, long ldo, float* ws, size_t ws_bytes, hipStream_t stream, bool any_m, int force_sk) {
  if (M <= 0) return 0;
  W4Plan p;
  if (!w4_plan(M, N, K, epi, p, any_m)) return -1;
  if (force_sk > 0) {   // measurements (tools/w4_bench.py): another split than the heuristic's
    p.sk = force_sk;
    if (p.sk > K / (kW4Sub * p.q)) return -2;
    if (p.sk > 1 && (ws == nullptr || ws_bytes < (size_t)p.sk * M * N * sizeof(float))) return -3;
  }
  if (p.sk > 1 && (ws == nullptr || ws_bytes < (size_t)p.sk * M * N * sizeof(float))) p.sk = 1;
  float* part = p.sk > 1 ? ws : nullptr;
#define W4_CASE(MT_, Q_)                                                                          \
  if (p.mt == MT_ && p.q == Q_)                                                                   \
    run_w4<MT_, 2, Q_>(X, ldx, W, scale, M, N, K, epi, out, ldo, part, p.sk, stream);
  W4_CASE(1, 1) W4_CASE(2, 1) W4_CASE(3, 1) W4_CASE(4, 1)
  W4_CASE(1, 2) W4_CASE(2, 2) W4_CASE(3, 2) W4_CASE(4, 2)
#undef W4_CASE
  if (part) launch_gemm_w8_reduce(part, p.sk, M, N, epi, out, ldo, stream);
  return 0;
}

static int w4_grid(long total) {
  long grid = (total + 255) / 256;
  return (int)(grid > 16384 ? 16384 : grid);
}

void launch_quant_mxfp4(const bf16* w, long ldw, long N, int K, uint8_t* code, uint8_t* scale,
                        hipStream_t stream) {
  if (N <= 0 || K <= 0) return;
  quant_mxfp4_kernel<<<w4_grid(N * (K / 32)), 256, 0, stream>>>(w, ldw, N, K, code, scale);
}

void launch_dequant_mxfp4(const uint8_t* code, const uint8_t* scale, long N, int K, bf16* out, long ldo,
                          hipStream_t stream) {
  if (N <= 0 || K <= 0) return;
  dequant_mxfp4_kernel<<<w4_grid(N * (K / 32)), 256, 0, stream>>>(code, scale, N, K, out, ldo);
}

}  // namespace bfly
