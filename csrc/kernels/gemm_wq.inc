// The decode GEMM of the weight-only formats: one skeleton, instantiated by gemm_w8.hip (FP8
// e4m3, one f32 scale per row) and gemm_w4.hip (MXFP4) with a format struct each. Included
// inside namespace bfly, after bfly_common.h and bfly_kernels.h.
//
//  * wq_gemm_kernel (up to Fmt::kMaxRows rows, in 64-row tiles): a workgroup of 4 waves owns
//    64*NT (NT = 2) weight rows and one K range (split-K over blockIdx.y, f32 slabs +
//    gemm_wq_reduce_kernel). Each wave streams its 16*NT rows straight into VGPRs with
//    non-temporal 16-B loads, five chunks of 128 Q k ahead, and widens them in registers. The X
//    rows of a chunk are shared by the 4 waves, so they are staged once per workgroup through a
//    double-buffered padded LDS tile (X from L2 per wave would exceed the weight bytes at 64
//    rows). W is the MFMA A operand, as in gemm_skinny_kernel: a lane holds 4 consecutive n of
//    one token row.
//  * The host side: plan (shape contract, 16-row tiles, split-K factor), check, split-K and
//    workspace queries, launch.
//
// What a format struct `Fmt` supplies (g = lane >> 4, the lane group):
//   Q, kMaxRows, Scale   chunk width in units of 128 k; the native kernel's row limit; scale type
//   Regs, load<NT>(W, S, pitch, n0, kc, lane, a)   a lane's weight registers of one (chunk,
//       16-row tile), and chunk kc of rows n0 .. n0 + 16 NT - 1 -> a[NT]: 16-B loads 64 B apart
//       at byte 16 g, so that one load instruction reads 64 contiguous bytes per row.
//       pitch = pitch(K): what load needs of K, the code bytes (and scales) per weight row
//   kLoads, kSteps, koff(q, s, g), scale(regs, q, g), frag(regs, q, s, sc)   the K permutation:
//       MFMA step (q, s), s < kSteps, takes 8 weights of 16-B load q < kLoads. koff: their k
//       offset in the chunk, where the X fragment is read; frag: the 8 weights widened to bf16,
//       given sc = scale(regs, q, g), which the steps of load q share (MXFP4: 2^E)
//   kRowScale   S is one f32 scale per weight row, which multiplies the f32 sums (FP8)
//   splitk(mt, ztiles, blocks, nsub)   host: the split-K factor for `mt` 16-row tiles in each of
//       `ztiles` 64-row tiles, `blocks` workgroups unsplit, K = 128 nsub

constexpr int kWqThreads = 256;
constexpr int kWqSub = 128;          // K elements of a sub-chunk; a pipeline step covers Q of them
template <int Q> constexpr int kWqXPitch = 256 * Q + 16;   // bytes per X row in LDS (rows 4 banks apart)

// The workgroup's 256 threads copy MT x 16 rows x 128 Q k of X: 16 Q lanes per row (one 16-B
// column each), 16 / Q rows per pass. (Q = 1: thread -> row tid / 16, one 256-B row per 16 lanes.)
template <int MT, int Q>
__device__ __forceinline__ void wq_x_load(const bf16* __restrict__ X, long ldx, int m0, int M, int kc,
                                          bf16x8 (&xr)[MT * Q]) {
  const int row = threadIdx.x / (16 * Q), kb = threadIdx.x % (16 * Q);
#pragma unroll
  for (int p = 0; p < MT * Q; ++p) {
    int m = m0 + (16 / Q) * p + row;
    m = m < M ? m : M - 1;
    xr[p] = *reinterpret_cast<const bf16x8*>(X + (long)m * ldx + (long)kc * (kWqSub * Q) + 8 * kb);
  }
}

template <int MT, int Q>
__device__ __forceinline__ void wq_x_store(unsigned char* buf, const bf16x8 (&xr)[MT * Q]) {
  const int row = threadIdx.x / (16 * Q), kb = threadIdx.x % (16 * Q);
#pragma unroll
  for (int p = 0; p < MT * Q; ++p)
    *reinterpret_cast<bf16x8*>(buf + ((16 / Q) * p + row) * kWqXPitch<Q> + 16 * kb) = xr[p];
}

template <class Fmt, int MT, int NT>
__device__ __forceinline__ void wq_mma(const typename Fmt::Regs (&a)[NT], const unsigned char* buf, int lane,
                                       f32x4 (&acc)[NT][MT]) {
  const int g = lane >> 4, r = lane & 15;
#pragma unroll
  for (int q = 0; q < Fmt::kLoads; ++q) {
    float sc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) sc[t] = Fmt::scale(a[t], q, g);
#pragma unroll
    for (int s = 0; s < Fmt::kSteps; ++s) {
      bf16x8 b[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        b[mt] = *reinterpret_cast<const bf16x8*>(buf + (16 * mt + r) * kWqXPitch<Fmt::Q> + 2 * Fmt::koff(q, s, g));
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const bf16x8 wa = Fmt::frag(a[t], q, s, sc[t]);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[t][mt] = mfma16(wa, b[mt], acc[t][mt]);
      }
    }
  }
}

template <class Fmt, int MT, int NT>
__global__ void __launch_bounds__(kWqThreads)
wq_gemm_kernel(const bf16* __restrict__ X, long ldx, const uint8_t* __restrict__ W,
               const typename Fmt::Scale* __restrict__ S, int M, int N, int K, int epi,
               bf16* __restrict__ out, long ldo, float* __restrict__ part) {
  constexpr int Q = Fmt::Q, kBuf = MT * 16 * kWqXPitch<Q>;
  __shared__ __attribute__((aligned(16))) unsigned char xs[2 * kBuf];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int n0 = blockIdx.x * 64 * NT + wid * 16 * NT;
  const int m0 = blockIdx.z * 64;
  const auto pitch = Fmt::pitch(K);
  const int nchunks = K / (kWqSub * Q);
  const int SK = gridDim.y;
  const int c0 = (int)(((long)nchunks * blockIdx.y) / SK);
  const int c1 = (int)(((long)nchunks * (blockIdx.y + 1)) / SK);

  f32x4 acc[NT][MT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[t][mt] = f32x4{0.f, 0.f, 0.f, 0.f};

  // A ring of R weight register sets: chunk s is consumed while s + 1 .. s + R - 1 are in flight
  // (R - 1 chunks of 16 NT rows per wave, 128 B a row in FP8, cover the HBM latency with one
  // workgroup per CU). X goes L2 -> registers -> LDS: loaded three steps ahead, stored into the
  // other LDS buffer one step ahead. Every ring index below is a compile-time constant after
  // unrolling (runtime-indexed register arrays would go to scratch); the step count is uniform
  // over the workgroup, so every barrier is too. X loads are issued before the W loads of a
  // step: memory returns in order, and the X store of step s must not wait for the newest weights.
  constexpr int R = 6;
  typename Fmt::Regs a[R][NT];
  bf16x8 xr[2][MT * Q];
  const int n = c1 - c0;
  if (n > 0) wq_x_load<MT, Q>(X, ldx, m0, M, c0, xr[0]);
  if (n > 1) wq_x_load<MT, Q>(X, ldx, m0, M, c0 + 1, xr[1]);
#pragma unroll
  for (int j = 0; j < R - 1; ++j)
    if (j < n) Fmt::template load<NT>(W, S, pitch, n0, c0 + j, lane, a[j]);
  if (n > 0) wq_x_store<MT, Q>(xs, xr[0]);
  if (n > 2) wq_x_load<MT, Q>(X, ldx, m0, M, c0 + 2, xr[0]);
  __syncthreads();
  for (int i = 0; i < n; i += R) {
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int s = i + j;                 // R is even: s and j have the same parity
      if (s >= n) break;
      if (s + 1 < n) wq_x_store<MT, Q>(xs + ((j + 1) & 1) * kBuf, xr[(j + 1) & 1]);
      if (s + 3 < n) wq_x_load<MT, Q>(X, ldx, m0, M, c0 + s + 3, xr[(j + 1) & 1]);
      if (s + R - 1 < n) Fmt::template load<NT>(W, S, pitch, n0, c0 + s + R - 1, lane, a[(j + R - 1) % R]);
      wq_mma<Fmt, MT, NT>(a[j], xs + (j & 1) * kBuf, lane, acc);
      __syncthreads();
    }
  }

  // Epilogue: lane (g, r) holds n = n0 + 16 t + 4 g + i (i < 4) of token row m0 + 16 mt + r.
  const int g = lane >> 4, r = lane & 15;
  if constexpr (Fmt::kRowScale) {   // one scale per weight row: it multiplies the f32 sums
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const f32x4 sc = *reinterpret_cast<const f32x4*>(S + n0 + 16 * t + 4 * g);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[t][mt] *= sc;
    }
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

// ---------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------
// The grid of an elementwise kernel that strides 256-thread workgroups over `total` items.
static inline int wq_grid(long total, long cap = 16384) {
  const long grid = (total + 255) / 256;
  return (int)(grid > cap ? cap : grid);
}

struct WqPlan { int mt, sk; };   // 16-row tiles per workgroup, split-K factor; NT = 2 throughout

// Shape contract: N % 128 == 0, K % 128 == 0, epilogue none / SiLU. (`any_m`: skip the row limit.)
// 128 weight rows per workgroup; the plan does not depend on Fmt::Q.
template <class Fmt>
static bool wq_plan(int M, int N, int K, int epi, WqPlan& p, bool any_m = false) {
  if (M <= 0 || N <= 0 || K <= 0 || N % 128 != 0 || K % kWqSub != 0) return false;
  if (epi != EPI_NONE && epi != EPI_SILU) return false;
  if (!any_m && M > Fmt::kMaxRows) return false;
  p.mt = M >= 64 ? 4 : (M + 15) / 16;
  const int ztiles = (M + 63) / 64;
  p.sk = Fmt::splitk(p.mt, ztiles, N / 128 * ztiles, K / kWqSub);
  return true;
}

template <class Fmt>
static int wq_check(int M, int N, int K, int epi) {
  WqPlan p;
  return M <= 0 || wq_plan<Fmt>(M, N, K, epi, p) ? 0 : -1;
}

template <class Fmt>
static int wq_splitk(int M, int N, int K, int epi) {
  WqPlan p;
  return wq_plan<Fmt>(M, N, K, epi, p, true) ? p.sk : 0;
}

template <class Fmt>
static size_t wq_workspace_bytes(int M, int N, int K) {
  const int sk = wq_splitk<Fmt>(M, N, K, EPI_NONE);
  return sk > 1 ? (size_t)sk * M * N * sizeof(float) : 0;
}

// 0: launched (or nothing to do), -1: outside the contract, -2 / -3: a forced split with more
// splits than chunks / without the workspace for it. The heuristic's split falls back to
// sk = 1 when the workspace is missing or too small.
template <class Fmt>
static int wq_launch(const bf16* X, long ldx, const uint8_t* W, const typename Fmt::Scale* S, int M, int N, int K,
                     int epi, bf16* out, long ldo, float* ws, size_t ws_bytes, hipStream_t stream, bool any_m,
                     int force_sk) {
  if (M <= 0) return 0;
  WqPlan p;
  if (!wq_plan<Fmt>(M, N, K, epi, p, any_m)) return -1;
  if (force_sk > 0) {   // measurements (tools/w8_bench.py, tools/w4_bench.py): another split than the heuristic's
    p.sk = force_sk;
    if (p.sk > K / (kWqSub * Fmt::Q)) return -2;
    if (p.sk > 1 && (ws == nullptr || ws_bytes < (size_t)p.sk * M * N * sizeof(float))) return -3;
  }
  if (p.sk > 1 && (ws == nullptr || ws_bytes < (size_t)p.sk * M * N * sizeof(float))) p.sk = 1;
  float* part = p.sk > 1 ? ws : nullptr;
  const auto kernel = p.mt == 1 ? wq_gemm_kernel<Fmt, 1, 2> : p.mt == 2 ? wq_gemm_kernel<Fmt, 2, 2>
                    : p.mt == 3 ? wq_gemm_kernel<Fmt, 3, 2> : wq_gemm_kernel<Fmt, 4, 2>;
  kernel<<<dim3(N / 128, p.sk, (M + 63) / 64), kWqThreads, 0, stream>>>(X, ldx, W, S, M, N, K, epi, out, ldo, part);
  if (part) launch_gemm_wq_reduce(part, p.sk, M, N, epi, out, ldo, stream);
  return 0;
}
