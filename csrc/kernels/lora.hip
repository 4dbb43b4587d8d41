// Multi-LoRA delta of a dense projection (K20): every row m of a batch picks its own adapter
// idx[m] out of S stacked slots, or none, and the projection's bf16 output y gets
//   y[m, n] += scale[s] * sum_r  t[m, seg(n) * R + r] * b[s, n, r],   t[m, j] = sum_k x[m, k] * a[s, j, k]
// with s = idx[m]. a [S][J][K] and b [S][N][R] bf16, J = nseg * R: the weight fuses nseg logical
// projections (q | k | v, gate | up) that share x but have their own rank-R slice of t; seg [N]
// uint8 names the slice of output row n and is read once per aligned group of 16 rows. Semantics:
// ops/reference.py lora_shrink / lora_expand_.
//
// An index outside [0, S) means "no adapter", here too (the host cannot see device values). Both
// kernels sanitise idx into a slot number or -1 before anything is addressed with it; rows
// without an adapter are never written, and a 16-row tile without any returns after reading idx.
//
// Both grids have a third dimension Z (4 up to 256 rows, else 1): the distinct valid adapters of
// a tile, in order of their first row, are dealt over its Z workgroups, so a decode tile of 16
// adapters waits for 4 dependent adapter passes, not 16. Every row belongs to one adapter, hence
// to one workgroup; a workgroup that draws no adapter returns after reading idx.
//
// lora_shrink_kernel   grid (16-row tiles, K splits, Z), 4 waves. A workgroup loops over its DISTINCT
//   valid adapters; for each one the x tile (MFMA A operand) meets 16 rows of a[s]
//   (B operand) in mfma_f32_16x16x32_bf16, both loaded straight from global memory in fragment
//   shape (lane l: 16 B at [row l & 15][k + 8 (l >> 4)]), two k-steps per iteration so a row reads
//   128 contiguous bytes. Of the product only the rows with idx == s are kept. A tile whose rows
//   share one adapter (every prefill tile) reads `a` once per 16 rows; a decode tile of 16
//   adapters reads the 16 it needs. The K range is dealt in 64-element chunks over
//   (K split, wave); the waves' partial sums meet in LDS in wave order and the K-split partials
//   go to part [KS][T][J] f32, summed by the expand kernel in split order: no atomics, the same
//   bits every launch. Only rows with an adapter are stored.
// lora_expand_kernel   grid (16-row tiles, groups of 16-column chunks, Z), 4 waves, one chunk of 16
//   output columns per wave and step. The exact-f32 mfma_f32_16x16x4 forms D[n][m] with b[s] as
//   the A operand and the summed partials of t as the B operand (element r of the rank at lane
//   quarter r / (R/4): both operands read contiguous runs), so a lane ends with 4 adjacent
//   columns of one row of y: one 8-B read-modify-write, one rounding.
//
// Fixed grids from (T, N, K) only, no host sync, no allocation: graph-capturable.
#include "bfly_common.h"
#include "bfly_kernels.h"

namespace bfly {
namespace {

constexpr int kLoraThreads = 256;
constexpr int kLoraJB = 4;        // 16-row chunks of a[s] per pass over K (shrink)

// idx[row] as a slot number, or -1: no adapter (row beyond T, negative, >= S)
__device__ __forceinline__ int lora_slot(const int* __restrict__ idx, int row, int T, int S) {
  if (row >= T) return -1;
  const int v = idx[row];
  return (unsigned)v < (unsigned)S ? v : -1;
}

// lanes 0..15 hold the tile's rows (the other lane quarters repeat them)
__device__ __forceinline__ uint32_t lora_rows_where(bool p) { return (uint32_t)(__ballot(p) & 0xFFFFull); }

// Rows (bit r: row r of the tile) whose adapter this workgroup computes: the tile's distinct
// adapters, ordered by first row, go round robin over the Z workgroups. `todo`: rows with an adapter.
__device__ __forceinline__ uint32_t lora_my_rows(int my, uint32_t todo, int z, int Z) {
  uint32_t mine = 0;
  for (int ord = 0; todo; ++ord) {
    const int s = __builtin_amdgcn_readfirstlane(__shfl(my, __builtin_ctz(todo), 64));
    const uint32_t same = lora_rows_where(my == s);
    todo &= ~same;
    if (ord % Z == z) mine |= same;
  }
  return mine;
}

__global__ void __launch_bounds__(kLoraThreads)
lora_shrink_kernel(const bf16* __restrict__ x, long ldx, const bf16* __restrict__ a,
                   const int* __restrict__ idx, float* __restrict__ part, int T, int K, int J, int S) {
  __shared__ float red[4][kLoraJB][4][kWave];   // [wave][chunk][register][lane]
  const int tile = blockIdx.x, ks = blockIdx.y, KS = gridDim.y;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r16 = lane & 15, kq = lane >> 4;
  const int my = lora_slot(idx, tile * 16 + r16, T, S);
  const uint32_t todo = lora_my_rows(my, lora_rows_where(my >= 0), blockIdx.z, gridDim.z);
  if (!todo) return;                       // the same in every wave of the workgroup
  int rowidx[4];                           // adapters of the accumulator's rows 4 kq + r
#pragma unroll
  for (int r = 0; r < 4; ++r) rowidx[r] = __shfl(my, 4 * kq + r, 64);

  const int n32 = K / 32, nc = (n32 + 1) / 2;      // 64-element chunks, the last one may be half
  const int G = KS * 4, g = ks * 4 + w;
  const bf16* xp = x + (long)min(tile * 16 + r16, T - 1) * ldx + kq * 8;   // rows beyond T: never kept
  const int nj = (J + 15) / 16;

  for (int jg = 0; jg < nj; jg += kLoraJB) {
    f32x4 out[kLoraJB];
#pragma unroll
    for (int jt = 0; jt < kLoraJB; ++jt) out[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
    uint32_t td = todo;
    while (td) {
      const int s = __builtin_amdgcn_readfirstlane(__shfl(my, __builtin_ctz(td), 64));
      td &= ~lora_rows_where(my == s);
      f32x4 acc[kLoraJB];
      const bf16* ap[kLoraJB];
#pragma unroll
      for (int jt = 0; jt < kLoraJB; ++jt) {
        acc[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
        // rows beyond J (a last chunk of 8): clamped, their columns are not stored
        ap[jt] = a + ((long)s * J + min((jg + jt) * 16 + r16, J - 1)) * K + kq * 8;
      }
#pragma unroll 2
      for (int c = g; c < nc; c += G) {
        const int k0 = c * 64;
        const bool two = 2 * c + 1 < n32;
        const int k1 = two ? k0 + 32 : k0;          // a half chunk re-reads k0 against zeros
        const bf16x8 x0 = *reinterpret_cast<const bf16x8*>(xp + k0);
        bf16x8 x1 = *reinterpret_cast<const bf16x8*>(xp + k1);
        if (!two) x1 = bf16x8{};
#pragma unroll
        for (int jt = 0; jt < kLoraJB; ++jt) {
          if (jg + jt < nj) {
            const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(ap[jt] + k0);
            const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(ap[jt] + k1);
            acc[jt] = mfma16(x0, a0, acc[jt]);
            acc[jt] = mfma16(x1, a1, acc[jt]);
          }
        }
      }
#pragma unroll
      for (int jt = 0; jt < kLoraJB; ++jt) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (rowidx[r] == s) out[jt][r] = acc[jt][r];
      }
    }
    // the four waves' K slices, summed in wave order
#pragma unroll
    for (int jt = 0; jt < kLoraJB; ++jt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) red[w][jt][r][lane] = out[jt][r];
    }
    __syncthreads();
#pragma unroll
    for (int jt = 0; jt < kLoraJB; ++jt) {
      // thread (w, lane) stores accumulator register w of lane `lane`: row 4 (lane >> 4) + w
      const float v = ((red[0][jt][w][lane] + red[1][jt][w][lane]) + red[2][jt][w][lane]) + red[3][jt][w][lane];
      const int row = tile * 16 + 4 * kq + w, j = (jg + jt) * 16 + r16;
      if (((todo >> (4 * kq + w)) & 1) && j < J) part[((long)ks * T + row) * J + j] = v;
    }
    __syncthreads();
  }
}

template <int RQ> struct LoraVec;
template <> struct LoraVec<2> { typedef float f __attribute__((ext_vector_type(2))); typedef bf16x2 h; };
template <> struct LoraVec<4> { typedef f32x4 f; typedef bf16x4 h; };
template <> struct LoraVec<8> { typedef float f __attribute__((ext_vector_type(8))); typedef bf16x8 h; };
template <> struct LoraVec<16> {
  typedef float f __attribute__((ext_vector_type(16)));
  typedef __bf16 h __attribute__((ext_vector_type(16)));
};

template <int R>
__global__ void __launch_bounds__(kLoraThreads)
lora_expand_kernel(bf16* __restrict__ y, long ldy, const float* __restrict__ part, int KS, int T, int J,
                   const bf16* __restrict__ b, int N, const uint8_t* __restrict__ seg,
                   const float* __restrict__ scale, const int* __restrict__ idx, int S, int per_wave) {
  constexpr int RQ = R / 4;                 // rank elements per lane quarter: r = kq * RQ + i
  typedef typename LoraVec<RQ>::f fvec;
  typedef typename LoraVec<RQ>::h hvec;
  const int tile = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r16 = lane & 15, kq = lane >> 4;
  const int m = tile * 16 + r16;
  const int my = lora_slot(idx, m, T, S);
  const uint32_t todo = lora_my_rows(my, lora_rows_where(my >= 0), blockIdx.z, gridDim.z);
  if (!todo) return;
  const bool mine = (todo >> r16) & 1;     // this lane's row is one of the workgroup's
  const int nseg = J / R, groups = N / 16;
  const int g0 = (blockIdx.y * 4 + w) * per_wave, g1 = min(g0 + per_wave, groups);
  for (int g = g0; g < g1; ++g) {
    const int n0 = g * 16;
    const int sg = min((int)seg[n0], nseg - 1);
    // B operand: this row's slice of t, the K-split partials summed in split order
    fvec tv = {};
    if (mine) {
      const float* tp = part + (long)m * J + sg * R + kq * RQ;
      for (int ks = 0; ks < KS; ++ks) tv += *reinterpret_cast<const fvec*>(tp + (long)ks * T * J);
    }
    f32x4 out = {0.f, 0.f, 0.f, 0.f};
    uint32_t td = todo;
    while (td) {
      const int s = __builtin_amdgcn_readfirstlane(__shfl(my, __builtin_ctz(td), 64));
      td &= ~lora_rows_where(my == s);
      // A operand: output rows n0 .. n0 + 15 of b[s]
      const hvec bv = *reinterpret_cast<const hvec*>(b + ((long)s * N + n0 + r16) * R + kq * RQ);
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < RQ; ++i) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(bf2f(bv[i]), tv[i], acc, 0, 0, 0);
      if (my == s) out = acc * scale[s];
    }
    if (mine) {                             // y[m][n0 + 4 kq .. + 4)
      bf16x4* yp = reinterpret_cast<bf16x4*>(y + (long)m * ldy + n0 + 4 * kq);
      bf16x4 v = *yp;
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = f2bf(bf2f(v[r]) + out[r]);
      *yp = v;
    }
  }
}

}  // namespace

int lora_splitk(int T, int K) {
  const int tiles = (T + 15) / 16, nc = (K / 32 + 1) / 2;
  return max(1, min(min(kLoraMaxSplitK, nc / 2), 512 / max(tiles, 1)));
}

// workgroups sharing the distinct adapters of a tile: decode batches only
static int lora_adapter_split(int T) { return T <= 256 ? 4 : 1; }

int lora_check(int K, int J, int N, int R) {
  if (K <= 0 || K % 32 != 0) return -1;
  if (N <= 0 || N % 16 != 0) return -2;
  if (R != 8 && R != 16 && R != 32 && R != 64) return -3;
  if (J <= 0 || J % R != 0 || J / R > 3) return -4;
  return 0;
}

void launch_lora_shrink(const bf16* x, long ldx, const bf16* a, const int* idx, float* part, int KS, int T,
                        int K, int J, int S, hipStream_t stream) {
  if (T <= 0 || S <= 0) return;
  lora_shrink_kernel<<<dim3((T + 15) / 16, KS, lora_adapter_split(T)), kLoraThreads, 0, stream>>>(x, ldx, a, idx, part, T, K, J, S);
}

void launch_lora_expand(bf16* y, long ldy, const float* part, int KS, int T, int J, const bf16* b, int N, int R,
                        const uint8_t* seg, const float* scale, const int* idx, int S, hipStream_t stream) {
  if (T <= 0 || S <= 0) return;
  const int tiles = (T + 15) / 16, groups = N / 16;
  const int per_wave = tiles >= 16 ? 4 : 1;       // larger batches: fewer, longer workgroups
  const dim3 grid(tiles, (groups + 4 * per_wave - 1) / (4 * per_wave), lora_adapter_split(T));
#define BFLY_LORA_EXPAND(RR)                                                                            \
  lora_expand_kernel<RR><<<grid, kLoraThreads, 0, stream>>>(y, ldy, part, KS, T, J, b, N, seg, scale, idx, S, \
                                                            per_wave)
  switch (R) {
    case 8: BFLY_LORA_EXPAND(8); break;
    case 16: BFLY_LORA_EXPAND(16); break;
    case 32: BFLY_LORA_EXPAND(32); break;
    default: BFLY_LORA_EXPAND(64); break;
  }
#undef BFLY_LORA_EXPAND
}

}  // namespace bfly
