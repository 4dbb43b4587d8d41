// Per-token log-probabilities (K18): log_softmax of the raw logits over the whole vocabulary at
// the chosen token, and the n most likely tokens of the row, over the (possibly
// vocab-parallel) bf16 logits shard. No [rows, V] f32 temporary, no sort, no host sync, fixed
// grids (graph-capturable).
//
// Stage 1 (grid rows x chunks of kLogprobsChunk logits, 256 threads): a workgroup holds its
// chunk in registers (16 logits per thread, two 16-B loads; per-element loads on the ragged
// tail) and writes the chunk max, sum(exp(x - max)), the logit of the chosen id when it lies in
// the chunk, and the chunk's n largest packed keys ordered(logit) << 32 | ~global index (the
// sampler's key: max(key) = largest logit, smallest token id on ties). The n keys come from n
// rounds of a block-wide maximum over the keys strictly below the previous round's winner;
// keys are unique, so round r yields exactly the r-th largest. Inside a chunk the rounds run on
// a 32-bit form of the key (ordered bf16 bits << 16 | 4095 - index in the chunk: the same
// order), and every wave maximum is six DPP steps (row shifts, then the gfx9 row broadcasts)
// with no LDS traffic; the rounds are the whole cost of large n.
// Stage 2 (one workgroup per row): merges the chunk statistics (M = max m_c,
// S = sum s_c exp(m_c - M)) and the chunks' candidate keys by the same selection into one f32
// record per row: (M, S, chosen logit, n x (logit, global id)); ids < 2^24 are exact in f32
// (sample_pack's convention). Missing entries are (-inf, -1).
// Stage 3 (one workgroup per row): the same merge over [tp] records (all-gathered under tensor
// parallelism; tp = 1 too): chosen_lp = chosen - (M + log S), top ids and their logprobs.
//
// A -inf logit has probability 0 and leaves the rest of the row alone (exp(-inf - m) = 0; an
// all -inf chunk contributes no mass). Rows with NaN logits are unspecified (the sampler's
// NaN guard flags them).
#include "bfly_common.h"
#include "bfly_kernels.h"

namespace bfly {
namespace {

constexpr int kLpThreads = 256;
constexpr int kLpWaves = kLpThreads / 64;
constexpr int kLpPer = kLogprobsChunk / kLpThreads;   // logits per thread
constexpr int kLpCand = kLogprobsMaxChunks * kLogprobsMaxN / kLpThreads;   // stage-2 keys per thread
static_assert(kLpPer % 8 == 0 && kLpPer * kLpThreads == kLogprobsChunk, "chunk = whole 16-B loads per thread");
static_assert(kLpCand * kLpThreads == kLogprobsMaxChunks * kLogprobsMaxN, "stage-2 candidates per thread");
static_assert(kLogprobsMaxChunks <= 64, "stage 2 merges the chunk statistics in one wave");

__device__ __forceinline__ uint32_t lp_ordered(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float lp_unordered(uint32_t o) {
  const uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
  return __uint_as_float(u);
}
__device__ __forceinline__ uint64_t lp_key(float x, uint32_t gidx) {
  return ((uint64_t)lp_ordered(x) << 32) | (uint32_t)(~gidx);
}
__device__ __forceinline__ uint64_t lp_umax(uint64_t a, uint64_t b) { return a > b ? a : b; }
// The key of a bf16 logit inside its chunk: the upper half of lp_ordered (a bf16's f32 has a zero
// lower half, so the upper half keeps the order) over 4095 - index (smallest index wins ties).
__device__ __forceinline__ uint32_t lp_key32(float x, int lidx) {
  return (lp_ordered(x) & 0xffff0000u) | (uint32_t)(kLogprobsChunk - 1 - lidx);
}
__device__ __forceinline__ float lp_key32_logit(uint32_t k) {
  const uint32_t o = k >> 16;
  return __uint_as_float(((o & 0x8000u) ? (o & 0x7fffu) : (~o & 0xffffu)) << 16);
}
__device__ __forceinline__ int lp_key32_index(uint32_t k) { return kLogprobsChunk - 1 - (int)(k & 0xffffu); }
static_assert(kLogprobsChunk <= 65536, "the index of a chunk's logit fits the key's lower half");

// One step of a DPP wave reduction: lanes the control leaves without a source read 0, the
// identity of an unsigned maximum. Every lane of the wave must be active.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t lp_dpp(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false);
}
// Wave maxima on every lane: row_shr 1, 2, 4, 8 leave each 16-lane row's maximum in its last
// lane; row_bcast15 folds rows 0 / 2 into rows 1 / 3, row_bcast31 folds lane 31 into rows 2-3;
// lane 63 then holds the wave's maximum.
__device__ __forceinline__ uint32_t lp_wave_max32(uint32_t v) {
  v = max(v, lp_dpp<0x111, 0xf>(v));
  v = max(v, lp_dpp<0x112, 0xf>(v));
  v = max(v, lp_dpp<0x114, 0xf>(v));
  v = max(v, lp_dpp<0x118, 0xf>(v));
  v = max(v, lp_dpp<0x142, 0xa>(v));
  v = max(v, lp_dpp<0x143, 0xc>(v));
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint64_t lp_dpp_max64(uint64_t v) {
  const uint32_t lo = lp_dpp<CTRL, ROW_MASK>((uint32_t)v), hi = lp_dpp<CTRL, ROW_MASK>((uint32_t)(v >> 32));
  return lp_umax(v, ((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ uint64_t lp_wave_max(uint64_t v) {
  v = lp_dpp_max64<0x111, 0xf>(v);
  v = lp_dpp_max64<0x112, 0xf>(v);
  v = lp_dpp_max64<0x114, 0xf>(v);
  v = lp_dpp_max64<0x118, 0xf>(v);
  v = lp_dpp_max64<0x142, 0xa>(v);
  v = lp_dpp_max64<0x143, 0xc>(v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 63);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 63);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ float lp_wave_fmax(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float lp_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Maximum over the workgroup, on every thread. One barrier per call: callers alternate between
// two `red` buffers, so a buffer is rewritten only after the barrier of the call in between,
// which every thread reaches after its reads of the earlier call.
__device__ __forceinline__ uint64_t lp_block_max(uint64_t v, uint64_t* red) {
  v = lp_wave_max(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  uint64_t b = red[0];
#pragma unroll
  for (int w = 1; w < kLpWaves; ++w) b = lp_umax(b, red[w]);
  return b;
}

__device__ __forceinline__ uint32_t lp_block_max32(uint32_t v, uint32_t* red) {
  v = lp_wave_max32(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t b = red[0];
#pragma unroll
  for (int w = 1; w < kLpWaves; ++w) b = max(b, red[w]);
  return b;
}

// The n largest of the keys a workgroup holds (kLpCand per thread, 0 = none), largest first:
// emit(r, key) runs on thread 0.
template <typename Emit>
__device__ __forceinline__ void lp_select(const uint64_t (&key)[kLpCand], int n, uint64_t (*red)[kLpWaves], Emit emit) {
  uint64_t prev = ~0ULL;
  for (int r = 0; r < n; ++r) {
    uint64_t b = 0;
#pragma unroll
    for (int j = 0; j < kLpCand; ++j)
      if (key[j] < prev) b = lp_umax(b, key[j]);
    b = lp_block_max(b, red[r & 1]);
    if (threadIdx.x == 0) emit(r, b);
    prev = b;     // 0 once the candidates are exhausted: no key is below it
  }
}

// scale of a partial sum taken relative to max m when the running max becomes M
__device__ __forceinline__ float lp_rescale(float s, float m, float M) {
  return m > -INFINITY ? s * __expf(m - M) : 0.f;
}

__global__ void __launch_bounds__(kLpThreads)
logprobs_partial_kernel(const bf16* __restrict__ logits, long row_stride, int V, int vstart,
                        const int* __restrict__ ids, int n, uint64_t* __restrict__ ws) {
  __shared__ uint32_t red[2][kLpWaves];
  __shared__ float fred[2][kLpWaves];
  const int row = blockIdx.x, c = blockIdx.y;
  const int begin = c * kLogprobsChunk, end = min(V, begin + kLogprobsChunk);
  const bf16* lr = logits + (long)row * row_stride;
  float x[kLpPer];
  uint32_t key[kLpPer];     // ordered bf16 << 16 | 4095 - index in the chunk; 0 = no token (beyond the shard)
#pragma unroll
  for (int k = 0; k < kLpPer / 8; ++k) {
    const int i = begin + (k * kLpThreads + (int)threadIdx.x) * 8;
    if (i + 8 <= end) {
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(lr + i);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        x[k * 8 + j] = bf2f(v[j]);
        key[k * 8 + j] = lp_key32(x[k * 8 + j], i + j - begin);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bool in = i + j < end;
        x[k * 8 + j] = in ? bf2f(lr[i + j]) : -INFINITY;
        key[k * 8 + j] = in ? lp_key32(x[k * 8 + j], i + j - begin) : 0u;
      }
    }
  }
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < kLpPer; ++k) m = fmaxf(m, x[k]);
  m = lp_wave_fmax(m);
  if ((threadIdx.x & 63) == 0) fred[0][threadIdx.x >> 6] = m;
  __syncthreads();
  m = fred[0][0];
#pragma unroll
  for (int w = 1; w < kLpWaves; ++w) m = fmaxf(m, fred[0][w]);
  float s = 0.f;
  if (m > -INFINITY) {
#pragma unroll
    for (int k = 0; k < kLpPer; ++k) s += __expf(x[k] - m);   // columns beyond the shard: exp(-inf) = 0
  }
  s = lp_wave_sum(s);
  if ((threadIdx.x & 63) == 0) fred[1][threadIdx.x >> 6] = s;
  __syncthreads();
  uint64_t* out = ws + ((long)row * gridDim.y + c) * (2 + n);
  if (threadIdx.x == 0) {
    float st = fred[1][0];
#pragma unroll
    for (int w = 1; w < kLpWaves; ++w) st += fred[1][w];
    const int lid = ids[row] - vstart;
    const float ch = (lid >= begin && lid < end) ? bf2f(lr[lid]) : -INFINITY;
    out[0] = (uint64_t)__float_as_uint(m) | ((uint64_t)__float_as_uint(st) << 32);
    out[1] = (uint64_t)__float_as_uint(ch);
  }
  uint32_t prev = ~0u;
  for (int r = 0; r < n; ++r) {
    uint32_t b = 0;
#pragma unroll
    for (int k = 0; k < kLpPer; ++k) b = max(b, key[k] < prev ? key[k] : 0u);
    b = lp_block_max32(b, red[r & 1]);
    if (threadIdx.x == 0)
      out[2 + r] = b ? lp_key(lp_key32_logit(b), (uint32_t)(vstart + begin + lp_key32_index(b))) : 0ULL;
    prev = b;     // 0 once the chunk is exhausted: no key is below it
  }
}

__global__ void __launch_bounds__(kLpThreads)
logprobs_row_kernel(const uint64_t* __restrict__ ws, int chunks, int n, float* __restrict__ record) {
  __shared__ uint64_t red[2][kLpWaves];
  const int row = blockIdx.x;
  const uint64_t* base = ws + (long)row * chunks * (2 + n);
  float* rec = record + (long)row * (3 + 2 * n);
  if (threadIdx.x < 64) {
    float m = -INFINITY, s = 0.f, ch = -INFINITY;
    if ((int)threadIdx.x < chunks) {
      const uint64_t w0 = base[(long)threadIdx.x * (2 + n)];
      m = __uint_as_float((uint32_t)w0);
      s = __uint_as_float((uint32_t)(w0 >> 32));
      ch = __uint_as_float((uint32_t)base[(long)threadIdx.x * (2 + n) + 1]);
    }
    const float M = lp_wave_fmax(m);
    const float S = lp_wave_sum(lp_rescale(s, m, M));
    ch = lp_wave_fmax(ch);
    if (threadIdx.x == 0) {
      rec[0] = M;
      rec[1] = S;
      rec[2] = ch;
    }
  }
  uint64_t key[kLpCand];
  const int cand = chunks * n;
#pragma unroll
  for (int j = 0; j < kLpCand; ++j) {
    const int idx = j * kLpThreads + (int)threadIdx.x;
    key[j] = idx < cand ? base[(long)(idx / n) * (2 + n) + 2 + idx % n] : 0ULL;
  }
  lp_select(key, n, red, [&](int r, uint64_t b) {
    rec[3 + 2 * r] = b ? lp_unordered((uint32_t)(b >> 32)) : -INFINITY;
    rec[4 + 2 * r] = b ? (float)(~(uint32_t)b) : -1.f;
  });
}

__global__ void __launch_bounds__(kLpThreads)
logprobs_merge_kernel(const float* __restrict__ recs, int tp, int rows, int n,
                      float* __restrict__ chosen_lp, int* __restrict__ top_ids,
                      float* __restrict__ top_lp) {
  __shared__ uint64_t red[2][kLpWaves];
  const int row = blockIdx.x;
  const int L = 3 + 2 * n;
  float lse = 0.f;      // on thread 0, which writes the outputs
  if (threadIdx.x < 64) {
    float m = -INFINITY, s = 0.f, ch = -INFINITY;
    for (int k = threadIdx.x; k < tp; k += 64) {
      const float* rec = recs + ((long)k * rows + row) * L;
      const float mk = rec[0], nm = fmaxf(m, mk);
      s = lp_rescale(s, m, nm) + lp_rescale(rec[1], mk, nm);
      m = nm;
      ch = fmaxf(ch, rec[2]);
    }
    const float M = lp_wave_fmax(m);
    const float S = lp_wave_sum(lp_rescale(s, m, M));
    ch = lp_wave_fmax(ch);
    lse = M + logf(S);
    if (threadIdx.x == 0) chosen_lp[row] = ch - lse;
  }
  uint64_t key[kLpCand];      // the shards' tp * n record entries (the host checks tp * n)
  const int cand = tp * n;
#pragma unroll
  for (int j = 0; j < kLpCand; ++j) {
    const int idx = j * kLpThreads + (int)threadIdx.x;
    key[j] = 0ULL;
    if (idx < cand) {
      const float* e = recs + ((long)(idx / n) * rows + row) * L + 3 + 2 * (idx % n);
      const float id = e[1];
      if (id >= 0.f) key[j] = lp_key(e[0], (uint32_t)(int)id);
    }
  }
  lp_select(key, n, red, [&](int r, uint64_t b) {
    top_ids[(long)row * n + r] = b ? (int)(~(uint32_t)b) : -1;
    top_lp[(long)row * n + r] = b ? lp_unordered((uint32_t)(b >> 32)) - lse : -INFINITY;
  });
}

}  // namespace

void launch_logprobs_partial(const bf16* logits, long row_stride, int rows, int V, int vstart,
                             const int* ids, int n, uint64_t* workspace, float* record,
                             hipStream_t stream) {
  if (rows <= 0) return;
  const int chunks = logprobs_chunks(V);
  if (chunks > 0)
    logprobs_partial_kernel<<<dim3(rows, chunks), kLpThreads, 0, stream>>>(logits, row_stride, V, vstart, ids, n,
                                                                            workspace);
  logprobs_row_kernel<<<rows, kLpThreads, 0, stream>>>(workspace, chunks, n, record);
}

void launch_logprobs_merge(const float* records, int tp, int rows, int n, float* chosen_lp,
                           int* top_ids, float* top_lp, hipStream_t stream) {
  if (rows <= 0) return;
  logprobs_merge_kernel<<<rows, kLpThreads, 0, stream>>>(records, tp, rows, n, chosen_lp, top_ids, top_lp);
}

}  // namespace bfly
