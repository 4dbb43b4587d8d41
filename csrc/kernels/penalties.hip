// Presence / frequency / repetition penalties (K19) over the (possibly vocab-parallel) bf16
// logits shard, out of place: the raw logits stay as they are for the logprobs kernels.
//
// A row's token history lives on the device: hist[slot][0 .. len-1] int32, positions below
// prompt_len are the request's prompt, the rest its output. The newest token (position len - 1)
// is passed separately (`last`): the asynchronous engine only has it on the device, gathered from
// the previous step's ids. With c = occurrences of token t among the output positions, all in
// f32, rounded to bf16 once:
//   if t occurs anywhere in the history:  x = x > 0 ? x * inv_rep : x * rep
//   x -= freq * c;  x -= pres * (c > 0)
// inv_rep = 1 / rep comes from the host (-ffast-math: an in-kernel division is not correctly
// rounded).
//
// Grid rows x chunks of kPenaltyChunk logits, 256 threads, shaped like logprobs_partial_kernel:
// a workgroup holds its chunk in registers (16 logits per thread, two 16-B loads; per-element
// loads on the ragged tail), walks the whole history of its row with 16-B loads and counts the
// tokens that fall into its chunk with LDS atomics, one uint32 per column: output occurrences in
// the lower half, prompt occurrences in the upper half (the host keeps histories below 65536
// tokens). Tokens of other chunks or other shards, negative ids and ids beyond the shard are
// skipped. After one barrier the formula is applied to the columns with a non-zero counter; every
// other column, and every column of a row without history (slot < 0, len <= 0), is stored with
// the bits it was loaded with.
//
// Thread 0 of the row's first workgroup also stores `last` to hist[slot][len - 1] for the steps
// to come. No workgroup of the launch reads that position (the walk ends at len - 2), and the
// value stored is the one a repeated launch would store again. A slot beyond the table or a
// length beyond its width never reaches memory: the row is copied / the length is cut.
// Fixed grid, no host sync, no allocation: graph-capturable.
#include "bfly_common.h"
#include "bfly_kernels.h"

namespace bfly {
namespace {

constexpr int kPenThreads = 256;
constexpr int kPenPer = kPenaltyChunk / kPenThreads;   // logits per thread
constexpr int kPenVecs = kPenPer / 8;                  // 16-B loads per thread
static_assert(kPenPer % 8 == 0 && kPenPer * kPenThreads == kPenaltyChunk, "chunk = whole 16-B loads per thread");
static_assert(kPenaltyChunk % (4 * kPenThreads) == 0, "the counters are cleared with 16-B stores");

constexpr uint32_t kPenPrompt = 1u << 16;              // one prompt occurrence in a counter

// The formula with every product and difference rounded to f32 on its own, as the reference
// does: fused into x - freq * c the unrounded product changes the result, and where the terms
// cancel (3.25 / 1.3 = 0.7 * 3 + 0.4) that is the whole of it, far more than a bf16 ulp.
__device__ __forceinline__ float pen_apply(float x, float rep, float inv_rep, float freq, float pres, uint32_t oc) {
#pragma clang fp contract(off) reassociate(off)
  x = x > 0.f ? x * inv_rep : x * rep;
  const float f = freq * (float)oc;
  x = x - f;
  const float p = oc ? pres : 0.f;
  return x - p;
}

__global__ void __launch_bounds__(kPenThreads)
apply_penalties_kernel(const bf16* __restrict__ logits, long row_stride, int V, int vstart,
                       int* __restrict__ hist, long hist_stride, int hist_rows,
                       const int* __restrict__ slots, const int* __restrict__ lens,
                       const int* __restrict__ prompt_lens, const int* __restrict__ last,
                       const float* __restrict__ params, bf16* __restrict__ out, long out_stride) {
  __shared__ __attribute__((aligned(16))) uint32_t cnt[kPenaltyChunk];
  const int row = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
  const int begin = c * kPenaltyChunk, end = min(V, begin + kPenaltyChunk);
  const bf16* lr = logits + (long)row * row_stride;
  bf16* orow = out + (long)row * out_stride;
  const int slot = slots[row];
  const int len = min(lens[row], (int)hist_stride);
  const bool on = slot >= 0 && slot < hist_rows && len > 0;   // the same for the whole workgroup

  bf16x8 v[kPenVecs];
#pragma unroll
  for (int k = 0; k < kPenVecs; ++k) {
    const int i = begin + (k * kPenThreads + tid) * 8;
    if (i + 8 <= end) {
      v[k] = *reinterpret_cast<const bf16x8*>(lr + i);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[k][j] = i + j < end ? lr[i + j] : (bf16)0.f;
    }
  }

  if (on) {
#pragma unroll
    for (int k = 0; k < kPenaltyChunk / (4 * kPenThreads); ++k)
      reinterpret_cast<u32x4*>(cnt)[k * kPenThreads + tid] = u32x4{0u, 0u, 0u, 0u};
    __syncthreads();
    int* h = hist + (long)slot * hist_stride;
    const int plen = prompt_lens[row];
    const uint32_t lo = (uint32_t)(vstart + begin), span = (uint32_t)(end - begin);
    // a token at position p of the history: ids outside [lo, lo + span) wrap to >= span
    auto count = [&](int t, int p) {
      const uint32_t d = (uint32_t)t - lo;
      if (d < span) atomicAdd(&cnt[d], p < plen ? kPenPrompt : 1u);
    };
    const int n = len - 1;          // positions 0 .. n-1 come from hist, position n is `last`
    for (int p = tid * 4; p < n; p += kPenThreads * 4) {
      if (p + 4 <= n) {
        const int4 t = *reinterpret_cast<const int4*>(h + p);
        count(t.x, p);
        count(t.y, p + 1);
        count(t.z, p + 2);
        count(t.w, p + 3);
      } else {
        for (int j = 0; p + j < n; ++j) count(h[p + j], p + j);
      }
    }
    if (tid == 0) {
      const int t = last[row];
      count(t, n);
      if (c == 0) h[n] = t;
    }
    __syncthreads();
    const f32x4 pr = *reinterpret_cast<const f32x4*>(params + (long)row * 4);
    const float rep = pr[0], inv_rep = pr[1], freq = pr[2], pres = pr[3];
#pragma unroll
    for (int k = 0; k < kPenVecs; ++k) {
      const int l = (k * kPenThreads + tid) * 8;
      const u32x4 w0 = *reinterpret_cast<const u32x4*>(cnt + l);
      const u32x4 w1 = *reinterpret_cast<const u32x4*>(cnt + l + 4);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const uint32_t w = j < 4 ? w0[j] : w1[j - 4];
        if (w) {
          v[k][j] = f2bf(pen_apply(bf2f(v[k][j]), rep, inv_rep, freq, pres, w & (kPenPrompt - 1)));
        }
      }
    }
  }

#pragma unroll
  for (int k = 0; k < kPenVecs; ++k) {
    const int i = begin + (k * kPenThreads + tid) * 8;
    if (i + 8 <= end) {
      *reinterpret_cast<bf16x8*>(orow + i) = v[k];
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (i + j < end) orow[i + j] = v[k][j];
    }
  }
}

}  // namespace

void launch_apply_penalties(const bf16* logits, long row_stride, int rows, int V, int vstart,
                            int* hist, long hist_stride, int hist_rows, const int* slots,
                            const int* lens, const int* prompt_lens, const int* last,
                            const float* params, bf16* out, long out_stride, hipStream_t stream) {
  if (rows <= 0 || V <= 0) return;
  apply_penalties_kernel<<<dim3(rows, penalty_chunks(V)), kPenThreads, 0, stream>>>(
      logits, row_stride, V, vstart, hist, hist_stride, hist_rows, slots, lens, prompt_lens, last, params, out,
      out_stride);
}

}  // namespace bfly
