// Multi-query paged decode attention for speculative decoding ("verify" step).
//
// A verify step runs QN = 1 + k rows per sequence: row 0 is the newest token, rows 1 .. k are
// draft tokens at the following positions. rope_kv has appended every row's K/V to the paged
// cache, so row t of sequence b attends to keys [0, ctx_lens[b] + min(t, q_lens[b] - 1)):
// ctx_lens has the decode kernel's meaning (the keys row 0 sees, its own included), rows
// t >= q_lens[b] are padding and are computed with the last valid row's limit (never skipped
// divergently, never reading past that limit) and written.
//
// Structure of attn_decode_kernel (attention.hip): one workgroup per (context split, kv head,
// sequence), 4 waves walking the split's pages round-robin, S^T = K . Q^T with K pages as the A
// operand in the sigma key order, V^T pages as the A operand of O^T = V^T . P^T, both straight
// to VGPRs, two register sets for bf16 pages and three for FP8. What differs: the B operand is
// QT tiles of 16 columns, column c = t * G + g (row t, query head g of the kv head), and every
// K / V fragment a wave loads feeds all QT tiles: the pages are streamed ONCE for all draft rows,
// where QN calls of the decode kernel stream them QN times and attn_prefill_paged has no
// context split (8 workgroups at B = 1). Softmax state (m, l) is per lane per tile, the key mask
// is the column's own limit, and split range / emptiness follow the sequence's largest limit.
// Own wave merge and split combine: the partial layout carries 16 * QT columns.
#include "bfly_common.h"
#include "bfly_kernels.h"
#include "bfly_kv.h"

namespace bfly {

namespace {

constexpr int kVfThreads = 256;
constexpr float kVfNegInf = -INFINITY;

template <int D, int BS, typename CT, int QT>
__global__ void __launch_bounds__(kVfThreads)
attn_verify_kernel(const bf16* __restrict__ q, long q_stride, const CT* __restrict__ k_cache,
                   const CT* __restrict__ v_cache, const int* __restrict__ block_tables, int bt_stride,
                   const int* __restrict__ ctx_lens, const int* __restrict__ q_lens, int QN, int Hq, int Hkv,
                   float scale_log2, int part_tokens, bf16* __restrict__ out, float* __restrict__ part_o,
                   float* __restrict__ part_ml) {
  static_assert(D == 128 && BS == 32, "verify kernel is specialised for D=128, BS=32");
  static_assert(QT >= 1 && QT <= 4, "1 .. 4 column tiles");
  constexpr int NC = 16 * QT;                       // columns of the partial layout
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int s = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int nsplit = gridDim.x;
  const int G = Hq / Hkv;
  const int ncol = QN * G;                          // valid columns (<= NC)
  const int ql = min(max(q_lens[b], 1), QN);
  // largest limit of the sequence, never past what the block table addresses
  const int ctx = min(ctx_lens[b], bt_stride * BS - (ql - 1));
  const int lim_max = ctx + ql - 1;
  const int tok0 = s * part_tokens;
  const int tok1 = min(lim_max, tok0 + part_tokens);
  const long part_base = ((long)(b * Hkv + h) * nsplit + s);

  __shared__ float s_o[4][8][4][64];
  __shared__ float s_m[4][16], s_l[4][16];
  // QT = 4: the 64 VGPRs of Q^T fragments live in LDS (identical for the four waves) and are
  // re-read per page, which keeps two bf16 page sets in registers without scratch
  constexpr bool kQLds = QT == 4;
  __shared__ bf16x8 s_q[kQLds ? QT : 1][4][64];

  if (tok0 >= tok1) {  // empty split: mark it so the combine skips it
    if (nsplit > 1 && threadIdx.x < NC) {
      part_ml[(part_base * NC + threadIdx.x) * 2 + 0] = kVfNegInf;
      part_ml[(part_base * NC + threadIdx.x) * 2 + 1] = 0.f;
    }
    return;
  }

  const int g = lane >> 4, r = lane & 15;
  constexpr bool kF8 = sizeof(CT) == 1;
  auto d_off = [&](int ds) { return kF8 ? 64 * (ds >> 1) + 16 * g + 8 * (ds & 1) : 32 * ds + 8 * g; };
  // Q^T fragments (B operand): tile j, lane column r is column c = 16 j + r = t * G + head;
  // columns >= ncol are zero and see no key
  bf16x8 qf[QT][4];
  int lim[QT];
#pragma unroll
  for (int j = 0; j < QT; ++j) {
    const int c = 16 * j + r;
    const bool valid = c < ncol;
    const int t = valid ? c / G : 0, hh = valid ? c % G : 0;
    lim[j] = valid ? ctx + min(t, ql - 1) : 0;
    const bf16* qp = q + (long)(b * QN + t) * q_stride + (long)(h * G + hh) * D;
#pragma unroll
    for (int ds = 0; ds < 4; ++ds) {
      qf[j][ds] = *reinterpret_cast<const bf16x8*>(qp + d_off(ds));
      if (!valid) qf[j][ds] = bf16x8{};
      if (kQLds && wid == 0) s_q[j][ds][lane] = qf[j][ds];
    }
  }
  if constexpr (kQLds) __syncthreads();

  f32x4 o[QT][8];
  float m[QT], l[QT];
#pragma unroll
  for (int j = 0; j < QT; ++j) {
    m[j] = kVfNegInf;
    l[j] = 0.f;
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) o[j][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  const int p0 = tok0 / BS, p1 = (tok1 + BS - 1) / BS;
  const int* bt = block_tables + (long)b * bt_stride;

  typedef typename KV<CT>::raw_t raw_t;
  auto load_page = [&](int p, raw_t (&kf)[2][4], raw_t (&vf)[8]) {
    const long blk = bt[p];
    const CT* kb = k_cache + ((blk * Hkv + h) * BS) * D;
    const CT* vb = v_cache + (blk * Hkv + h) * (long)D * BS;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      const int key = 8 * (r >> 2) + 4 * kt + (r & 3);   // sigma: lane ends with 8 consecutive keys
#pragma unroll
      for (int ds = 0; ds < 4; ++ds)
        if constexpr (kF8) {
          if (ds & 1) continue;
          const u32x4 w = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(kb + key * D + d_off(ds)));
          kf[kt][ds] = raw_t{w[0], w[1]};
          kf[kt][ds + 1] = raw_t{w[2], w[3]};
        } else {
          kf[kt][ds] = KV<CT>::ld(kb + key * D + d_off(ds));
        }
    }
    // V^T rows: d = 16dt + r, keys 8g .. 8g+7
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) vf[dt] = KV<CT>::ld(vb + (16 * dt + r) * BS + 8 * g);
  };
  auto compute_page = [&](int p, const raw_t (&kf)[2][4], const raw_t (&vf)[8]) {
    bf16x8 pb[QT];
    float alpha[QT];
    // every K fragment is widened once (a no-op for bf16 pages) and feeds all QT tiles
    bf16x8 kw[2][4];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int ds = 0; ds < 4; ++ds) kw[kt][ds] = KV<CT>::widen(kf[kt][ds]);
    if constexpr (kQLds) asm volatile("" ::: "memory");   // the Q reads below stay in this page's body
#pragma unroll
    for (int j = 0; j < QT; ++j) {
      f32x4 st[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int ds = 0; ds < 4; ++ds) {
        bf16x8 qv;
        if constexpr (kQLds) qv = s_q[j][ds][lane];
        else qv = qf[j][ds];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) st[kt] = mfma16(kw[kt][ds], qv, st[kt]);
      }
      // st[kt][i] = S[key = p*BS + 8g + 4kt + i][column 16 j + r]
      float x[8];
      float tmax = kVfNegInf;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int key = p * BS + 8 * g + 4 * kt + i;
          const float v = key < lim[j] ? st[kt][i] * scale_log2 : kVfNegInf;
          x[kt * 4 + i] = v;
          tmax = fmaxf(tmax, v);
        }
      tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
      tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
      const float mn = fmaxf(m[j], tmax);
      const float mb = mn == kVfNegInf ? 0.f : mn;
      alpha[j] = exp2f(m[j] - mb);
      float ps = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float pv = exp2f(x[i] - mb);
        ps += pv;
        pb[j][i] = f2bf(pv);
      }
      l[j] = l[j] * alpha[j] + ps;
      m[j] = mn;
    }
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) {
      const bf16x8 vw = KV<CT>::widen(vf[dt]);
#pragma unroll
      for (int j = 0; j < QT; ++j) {
        o[j][dt] *= alpha[j];
        o[j][dt] = mfma16(vw, pb[j], o[j][dt]);
      }
    }
  };

  // software pipeline over this wave's pages (p0 + wid, +4, ...), as in attn_decode_kernel
  raw_t kA[2][4], vA[8], kB[2][4], vB[8];
  int p = p0 + wid;
  if (p < p1) load_page(p, kA, vA);
  if constexpr (sizeof(CT) == 2) {
    while (p < p1) {
      if (p + 4 < p1) load_page(p + 4, kB, vB);
      compute_page(p, kA, vA);
      p += 4;
      if (p >= p1) break;
      if (p + 4 < p1) load_page(p + 4, kA, vA);
      compute_page(p, kB, vB);
      p += 4;
    }
  } else {
    raw_t kC[2][4], vC[8];
    if (p + 4 < p1) load_page(p + 4, kB, vB);
    while (p < p1) {
      if (p + 8 < p1) load_page(p + 8, kC, vC);
      compute_page(p, kA, vA);
      p += 4;
      if (p >= p1) break;
      if (p + 8 < p1) load_page(p + 8, kA, vA);
      compute_page(p, kB, vB);
      p += 4;
      if (p >= p1) break;
      if (p + 8 < p1) load_page(p + 8, kB, vB);
      compute_page(p, kC, vC);
      p += 4;
    }
  }

  // Merge the 4 waves, one tile at a time through the same 32 KiB of LDS:
  // o[j][dt][i] = O[column 16 j + r][d = 16dt + 4g + i]
#pragma unroll
  for (int j = 0; j < QT; ++j) {
    float lj = l[j];
    lj += __shfl_xor(lj, 16, 64);
    lj += __shfl_xor(lj, 32, 64);
    if (j > 0) __syncthreads();   // the previous tile's readers are done
#pragma unroll
    for (int dt = 0; dt < 8; ++dt)
#pragma unroll
      for (int i = 0; i < 4; ++i) s_o[wid][dt][i][lane] = o[j][dt][i];
    if (g == 0) {
      s_m[wid][r] = m[j];
      s_l[wid][r] = lj;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 16 * D; e += kVfThreads) {
      const int cr = e / D, d = e % D;
      const int c = 16 * j + cr;
      if (c >= ncol) continue;
      float M = kVfNegInf;
#pragma unroll
      for (int w = 0; w < 4; ++w) M = fmaxf(M, s_m[w][cr]);
      const float Mb = M == kVfNegInf ? 0.f : M;
      float L = 0.f, O = 0.f;
      const int dt = d >> 4, i = d & 3, ln = cr + 16 * ((d & 15) >> 2);
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const float f = exp2f(s_m[w][cr] - Mb);
        L += f * s_l[w][cr];
        O += f * s_o[w][dt][i][ln];
      }
      if (nsplit == 1) {
        const int t = c / G, hh = c % G;
        out[((long)(b * QN + t) * Hq + h * G + hh) * D + d] = f2bf(L > 0.f ? O / L : 0.f);
      } else {
        part_o[(part_base * NC + c) * D + d] = O;
        if (d == 0) {
          part_ml[(part_base * NC + c) * 2 + 0] = M;
          part_ml[(part_base * NC + c) * 2 + 1] = L;
        }
      }
    }
  }
}

// One workgroup per (column c = t * G + g, kv head, sequence); thread = head dim element.
// NC = 16 * QT columns per (sequence, kv head, split) in the partial layout.
template <int D>
__global__ void __launch_bounds__(D)
attn_verify_combine_kernel(const float* __restrict__ part_o, const float* __restrict__ part_ml, int nsplit, int NC,
                           int QN, int Hq, int Hkv, bf16* __restrict__ out) {
  static_assert(D >= 64, "one full wave reduces the split pairs");
  __shared__ float s_m[256], s_l[256], s_w[256];
  __shared__ float s_inv;
  const int c = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int G = Hq / Hkv;
  const long base = (long)(b * Hkv + h) * nsplit;
  const int d = threadIdx.x;
  const int ns = nsplit < 256 ? nsplit : 256;
  for (int s = d; s < ns; s += D) {
    const float2 ml = *reinterpret_cast<const float2*>(part_ml + ((base + s) * NC + c) * 2);
    s_m[s] = ml.x;
    s_l[s] = ml.y;
  }
  __syncthreads();
  if (d < 64) {
    float M = kVfNegInf;
    for (int s = d; s < ns; s += 64) M = fmaxf(M, s_m[s]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) M = fmaxf(M, __shfl_xor(M, o, 64));
    const float Mb = M == kVfNegInf ? 0.f : M;
    float L = 0.f;
    for (int s = d; s < ns; s += 64) {
      const float ms = s_m[s];
      const float w = ms == kVfNegInf ? 0.f : exp2f(ms - Mb);
      s_w[s] = w;
      L += w * s_l[s];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) L += __shfl_xor(L, o, 64);
    if (d == 0) s_inv = L > 0.f ? 1.f / L : 0.f;
  }
  __syncthreads();
  const float* po = part_o + (base * NC + c) * D + d;
  const long sstride = (long)NC * D;
  float O = 0.f;
  int s = 0;
  for (; s + 4 <= ns; s += 4) {
    float x[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = po[(s + j) * sstride];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float w = s_w[s + j];
      O += w != 0.f ? w * x[j] : 0.f;   // empty splits wrote no output (it may be poison)
    }
  }
  for (; s < ns; ++s) {
    const float w = s_w[s];
    if (w != 0.f) O += w * po[s * sstride];
  }
  const int t = c / G, hh = c % G;
  out[((long)(b * QN + t) * Hq + h * G + hh) * D + d] = f2bf(O * s_inv);
}

template <typename CT, int QT>
void vf_launch(dim3 grid, hipStream_t stream, const bf16* q, long q_stride, const void* k_cache, const void* v_cache,
               const int* block_tables, int bt_stride, const int* ctx_lens, const int* q_lens, int QN, int Hq, int Hkv,
               float scale_log2, int part_tokens, bf16* out, float* part_o, float* part_ml) {
  attn_verify_kernel<128, 32, CT, QT><<<grid, kVfThreads, 0, stream>>>(
      q, q_stride, static_cast<const CT*>(k_cache), static_cast<const CT*>(v_cache), block_tables, bt_stride, ctx_lens,
      q_lens, QN, Hq, Hkv, scale_log2, part_tokens, out, part_o, part_ml);
}

}  // namespace

int attn_verify_tiles(int QN, int G) { return (QN * G + 15) / 16; }

// q rows b * QN + t (row stride q_stride), out [B, QN, Hq, D] dense. max_ctx bounds ctx_lens;
// the split geometry is the decode kernel's over max_ctx + QN - 1 keys. Partials (nsplit > 1):
// part_o [B, Hkv, nsplit, 16 QT, D], part_ml [B, Hkv, nsplit, 16 QT, 2] f32.
int launch_attn_verify(const bf16* q, long q_stride, const void* k_cache, const void* v_cache, const int* block_tables,
                       int bt_stride, const int* ctx_lens, const int* q_lens, int B, int QN, int Hq, int Hkv, int D,
                       int block_size, float scale, int max_ctx, int part_tokens, bf16* out, float* part_o,
                       float* part_ml, hipStream_t stream, int kv_fp8) {
  if (B <= 0) return 0;
  if (D != 128 || block_size != 32 || Hkv <= 0 || Hq % Hkv != 0 || QN < 1) return -1;
  const int G = Hq / Hkv;
  const int QT = attn_verify_tiles(QN, G);
  if (QT > 4) return -1;
  const int keys = max_ctx + QN - 1;
  if ((long)bt_stride * block_size < keys) return -5;
  if (part_tokens <= 0) part_tokens = attn_decode_part_tokens(B, Hkv, keys);
  if (part_tokens % block_size != 0) return -2;
  const int nsplit = attn_decode_splits(keys, part_tokens);
  if (nsplit > 256) return -4;
  if (nsplit < 1) return 0;
  if (nsplit > 1 && (part_o == nullptr || part_ml == nullptr)) return -3;
  const float scale_log2 = scale * 1.4426950408889634f;
  const dim3 grid(nsplit, Hkv, B);
#define VF_LAUNCH(CT, QT_)                                                                                         \
  vf_launch<CT, QT_>(grid, stream, q, q_stride, k_cache, v_cache, block_tables, bt_stride, ctx_lens, q_lens, QN, Hq, \
                     Hkv, scale_log2, part_tokens, out, part_o, part_ml)
#define VF_TILES(CT)                 \
  switch (QT) {                      \
    case 1: VF_LAUNCH(CT, 1); break; \
    case 2: VF_LAUNCH(CT, 2); break; \
    case 3: VF_LAUNCH(CT, 3); break; \
    default: VF_LAUNCH(CT, 4); break; \
  }
  if (kv_fp8) {
    VF_TILES(fp8_t)
  } else {
    VF_TILES(bf16)
  }
#undef VF_TILES
#undef VF_LAUNCH
  if (nsplit > 1) {
    const dim3 g2(QN * G, Hkv, B);
    attn_verify_combine_kernel<128><<<g2, 128, 0, stream>>>(part_o, part_ml, nsplit, 16 * QT, QN, Hq, Hkv, out);
  }
  return 0;
}

}  // namespace bfly
