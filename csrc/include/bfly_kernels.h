// Host-side launch API of the butterfly_amd HIP kernels. Every launcher is stream-ordered,
// allocation-free and synchronisation-free, so it can be captured into a hipGraph.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace bfly {

typedef __bf16 bf16;

// EPI_SILU_GATE: the SwiGLU epilogue followed by the MoE dense decode path's routing weight
// (what moe_gate_scale did as a separate pass): see RowScale::gate.
enum GemmEpilogue { EPI_NONE = 0, EPI_BIAS = 1, EPI_SILU = 2, EPI_SILU_GATE = 3 };

// Per-row output scales of the tile / decode-ring / mid-M epilogues.
// RMSNorm: the X rows are un-normalised RMSNorm inputs (x * g); row m is multiplied by
// rsqrt(sum_c ss[m * chunks + c] * inv_dim + eps) before the epilogue.
// MoE gate (EPI_SILU_GATE, tile kernel only): SwiGLU output column f of row m is rounded to
// bf16, multiplied by gate[m * gld + ge0 + f / gF] and rounded again, bit-identical to the
// SiLU epilogue followed by moe_gate_scale.
struct RowScale {
  const float* ss;   // nullptr: no scaling
  int chunks;
  float inv_dim, eps;
  const float* gate = nullptr;
  int gld = 0, ge0 = 0, gF = 0;
};

// GEMM plan kinds. The numbers are the wire format (torch.ops.bfly.gemm_plan / gemm_plan_check /
// gemm_with_plan, BFLY_GEMM_PLAN, the rows of gemm_tuned.inc); 2 was the removed ring kernel.
enum GemmKind : int { kSkinny = 0, kTile = 1, kDec = 3, kBig8 = 4, kMid8 = 5, kBig4 = 6, kMid4 = 7, kTileMixed = 8 };

// A kernel family (`kind`) and the template instantiation of it; `sk` is the split-K factor of
// every kind. What the other fields hold ("-": not read):
//
//   kind        kernel                  mt                    nt                      wk                 bm     bn
//   kSkinny     gemm_skinny_kernel      16-token tiles        16-column weight tiles  waves splitting K  -      -
//                                       (M <= 16 mt)          per wave                (1, 2, 4)
//   kTile       gemm_tile_kernel        pipeline depth        - (1 on some table      waves along M      rows   columns
//                                       (0: 2)                rows: no meaning)
//   kDec        gemm_dec_kernel         weight ring depth     waves                   waves along M      rows   columns
//   kBig8       gemm_big8_kernel        -                     -                       -                  - (256 x 256)
//   kMid8       gemm_mid8_kernel        weight ring depth     activation ring depth   -                  rows   columns
//                                                             (0: that of the weight)
//   kBig4       gemm_wave4_kernel       -                     -                       -                  - (256 x 256)
//   kMid4       gemm_wave4_kernel       activation ring depth weight ring depth       -                  rows   columns
//   kTileMixed  gemm_tile_mixed_kernel  pipeline depth        -                       narrow columns     rows   wide columns
//                                       (0: 3)                                        (96)                      (128)
//
// Ring and pipeline depths count K-tiles of 64. A kind that is none of these runs as kTile.
struct GemmPlan {
  int kind;   // GemmKind
  int mt, nt, wk, bm, bn, sk;
};

// norm.hip
// `part` (optional): x is instead the sum of `sk` f32 split-K slabs [sk][rows][dim] of the
// producing GEMM (its deferred reduce fused here)
void launch_rmsnorm(const bf16* x, long x_stride, bf16* residual, const bf16* w, bf16* y,
                    long y_stride, int rows, int dim, float eps, bool add_residual,
                    hipStream_t stream, const float* part = nullptr, int sk = 0);
// launch_rmsnorm over split-K slabs that also routes every normalised row for a MoE layer
// (router_w [E][dim], E = 4 or 8): writes gates [rows][E], topk_ids / topk_w [rows][topk] as
// launch_moe_route would from y. < 0: unsupported.
int launch_rmsnorm_route(const float* part, int sk, bf16* residual, const bf16* w, bf16* y, int rows,
                         int dim, float eps, bool add_residual, const bf16* router_w, int E, int topk,
                         float* gates, int* topk_ids, float* topk_w, hipStream_t stream);
// Row-split add + RMSNorm whose consumer GEMM applies the row scale: writes y = x * w and the
// partial sums of squares ssp[rows][rmsnorm_rows_chunks(dim)]; pass RowScale{ssp, chunks, 1/dim,
// eps} to the GEMM that consumes y.
int rmsnorm_rows_chunks(int dim);
int launch_rmsnorm_rows(const bf16* x, long x_stride, bf16* residual, const bf16* w, bf16* y, float* ssp,
                        int rows, int dim, bool add_residual, hipStream_t stream,
                        const float* part = nullptr, int sk = 0);
void launch_layernorm(const bf16* x, bf16* residual, const bf16* w, const bf16* b, bf16* y,
                      int rows, int dim, float eps, bool add_residual, hipStream_t stream);

// rope.hip
// `part` (optional): the QKV row is the sum of `sk` f32 split-K slabs [sk][T][row] of the
// GEMM (deferred reduce fused here); the bf16 row is written to `qkv` as well
// Caches hold bf16, or FP8 e4m3 when `kv_fp8` (bfly_kv.h).
void launch_rope_kv(bf16* qkv, int T, int Hq, int Hkv, int D, const int* positions,
                    const float* cos_t, const float* sin_t, const int* slots, void* k_cache,
                    void* v_cache, int block_size, hipStream_t stream,
                    const float* part = nullptr, int sk = 0, int kv_fp8 = 0);
// launch_rope_kv with the per-head QK-norm of Qwen3 in front of the rotation: every Q / K head
// times rsqrt(mean of its squares + eps) times `q_norm_w` / `k_norm_w` (bf16 [D] each)
void launch_rope_qknorm_kv(bf16* qkv, int T, int Hq, int Hkv, int D, const int* positions,
                           const float* cos_t, const float* sin_t, const int* slots, void* k_cache,
                           void* v_cache, int block_size, hipStream_t stream, const float* part, int sk,
                           int kv_fp8, const bf16* q_norm_w, const bf16* k_norm_w, float eps);
void launch_kv_append(const bf16* k, long k_stride, const bf16* v, long v_stride,
                      const int* slots, void* k_cache, void* v_cache, int T, int Hkv, int D,
                      int block_size, hipStream_t stream, int kv_fp8 = 0);

// elementwise.hip
void launch_silu_mul(const bf16* gu, bf16* out, long rows, int ffn, int interleave,
                     hipStream_t stream);
void launch_gelu(const bf16* x, bf16* out, long n, hipStream_t stream);
void launch_add(const bf16* a, const bf16* b, bf16* out, long n, hipStream_t stream);
void launch_init_hash(bf16* out, long rows, int cols, long ld, long grow0, long gcol0, long gcols,
                      uint32_t seed, float amp, hipStream_t stream);
void launch_embed(const int* ids, const bf16* table, bf16* out, int T, int dim, int vstart,
                  int vlocal, hipStream_t stream);
// out[i, :] = src[idx[i], :] over rows of `words` 4-byte words (strides in words); idx < 0 or
// out of range leaves row i untouched
void launch_gather_rows(const void* src, long src_ld, const void* idx, bool idx64, void* out, long out_ld,
                        int words, long rows, long nsrc, hipStream_t stream);

// sample.hip
constexpr int kSampleMaxChunks = 64;
void launch_sample(const bf16* logits, long row_stride, int rows, int V, int vstart,
                   const float* temps, const long* seeds, uint64_t* workspace, int* out_ids,
                   float* out_scores, hipStream_t stream, const float* thresh = nullptr,
                   int check_finite = 0);
// TP merge of per-shard winners: pair [rows][2] f32 (score, id); allp [tp][rows][2] -> ids
void launch_sample_pack(const float* scores, const int* ids, float* pair, int rows, hipStream_t stream);
void launch_sample_merge(const float* allp, int tp, int rows, int* out, hipStream_t stream);
// exact top-k / top-p thresholds by radix select (sample.hip): state [rows, 8] f32 bits,
// smax [rows] int32 (zeroed), hist [rows, 512] f32 (zeroed); see the kernel comment
void launch_tkp_begin(const bf16* logits, long row_stride, int rows, int V, const float* temps,
                      const int* top_k, const float* top_p, float* state, int* smax, hipStream_t stream);
void launch_tkp_pass(const bf16* logits, long row_stride, int rows, int V, const float* temps,
                     float* state, const int* smax, float* hist, int pass, int phase, hipStream_t stream);
void launch_tkp_select(const float* top_p, float* state, float* hist, int rows, int pass, int phase,
                       hipStream_t stream);
void launch_tkp_final(const float* state, int rows, float* thresh, hipStream_t stream);

// logprobs.hip: log-softmax statistics and the n most likely tokens of each row of a (vocab
// shard of) logits. partial: record [rows][3 + 2n] f32 = (max, sum exp(x - max), logit of
// ids[row] or -inf when it lies outside the shard, n x (logit, global id; -inf, -1 = none)).
// merge: records [tp][rows][3 + 2n] -> chosen_lp [rows], top_ids / top_lp [rows][n].
constexpr int kLogprobsMaxN = 20;
constexpr int kLogprobsChunk = 4096;
constexpr int kLogprobsMaxChunks = 64;
inline int logprobs_chunks(int V) { return (V + kLogprobsChunk - 1) / kLogprobsChunk; }
// workspace of launch_logprobs_partial in u64 words
inline size_t logprobs_workspace_words(long rows, int V, int n) {
  return (size_t)rows * logprobs_chunks(V) * (2 + n);
}
void launch_logprobs_partial(const bf16* logits, long row_stride, int rows, int V, int vstart,
                             const int* ids, int n, uint64_t* workspace, float* record,
                             hipStream_t stream);
void launch_logprobs_merge(const float* records, int tp, int rows, int n, float* chosen_lp,
                           int* top_ids, float* top_lp, hipStream_t stream);

// penalties.hip: presence / frequency / repetition penalties, out of place. hist
// [hist_rows][hist_stride] int32 token histories (hist_stride % 4 == 0); per row: slots (< 0: the
// row is copied bit for bit), lens (tokens so far, the newest one being last[row], which is
// also stored to hist[slot][len - 1]), prompt_lens (positions below it are prompt tokens),
// params [rows][4] f32 (rep, 1 / rep, freq, pres). Row strides in elements.
constexpr int kPenaltyChunk = 4096;
inline int penalty_chunks(int V) { return (V + kPenaltyChunk - 1) / kPenaltyChunk; }
void launch_apply_penalties(const bf16* logits, long row_stride, int rows, int V, int vstart,
                            int* hist, long hist_stride, int hist_rows, const int* slots,
                            const int* lens, const int* prompt_lens, const int* last,
                            const float* params, bf16* out, long out_stride, hipStream_t stream);

// lora.hip: per-row LoRA delta of a projection's bf16 output. x [T][K] rows (ldx), a [S][J][K],
// b [S][N][R] bf16, J = nseg * R (nseg 1..3 logical projections fused in the weight), seg [N]
// uint8 (the rank slice of output row n, read once per aligned 16 rows and cut to nseg - 1),
// scale [S] f32, idx [T] int32 (outside [0, S): no adapter, the row of y is not written).
// part [KS][T][J] f32 holds the shrink's K-split partial sums; rows without an adapter are not
// written there and not read by the expand.
constexpr int kLoraMaxSplitK = 16;
int lora_splitk(int T, int K);                  // the K split ops.lora_add_ uses (any 1..16 runs)
int lora_check(int K, int J, int N, int R);     // 0, or < 0: K % 32, N % 16, R of 8 / 16 / 32 / 64, J = 1..3 R
void launch_lora_shrink(const bf16* x, long ldx, const bf16* a, const int* idx, float* part, int KS, int T,
                        int K, int J, int S, hipStream_t stream);
void launch_lora_expand(bf16* y, long ldy, const float* part, int KS, int T, int J, const bf16* b, int N, int R,
                        const uint8_t* seg, const float* scale, const int* idx, int S, hipStream_t stream);

// gemm.hip
GemmPlan plan_gemm(int M, int N, int K);
size_t gemm_workspace_bytes(int M, int N, int K);
int launch_gemm_plan(const GemmPlan& p, const bf16* X, long ldx, const bf16* W, long ldw, int M,
                     int N, int K, int epi, const bf16* bias, bf16* out, long ldo, float* ws,
                     size_t ws_bytes, hipStream_t stream, bool packed = false);
// 0 when `p` can run this shape and epilogue (`packed`: over a pack_w256 weight), < 0 otherwise;
// launches nothing
int gemm_plan_check(const GemmPlan& p, int M, int N, int K, int epi, bool packed);
// Mixed-width tile plans: 0 = never, 1 = the measured shapes, 2 = every shape they fit. Sets the
// mode (a value outside 0..2 only reads it) and returns the previous one.
int gemm_mixed_tiles_mode(int mode);
int gemm_check(int M, int N, int K, int epi);
// 0 if the auto plan for this shape takes a RowScale (tile and decode-ring kernels)
int gemm_rowscale_check(int M, int N, int K, int epi);
// Y = X W^T without epilogue; when the plan splits K, the f32 slabs are left in the workspace
// (at gemm_slab_offset_floats(), layout [sk][M][N]) for the consumer kernel to reduce, and the
// split count is returned; otherwise `out` is written and 1 is returned. < 0: error.
int launch_gemm_deferred(const bf16* X, long ldx, const bf16* W, long ldw, int M, int N, int K,
                         bf16* out, long ldo, float* ws, size_t ws_bytes, hipStream_t stream,
                         const RowScale* rs = nullptr);
size_t gemm_slab_offset_floats();
void launch_splitk_reduce(const float* part, int sk, int M, int N, bf16* out, long ldo,
                          hipStream_t stream);
int launch_gemm(const bf16* X, long ldx, const bf16* W, long ldw, int M, int N, int K, int epi,
                const bf16* bias, bf16* out, long ldo, float* ws, size_t ws_bytes,
                hipStream_t stream, const RowScale* rs = nullptr);
// out[M, N/2] = gate-scaled SwiGLU (EPI_SILU_GATE) on the tile kernel without split-K: the
// gate/up GEMM of the dense MoE decode path with moe_gate_scale folded into its epilogue.
// gates [M][gld] f32; output column f belongs to expert ge0 + f / gF.
// Decode GEMM over the K-tile-blocked copy Wp ([N/256][K/64][256][64]) of a weight, with the plan
// the row-major weight would run: < 0 (nothing launched) when that plan is not a 64-row tile plan.
// `rs`: row scale and / or MoE gate (EPI_SILU_GATE). Split-K plans need `ws`; with `defer` their
// slabs stay in it for the consumer (returns the split count), else they are reduced (returns 1).
int launch_gemm_packed(const bf16* X, long ldx, const bf16* Wp, int M, int N, int K, int epi, bf16* out,
                       long ldo, hipStream_t stream, const RowScale* rs = nullptr, float* ws = nullptr,
                       size_t ws_bytes = 0, bool defer = false);
// 0 when launch_gemm_packed applies to this shape and epilogue, else its error; launches nothing
int gemm_packed_check(int M, int N, int K, int epi);
int launch_gemm_silu_gate(const bf16* X, long ldx, const bf16* W, long ldw, int M, int N, int K,
                          bf16* out, long ldo, const float* gates, int gld, int ge0, int gF,
                          hipStream_t stream);

// gemm_w8.hip: FP8 e4m3 weight-only linear layers (codes [N][K] row-major, one f32 scale per row)
// code = RNE_e4m3fn(w / scale), scale = absmax(row) / 448 (1 for an all-zero row)
void launch_quant_fp8_rows(const bf16* w, long ldw, long N, int K, uint8_t* code, float* scale,
                           hipStream_t stream);
// out[n][k] = bf16(float(code[n][k]) * scale[n]); scale == nullptr: the bare codes (exact)
void launch_dequant_fp8(const uint8_t* code, const float* scale, long N, int K, bf16* out, long ldo,
                        hipStream_t stream);
// out = y[M][N] * scale[n] (EPI_NONE, in place allowed) or its SwiGLU [M][N/2] (EPI_SILU), y the
// bf16 GEMM result over bare codes; N % 32 == 0
void launch_w8_scale_cols(const bf16* y, long ldy, const float* scale, int M, int N, int epi, bf16* out,
                          long ldo, hipStream_t stream);
// 0 when the native kernel takes the shape (N % 128, K % 128, epilogue none / SiLU, M within
// its row limit); ops.linear_w8 dequantises and runs the bf16 GEMM otherwise
int gemm_w8_check(int M, int N, int K, int epi);
int gemm_w8_splitk(int M, int N, int K, int epi);        // the native plan's split-K factor (0: none)
size_t gemm_w8_workspace_bytes(int M, int N, int K);     // split-K slabs of the native plan
// Y = scale[n] * (X . code^T), epilogue none / SiLU. `any_m`: run the native kernel above its
// row limit too (64-row tiles, the weight re-streamed per tile), `force_sk`: another split-K
// factor than the heuristic's (both for measurements; a forced split needs a workspace of
// sk * M * N floats). < 0: not taken.
int launch_gemm_w8(const bf16* X, long ldx, const uint8_t* W, const float* scale, int M, int N, int K,
                   int epi, bf16* out, long ldo, float* ws, size_t ws_bytes, hipStream_t stream,
                   bool any_m = false, int force_sk = 0);
// Sum split-K slabs [sk][M][N] in a fixed order and apply the epilogue (none / SiLU); the slabs
// hold final f32 sums whatever the weight format, so gemm_w4.hip reduces through it too
void launch_gemm_wq_reduce(const float* part, int sk, int M, int N, int epi, bf16* out, long ldo,
                           hipStream_t stream);

// gemm_w4.hip: OCP MXFP4 weight-only linear layers: e2m1 codes [N][K / 2] (element 2 i in the low
// nibble of byte i), one e8m0 scale byte per 32 elements [N][K / 32]; K % 32 == 0
void launch_quant_mxfp4(const bf16* w, long ldw, long N, int K, uint8_t* code, uint8_t* scale,
                        hipStream_t stream);
// out[n][k] = bf16(value(code[n][k]) * 2^(scale[n][k / 32] - 127)), exact. Scale bytes must lie in
// 2 .. 252, the range the quantiser writes (every result a normal bf16); 0, 1, 253 - 255 are
// invalid input to the dequantiser and to the GEMM (0 gives 0, 255 infinity)
void launch_dequant_mxfp4(const uint8_t* code, const uint8_t* scale, long N, int K, bf16* out, long ldo,
                          hipStream_t stream);
// 0 when the native kernel takes the shape (N % 128, K % 128, epilogue none / SiLU, M within
// its row limit); ops.linear_w4 dequantises and runs the bf16 GEMM otherwise
int gemm_w4_check(int M, int N, int K, int epi);
int gemm_w4_splitk(int M, int N, int K, int epi);        // the native plan's split-K factor (0: none)
size_t gemm_w4_workspace_bytes(int M, int N, int K);     // split-K slabs of the native plan
// Y = X . dequant(code, scale)^T, epilogue none / SiLU; `any_m` and `force_sk` as in launch_gemm_w8.
// < 0: not taken.
int launch_gemm_w4(const bf16* X, long ldx, const uint8_t* W, const uint8_t* scale, int M, int N, int K,
                   int epi, bf16* out, long ldo, float* ws, size_t ws_bytes, hipStream_t stream,
                   bool any_m = false, int force_sk = 0);

// attention.hip
int attn_decode_splits(int max_ctx, int part_tokens);
int attn_decode_part_tokens(int B, int Hkv, int max_ctx);
int launch_attn_decode(const bf16* q, long q_stride, const void* k_cache, const void* v_cache,
                       const int* block_tables, int bt_stride, const int* ctx_lens, int B, int Hq,
                       int Hkv, int D, int block_size, float scale, int max_ctx, int part_tokens,
                       bf16* out, float* part_o, float* part_ml, hipStream_t stream,
                       int kv_fp8 = 0);            // caches hold FP8 e4m3 (bfly_kv.h)
// Multi-query paged decode attention of a speculative verify step (attention_verify.hip):
// q rows b * QN + t, row t of sequence b sees keys [0, ctx_lens[b] + min(t, q_lens[b] - 1)).
// QT = attn_verify_tiles(QN, Hq / Hkv) in 1 .. 4; the split geometry is attn_decode_part_tokens /
// attn_decode_splits over max_ctx + QN - 1 keys; partials carry 16 QT columns per split.
int attn_verify_tiles(int QN, int G);
int launch_attn_verify(const bf16* q, long q_stride, const void* k_cache, const void* v_cache,
                       const int* block_tables, int bt_stride, const int* ctx_lens, const int* q_lens, int B,
                       int QN, int Hq, int Hkv, int D, int block_size, float scale, int max_ctx, int part_tokens,
                       bf16* out, float* part_o, float* part_ml, hipStream_t stream, int kv_fp8 = 0);
int launch_attn_prefill(const bf16* q, long q_stride, const bf16* k, long k_stride, const bf16* v,
                        long v_stride, const int* cu_seqlens, int nseq, int max_seqlen, int Hq,
                        int Hkv, int D, float scale, bool causal, bf16* out, long o_stride,
                        hipStream_t stream, const int* cu_k = nullptr,
                        float* lse = nullptr);
// attention_paged.hip — chunked prefill over the paged cache: query rows [cu_q[s], cu_q[s+1])
// of sequence s at positions[row] attend causally to keys [0, positions[row]] read through
// tables[s] (the chunk's own K/V already appended). G = Hq / Hkv <= 8.
int launch_attn_prefill_paged(const bf16* q, long q_stride, const void* k_cache, const void* v_cache,
                              const int* tables, int bt_stride, const int* cu_q, const int* positions,
                              int nseq, int max_q, int Hq, int Hkv, int D, int block_size, float scale,
                              bf16* out, long o_stride, hipStream_t stream, int kv_fp8 = 0);
// K16 (context parallel): acc_o [T, H, 128] f32 / acc_lse [T, H] f32 absorb (o, lse).
int launch_attn_lse_merge(float* acc_o, float* acc_lse, const bf16* o, long o_stride,
                          const float* lse, int T, int H, int D, hipStream_t stream);

// allreduce.hip — one-shot IPC all-reduce (+ fused residual add / RMSNorm)
constexpr int kArBlocks = 128;
constexpr int kArMaxWorld = 8;
constexpr long kArDataOff = 65536;
// herr: this process's host-mapped health words (health_words_device()); a flag wait that
// times out also stores 1 into herr[kHealthCar] / herr[kHealthEp], which the host error
// poller reads without any HIP call (so it sees a stuck peer while the stream is still busy)
struct ArPeers { char* base[kArMaxWorld]; uint32_t* herr; };
constexpr int kHealthCar = 0, kHealthEp = 1, kHealthWords = 16;
uint32_t* health_words_device();        // lazily allocated pinned, mapped, coherent host memory
uint32_t health_word(int i);            // host read (no HIP call once allocated)
void health_clear(int word = -1);   // one word (kHealthCar / kHealthEp) or, -1, all of them
// flags/counters, two input buffers and two reduced-chunk buffers (two-shot), all double-buffered
inline long car_buffer_bytes(long cap) { return kArDataOff + 4 * cap; }
// `slabs` (optional): the input is split-K partials [sk][rows][dim] f32, reduced in the publish.
// `blocks`: the grid (<= kArBlocks), the same on every rank and for every call of a communicator:
// kArBlocks on a node (one rank per GPU); kArBlocks / world for ranks that share one GPU (tests),
// so the waves of ranks that arrived first and spin on their peers' flags can never occupy every
// CU — a late rank's one-workgroup-per-CU GEMM must still find CUs to run on.
int launch_custom_allreduce(const bf16* in, bf16* out, bf16* residual, const bf16* w, float eps,
                            int rows, int dim, const ArPeers& peers, int world, int rank,
                            long cap, hipStream_t stream, const float* slabs = nullptr, int sk = 0,
                            bool two_shot = false, int blocks = kArBlocks);
void* car_alloc(size_t bytes);
void car_free(void* p);
int car_ipc_handle(void* p, unsigned char* out64);
void* car_ipc_open(const unsigned char* h64);
void car_ipc_close(void* p);
int car_clear_error(void* base);
int car_error(const void* base);

// ep_ipc.hip — byte-minimal EP dispatch / return over peer IPC buffers (decode MoE)
constexpr long kEpHeaderBytes = 65536;
struct EpLayout { long x, ids, w, back, total; };   // byte offsets in a rank's buffer
EpLayout ep_ipc_layout(int ep, int capmax, int H, int K);
int launch_ep_ipc_dispatch(const bf16* x, const int* ids, const float* w, const int* slots, int T, int K,
                           int H, int El, int ep, int capmax, const ArPeers& peers, int rank, int* slot_out,
                           hipStream_t stream);
int launch_ep_ipc_wait(const ArPeers& peers, int ep, int rank, hipStream_t stream);
int launch_ep_ipc_return(const bf16* y, int H, int K, int ep, int capmax, const ArPeers& peers, int rank,
                         hipStream_t stream);
int launch_ep_ipc_combine(const int* slot, int T, int H, int K, int ep, int capmax, const ArPeers& peers,
                          int rank, bf16* out, hipStream_t stream);
// Prefill-sized dispatch (any T <= capmax): a one-workgroup scan routes the tokens (slot_out,
// per-destination totals), then one workgroup per token stores its row once into each owning
// rank's block; the last arriver publishes the row counts and raises the dispatch flags. The
// receive blocks are not marked row by row: consumers bound each block by its count
// (ep_ipc_counts_offset / launch_moe_align bcnt).
int launch_ep_ipc_dispatch_prefill(const bf16* x, const int* ids, const float* w, int T, int K, int H, int El,
                                   int ep, int capmax, const ArPeers& peers, int rank, int* slot_out,
                                   hipStream_t stream);
long ep_ipc_counts_offset();
int ep_ipc_stats(const void* base, long long* out2);
int ep_ipc_error(const void* base);

// moe.hip
int launch_moe_route(const bf16* x, long x_stride, const bf16* wr, int T, int H, int E, int K,
                     float* gates, int* topk_ids, float* topk_w, hipStream_t stream);
void launch_moe_gate_scale(bf16* h, const float* gates, long T, int E, int e0, int El, int F,
                           hipStream_t stream);

// sparse MoE (moe.hip + gemm.hip grouped tiles)
int moe_max_tiles(int TK, int El, int BM);
// bcnt / bcap (optional): rows are blocks of bcap rows, of which the first bcnt[block] are
// valid (EP IPC receive buffer): other rows get no slot and no combined output
int launch_moe_align(const int* topk_ids, int T, int K, int e0, int El, int BM, int* rows,
                     int* slot_of, int4* tiles, int* count, hipStream_t stream,
                     const int* bcnt = nullptr, int bcap = 0);
int launch_moe_combine(const bf16* y, const int* slot_of, const float* w, int T, int K, int H,
                       bf16* out, hipStream_t stream, const int* bcnt = nullptr, int bcap = 0);
constexpr int kMoeGroupBM = 64;
int launch_gemm_grouped(const bf16* X, long ldx, const bf16* W, long ldw, long w_estride, int N,
                        int K, int epi, const int* rows, const int4* tiles, const int* count,
                        int max_tiles, bf16* out, long ldo, hipStream_t stream, int bm = 64,
                        int slots = 0, int sk = 1, float* part = nullptr);
int launch_ep_pack(const bf16* x, const int* ids, const float* w, const int* slots, int T, int K, int H,
                   int El, int ep, int cap, bf16* send, float* meta, int* slot, hipStream_t stream);
int launch_ep_combine(const bf16* back, const int* slot, int T, int H, int ep, bf16* out, hipStream_t stream);
int launch_moe_combine_slabs(const float* part, int sk, long slab, const int* slot_of, const float* w,
                             int T, int K, int H, bf16* out, hipStream_t stream,
                             const int* bcnt = nullptr, int bcap = 0);

// probe.hip
void launch_probe(int which, float* out, hipStream_t stream);

}  // namespace bfly
