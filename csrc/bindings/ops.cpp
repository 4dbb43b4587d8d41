// torch.ops.bfly.* registrations for the HIP kernels in csrc/kernels.
//
// Every op validates shapes/dtypes/strides on the host (a bad shape must never reach a
// kernel: a GPU fault can reset every GPU of the host) and launches on the current HIP stream
// without allocating or synchronising, so whole decode steps can be captured in a hipGraph
// (torch.cuda.CUDAGraph on ROCm). Ops write into caller-provided outputs ("out" style): the
// engine owns static buffers, which is what graph replay needs.
//
// A binding builds an `Op` from its name and its anchor tensor and takes every other tensor
// argument through one of the Op's accessors; only the accessor section turns a tensor into a
// pointer (tests/test_ops_args_cpu.py holds the file to that).
#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <c10/core/DeviceGuard.h>
#include <torch/library.h>

#include <cmath>

#include "bfly_kernels.h"

namespace {

using at::Tensor;
using OptTensor = c10::optional<Tensor>;
using bfly::bf16;

// torch on ROCm exposes HIP devices as device type 'cuda'; the masquerading stream is the
// one torch.cuda.current_stream() returns (so ops order correctly with torch's own kernels).
inline hipStream_t cur_stream() { return at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream(); }

// ==== BEGIN TENSOR ACCESSORS ===============================================================
// The only code that reads a tensor's storage pointer. An accessor checks, in this order, that
// the argument is defined, lies on the op's device, has the expected dtype and has the layout
// the launcher assumes; its error reads "<op>: <argument> ...".
template <class T> struct DType;
template <> struct DType<bf16> { static constexpr at::ScalarType v = at::kBFloat16; };
template <> struct DType<float> { static constexpr at::ScalarType v = at::kFloat; };
template <> struct DType<int> { static constexpr at::ScalarType v = at::kInt; };
template <> struct DType<long> { static constexpr at::ScalarType v = at::kLong; };
template <> struct DType<uint64_t> { static constexpr at::ScalarType v = at::kLong; };   // bit patterns in int64 storage
template <> struct DType<uint8_t> { static constexpr at::ScalarType v = at::kByte; };   // MXFP4 codes and scales

// extra conditions of an accessor (`need`)
enum : unsigned { kAlign16 = 1, kAlign8 = 2, kLd8 = 4, kLd4 = 8 };   // base address; leading dimension % n

// pointer + leading dimension of a strided view: 2-D rows, or [T, H, D] rows of dense heads
template <class T> struct Rows { T* p; long ld; };

using Shape = std::initializer_list<int64_t>;   // -1: any size

// Row-major without gaps. Unlike Tensor::is_contiguous() an empty tensor does not pass
// whatever its strides: a view that would be strided with rows is refused without them too.
bool is_dense(const Tensor& t) {
  int64_t expect = 1;
  for (int64_t d = t.dim() - 1; d >= 0; --d) {
    const int64_t n = t.size(d);
    if (n == 1) continue;
    if (t.stride(d) != expect) return false;
    if (n == 0) return true;   // no element is addressed through the outer strides
    expect *= n;
  }
  return true;
}

struct Op {
  const char* name;
  c10::Device dev;

  Op(const char* name_, const Tensor& anchor, const char* arg) : name(name_), dev(c10::kCPU) {
    TORCH_CHECK(anchor.defined() && anchor.is_cuda(), name, ": ", arg, " must be a GPU tensor");
    dev = anchor.device();
  }
  c10::DeviceGuard guard() const { return c10::DeviceGuard(dev); }

  // defined, on the op's device, one of the dtypes `ok` (none listed: any)
  void check(const Tensor& t, const char* arg, std::initializer_list<at::ScalarType> ok = {}) const {
    TORCH_CHECK(t.defined(), name, ": ", arg, " is undefined");
    TORCH_CHECK(t.device() == dev, name, ": ", arg, " must be on ", dev, ", got ", t.device());
    bool match = ok.size() == 0;
    for (at::ScalarType st : ok) match |= t.scalar_type() == st;
    TORCH_CHECK(match, name, ": ", arg, " has dtype ", t.scalar_type(), ", expected ",
                ok.size() ? c10::toString(*ok.begin()) : "any");
  }
  void check_need(const Tensor& t, const char* arg, unsigned need, long ld) const {
    const uintptr_t a = reinterpret_cast<uintptr_t>(t.data_ptr());
    TORCH_CHECK(!(need & kAlign16) || a % 16 == 0, name, ": ", arg, " must be 16-B aligned");
    TORCH_CHECK(!(need & kAlign8) || a % 8 == 0, name, ": ", arg, " must be 8-B aligned");
    TORCH_CHECK(!(need & kLd8) || ld % 8 == 0, name, ": ", arg, " row stride must be a multiple of 8");
    TORCH_CHECK(!(need & kLd4) || ld % 4 == 0, name, ": ", arg, " row stride must be a multiple of 4");
  }
  void check_dense(const Tensor& t, const char* arg) const {
    TORCH_CHECK(is_dense(t), name, ": ", arg, " must be contiguous, got sizes ", t.sizes(), " strides ", t.strides());
  }
  void check_shape(const Tensor& t, const char* arg, Shape shape) const {
    bool ok = t.dim() == (int64_t)shape.size();
    int64_t d = 0;
    for (int64_t n : shape) {
      ok = ok && (n < 0 || t.size(d) == n);
      ++d;
    }
    TORCH_CHECK(ok, name, ": ", arg, " must have shape ", at::IntArrayRef(shape.begin(), shape.size()),
                " (-1: any), got ", t.sizes());
  }

  // ---- pointers the launcher takes without a stride: contiguous, sized by count or by shape ----
  void* flat_any(const Tensor& t, const char* arg, std::initializer_list<at::ScalarType> ok, unsigned need = 0) const {
    check(t, arg, ok);
    check_dense(t, arg);
    check_need(t, arg, need, 0);
    return t.data_ptr();
  }
  template <class T> T* flat(const Tensor& t, const char* arg, int64_t n, unsigned need = 0) const {
    void* p = flat_any(t, arg, {DType<T>::v}, need);
    TORCH_CHECK(t.numel() == n, name, ": ", arg, " must have ", n, " elements, got ", t.numel());
    return static_cast<T*>(p);
  }
  template <class T> T* flat_min(const Tensor& t, const char* arg, int64_t n, unsigned need = 0) const {
    void* p = flat_any(t, arg, {DType<T>::v}, need);
    TORCH_CHECK(t.numel() >= n, name, ": ", arg, " must have at least ", n, " elements, got ", t.numel());
    return static_cast<T*>(p);
  }
  template <class T> T* shaped(const Tensor& t, const char* arg, Shape shape, unsigned need = 0) const {
    check(t, arg, {DType<T>::v});
    check_shape(t, arg, shape);
    return static_cast<T*>(flat_any(t, arg, {}, need));
  }
  template <class T> T* flat(const OptTensor& t, const char* arg, int64_t n, unsigned need = 0) const {
    return t.has_value() ? flat<T>(*t, arg, n, need) : nullptr;
  }
  template <class T> T* shaped(const OptTensor& t, const char* arg, Shape shape, unsigned need = 0) const {
    return t.has_value() ? shaped<T>(*t, arg, shape, need) : nullptr;
  }
  // FP8 e4m3 codes (torch.float8_e4m3fn or uint8) and paged KV caches (bf16 or e4m3)
  uint8_t* codes(const Tensor& t, const char* arg, Shape shape) const {
    check(t, arg, {at::kFloat8_e4m3fn, at::kByte});
    check_shape(t, arg, shape);
    return static_cast<uint8_t*>(flat_any(t, arg, {}, kAlign16));
  }
  void* kv_cache(const Tensor& t, const char* arg, Shape shape, at::ScalarType st) const {
    check(t, arg, {st});
    check_shape(t, arg, shape);
    return flat_any(t, arg, {}, 0);
  }
  int4* tiles(const Tensor& t, const char* arg) const {   // MoE tile list [max_tiles, 4] int32
    return reinterpret_cast<int4*>(shaped<int>(t, arg, {-1, 4}));
  }
  // Exact top-k / top-p radix select (sample.hip): one zeroed f32 buffer holding
  // state [rows, 8] | smax [rows] (int32 bits) | hist [rows, 512].
  struct Tkp { float* state; int* smax; float* hist; };
  Tkp tkp_workspace(const Tensor& ws, const char* arg, int64_t rows) const {
    float* b = flat_min<float>(ws, arg, rows * (8 + 1 + 512));
    return {b, reinterpret_cast<int*>(b + rows * 8), b + rows * 9};
  }

  // ---- pointers passed with a leading dimension -------------------------------------------------
  // `shape` {rows, cols}; the view may be strided over rows
  Rows<void> rows_any(const Tensor& t, const char* arg, std::initializer_list<at::ScalarType> ok, Shape shape,
                      unsigned need = 0) const {
    check(t, arg, ok);
    check_shape(t, arg, shape);
    TORCH_CHECK(t.stride(1) == 1, name, ": ", arg, " must have unit inner stride");
    check_need(t, arg, need, t.stride(0));
    return {t.data_ptr(), (long)t.stride(0)};
  }
  template <class T> Rows<T> rows(const Tensor& t, const char* arg, Shape shape, unsigned need = 0) const {
    const Rows<void> r = rows_any(t, arg, {DType<T>::v}, shape, need);
    return {static_cast<T*>(r.p), r.ld};
  }
  // [T, H, D] whose heads are dense in a row; rows may be strided
  template <class T> Rows<T> heads(const Tensor& t, const char* arg, Shape shape, unsigned need = 0) const {
    check(t, arg, {DType<T>::v});
    check_shape(t, arg, shape);
    TORCH_CHECK(t.stride(2) == 1 && t.stride(1) == t.size(2), name, ": ", arg, " rows must be dense over heads");
    check_need(t, arg, need, t.stride(0));
    return {static_cast<T*>(t.data_ptr()), (long)t.stride(0)};
  }
};
// ==== END TENSOR ACCESSORS =================================================================

// ---- argument groups that several ops share ------------------------------------------------

// [rows, V] bf16 logits of the sampling ops
Rows<bf16> logits_rows(const Op& op, const Tensor& logits) {
  return op.rows<bf16>(logits, "logits", {-1, -1}, kAlign16 | kLd8);
}

// f32 split-K slabs [sk, rows, dim] (-1: any)
struct Slabs { float* p; int sk; };
Slabs slabs_of(const Op& op, const Tensor& t, const char* arg, int64_t rows, int64_t dim, unsigned need = 0) {
  float* p = op.shaped<float>(t, arg, {-1, rows, dim}, need);
  return {p, (int)t.size(0)};
}

// Paged KV cache pair: k_cache [blocks, Hkv, BS, D], v_cache [blocks, Hkv, D, BS], both bf16 or
// both FP8 e4m3 (torch.float8_e4m3fn). hkv < 0: taken from k_cache.
struct KvCaches { void *k, *v; int Hkv, BS, fp8; };
KvCaches kv_caches(const Op& op, const Tensor& k_cache, const Tensor& v_cache, int64_t hkv, int64_t D) {
  op.check(k_cache, "k_cache", {at::kBFloat16, at::kFloat8_e4m3fn});
  KvCaches c{};
  c.k = op.kv_cache(k_cache, "k_cache", {-1, hkv, -1, D}, k_cache.scalar_type());
  c.v = op.kv_cache(v_cache, "v_cache", {k_cache.size(0), k_cache.size(1), D, k_cache.size(2)}, k_cache.scalar_type());
  c.Hkv = k_cache.size(1);
  c.BS = k_cache.size(2);
  c.fp8 = k_cache.scalar_type() == at::kFloat8_e4m3fn;
  return c;
}

// X [M, K] . W [N, K]^T -> out [M, N / out_div] of the bf16 GEMMs
enum GemmWeight {
  kTileWeight,     // row-major, K % 64 == 0 and N % 128 == 0
  kPlanWeight,     // row-major, the explicit plan decides which shapes it takes
  kPackedWeight,   // the pack_w256 copy: contiguous
};
struct GemmOperands { Rows<bf16> x, w, out; int M, N, K; };
GemmOperands gemm_operands(const Op& op, const Tensor& x, const Tensor& w, const char* w_arg, const Tensor& out,
                           GemmWeight kind, bool silu, bool dense_out = false) {
  GemmOperands g{};
  g.x = op.rows<bf16>(x, "x", {-1, -1}, kAlign16 | kLd8);
  g.M = x.size(0);
  g.K = x.size(1);
  if (kind == kPackedWeight)
    g.w = {op.shaped<bf16>(w, w_arg, {-1, g.K}, kAlign16), (long)g.K};
  else
    g.w = op.rows<bf16>(w, w_arg, {-1, g.K}, kAlign16 | kLd8);
  g.N = w.size(0);
  if (kind == kTileWeight) {
    TORCH_CHECK(g.K % 64 == 0, op.name, ": K must be a multiple of 64, got ", g.K);
    TORCH_CHECK(g.N % 128 == 0, op.name, ": N must be a multiple of 128, got ", g.N);
  }
  const int64_t nout = silu ? g.N / 2 : g.N;
  if (dense_out)
    g.out = {op.shaped<bf16>(out, "out", {g.M, nout}), (long)nout};
  else
    g.out = op.rows<bf16>(out, "out", {g.M, nout});
  return g;
}

// optional f32 GEMM workspace -> (pointer, bytes)
struct Workspace { float* p; size_t bytes; };
Workspace workspace_of(const Op& op, const OptTensor& ws, unsigned need = 0) {
  if (!ws.has_value()) return {nullptr, 0};
  return {op.flat_min<float>(*ws, "workspace", 0, need), (size_t)ws->numel() * sizeof(float)};
}

// plan vector [kind, mt, nt, wk, bm, bn, sk]
bfly::GemmPlan plan_of(const char* op, const std::vector<int64_t>& plan) {
  TORCH_CHECK(plan.size() == 7, op, ": plan must be [kind, mt, nt, wk, bm, bn, sk]");
  bfly::GemmPlan p{};
  p.kind = plan[0]; p.mt = plan[1]; p.nt = plan[2]; p.wk = plan[3]; p.bm = plan[4]; p.bn = plan[5]; p.sk = plan[6];
  return p;
}

// RMSNorm row scale of a consumer GEMM: ssp [M, chunks] f32 partial sums of squares written by
// rms_norm_rows for X = x * g rows of width K.
bfly::RowScale row_scale(const Op& op, const Tensor& ssp, double eps, int M, int K) {
  const float* p = op.shaped<float>(ssp, "ssp", {M, -1});
  return bfly::RowScale{p, (int)ssp.size(1), 1.f / (float)K, (float)eps};
}

// MoE routing weights gates [M, E] f32 with this rank's experts e0 .. e0 + num_local
float* gates_of(const Op& op, const Tensor& gates, int64_t M, int64_t E = -1) {
  return op.shaped<float>(gates, "gates", {M, E});
}

// routing outputs topk_ids / topk_w [rows, k]
struct TopK { int* ids; float* w; };
TopK topk_outputs(const Op& op, const Tensor& topk_ids, const Tensor& topk_w, int64_t rows, int64_t k) {
  return {op.shaped<int>(topk_ids, "topk_ids", {rows, k}), op.shaped<float>(topk_w, "topk_w", {rows, k})};
}

// block counts (EP IPC receive buffer): rows form blocks of `bcap`; only the first bcnt[b] rows of
// block b are valid (device-resident counts, so no host sync)
const int* block_counts(const Op& op, const OptTensor& bcnt, int64_t bcap, long rows) {
  if (!bcnt.has_value()) return nullptr;
  TORCH_CHECK(bcap > 0 && rows % bcap == 0, op.name, ": block counts need bcap > 0 dividing the rows");
  return op.flat_min<int>(*bcnt, "bcnt", rows / bcap);
}

// weighted combine of expert outputs: slot_of [T * k], topk_w [T, k], out [T, H]
struct CombineArgs { const int* slot_of; const float* w; bf16* out; const int* bcnt; int T, K, H; };
CombineArgs combine_args(const Op& op, const Tensor& slot_of, const Tensor& topk_w, Tensor& out, const OptTensor& bcnt,
                         int64_t bcap) {
  CombineArgs c{};
  c.w = op.shaped<float>(topk_w, "topk_w", {-1, -1});
  c.T = topk_w.size(0);
  c.K = topk_w.size(1);
  c.slot_of = op.flat<int>(slot_of, "slot_of", (long)c.T * c.K);
  c.out = op.shaped<bf16>(out, "out", {c.T, -1});
  c.H = out.size(1);
  c.bcnt = block_counts(op, bcnt, bcap, c.T);
  return c;
}

// EP dispatch of x [T, H] by ids / w [T, k] (slots [T]: optional) into `ep` ranks of capacity `cap`
struct EpArgs { const bf16* x; const int* ids; const float* w; const int* slots; int* slot; int T, K, H; };
EpArgs ep_dispatch_args(const Op& op, const Tensor& x, const Tensor& ids, const Tensor& w, const OptTensor& slots,
                        int64_t cap, int64_t ep, Tensor& slot) {
  EpArgs a{};
  a.x = op.shaped<bf16>(x, "x", {-1, -1});
  a.T = x.size(0);
  a.H = x.size(1);
  a.ids = op.shaped<int>(ids, "ids", {a.T, -1});
  a.K = ids.size(1);
  a.w = op.flat<float>(w, "w", (long)a.T * a.K);
  TORCH_CHECK(cap >= a.T, op.name, ": more tokens than the buffer's capacity");
  a.slot = op.flat<int>(slot, "slot", (long)a.T * ep);
  a.slots = op.flat<int>(slots, "slots", a.T);
  return a;
}

// ---- ops -------------------------------------------------------------------------------------

void rms_norm(const Tensor& x, const Tensor& w, double eps, Tensor& out, const OptTensor& residual) {
  const Op op("rms_norm", x, "x");
  const Rows<bf16> xr = op.rows<bf16>(x, "x", {-1, -1}, kAlign16 | kLd8);
  const int rows = x.size(0), dim = x.size(1);
  TORCH_CHECK(dim % 8 == 0 && dim <= 16384, "rms_norm: dim must be a multiple of 8, <= 16384");
  const Rows<bf16> o = op.rows<bf16>(out, "out", {rows, dim}, kAlign16 | kLd8);
  const bf16* wp = op.flat<bf16>(w, "w", dim);
  bf16* res = op.shaped<bf16>(residual, "residual", {rows, dim});
  auto g = op.guard();
  bfly::launch_rmsnorm(xr.p, xr.ld, res, wp, o.p, o.ld, rows, dim, (float)eps, res != nullptr, cur_stream());
}

void layer_norm(const Tensor& x, const Tensor& w, const Tensor& b, double eps, Tensor& out,
                const OptTensor& residual) {
  const Op op("layer_norm", x, "x");
  const bf16* xp = op.shaped<bf16>(x, "x", {-1, -1});
  const int rows = x.size(0), dim = x.size(1);
  TORCH_CHECK(dim % 8 == 0 && dim <= 16384, "layer_norm: dim");
  bf16* res = op.shaped<bf16>(residual, "residual", {rows, dim});
  auto g = op.guard();
  bfly::launch_layernorm(xp, res, op.flat<bf16>(w, "w", dim), op.flat<bf16>(b, "b", dim),
                         op.shaped<bf16>(out, "out", {rows, dim}), rows, dim, (float)eps, res != nullptr, cur_stream());
}

// rope_kv and rope_qknorm_kv: with `q_norm_w` / `k_norm_w` (both or neither) the launch is the
// variant that RMS-normalises every Q / K head in front of the rotation
void rope_kv_any(const char* name, Tensor& qkv, const Tensor& positions, const Tensor& cos_t, const Tensor& sin_t,
                 int64_t num_q_heads, int64_t num_kv_heads, const OptTensor& slots, const OptTensor& k_cache,
                 const OptTensor& v_cache, const OptTensor& partial, const Tensor* q_norm_w, const Tensor* k_norm_w,
                 double eps) {
  const Op op(name, qkv, "qkv");
  bf16* qp = op.shaped<bf16>(qkv, "qkv", {-1, -1});
  const int T = qkv.size(0);
  TORCH_CHECK(num_q_heads >= 0 && num_kv_heads >= 0, name, ": negative head count");
  const int H = num_q_heads + 2 * num_kv_heads;
  TORCH_CHECK(H > 0 && qkv.size(1) % H == 0, name, ": row length not divisible by heads");
  const int D = qkv.size(1) / H;
  TORCH_CHECK(D == 128 || D == 64, name, ": head_dim must be 64 or 128");
  const int* pos = op.flat<int>(positions, "positions", T);
  const float* cp = op.flat_min<float>(cos_t, "cos", 0);
  TORCH_CHECK(cos_t.dim() >= 1 && cos_t.size(-1) == D / 2, name, ": cos must be [max_pos, D/2]");
  const float* sp = op.flat<float>(sin_t, "sin", cos_t.numel());
  TORCH_CHECK(sin_t.sizes() == cos_t.sizes(), name, ": sin must have the shape of cos");
  const int* sl = op.flat<int>(slots, "slots", T);
  KvCaches kv{nullptr, nullptr, 0, 1, 0};
  if (slots.has_value()) {
    TORCH_CHECK(k_cache.has_value() && v_cache.has_value(), name, ": caches required with slots");
    kv = kv_caches(op, *k_cache, *v_cache, num_kv_heads, D);
  }
  Slabs part{nullptr, 0};
  if (partial.has_value()) part = slabs_of(op, *partial, "partial", T, qkv.size(1));
  if (q_norm_w == nullptr) {
    auto g = op.guard();
    bfly::launch_rope_kv(qp, T, num_q_heads, num_kv_heads, D, pos, cp, sp, sl, kv.k, kv.v, kv.BS, cur_stream(),
                         part.p, part.sk, kv.fp8);
    return;
  }
  const bf16* qw = op.flat<bf16>(*q_norm_w, "q_norm_w", D, kAlign16);
  const bf16* kw = op.flat<bf16>(*k_norm_w, "k_norm_w", D, kAlign16);
  TORCH_CHECK(eps >= 0.0 && std::isfinite(eps), name, ": eps must be finite and >= 0");
  auto g = op.guard();
  bfly::launch_rope_qknorm_kv(qp, T, num_q_heads, num_kv_heads, D, pos, cp, sp, sl, kv.k, kv.v, kv.BS, cur_stream(),
                              part.p, part.sk, kv.fp8, qw, kw, (float)eps);
}

void rope_kv(Tensor& qkv, const Tensor& positions, const Tensor& cos_t, const Tensor& sin_t,
             int64_t num_q_heads, int64_t num_kv_heads, const OptTensor& slots, const OptTensor& k_cache,
             const OptTensor& v_cache, const OptTensor& partial) {
  rope_kv_any("rope_kv", qkv, positions, cos_t, sin_t, num_q_heads, num_kv_heads, slots, k_cache, v_cache, partial,
              nullptr, nullptr, 0.0);
}

void rope_qknorm_kv(Tensor& qkv, const Tensor& positions, const Tensor& cos_t, const Tensor& sin_t,
                    int64_t num_q_heads, int64_t num_kv_heads, const OptTensor& slots, const OptTensor& k_cache,
                    const OptTensor& v_cache, const Tensor& q_norm_w, const Tensor& k_norm_w, double eps,
                    const OptTensor& partial) {
  rope_kv_any("rope_qknorm_kv", qkv, positions, cos_t, sin_t, num_q_heads, num_kv_heads, slots, k_cache, v_cache,
              partial, &q_norm_w, &k_norm_w, eps);
}

void kv_append(const Tensor& k, const Tensor& v, const Tensor& slots, Tensor& k_cache, Tensor& v_cache) {
  const Op op("kv_append", k, "k");
  const Rows<bf16> kr = op.heads<bf16>(k, "k", {-1, -1, -1});
  const int T = k.size(0), Hkv = k.size(1), D = k.size(2);
  const Rows<bf16> vr = op.heads<bf16>(v, "v", {T, Hkv, D});
  TORCH_CHECK(D == 128 || D == 64, "kv_append: head_dim");
  const KvCaches kv = kv_caches(op, k_cache, v_cache, Hkv, D);
  auto g = op.guard();
  bfly::launch_kv_append(kr.p, kr.ld, vr.p, vr.ld, op.flat<int>(slots, "slots", T), kv.k, kv.v, T, Hkv, D, kv.BS,
                         cur_stream(), kv.fp8);
}

void silu_mul(const Tensor& gu, Tensor& out, int64_t interleave) {
  const Op op("silu_mul", gu, "gu");
  TORCH_CHECK(out.defined() && out.dim() >= 1 && gu.dim() >= 1, "silu_mul: shapes");
  const int ffn = out.size(-1);
  TORCH_CHECK(gu.size(-1) == 2 * ffn && ffn % 8 == 0 && ffn > 0, "silu_mul: shapes");
  TORCH_CHECK(interleave == 0 || (interleave % 8 == 0 && ffn % interleave == 0), "silu_mul: interleave");
  const long rows = out.numel() / ffn;
  bf16* o = op.flat<bf16>(out, "out", rows * ffn);
  auto g = op.guard();
  bfly::launch_silu_mul(op.flat<bf16>(gu, "gu", rows * 2 * ffn), o, rows, ffn, interleave, cur_stream());
}

void gelu(const Tensor& x, Tensor& out) {
  const Op op("gelu", x, "x");
  TORCH_CHECK(x.numel() % 8 == 0, "gelu: shapes");
  auto g = op.guard();
  bfly::launch_gelu(op.flat<bf16>(x, "x", x.numel()), op.flat<bf16>(out, "out", x.numel()), x.numel(), cur_stream());
}

void add(const Tensor& a, const Tensor& b, Tensor& out) {
  const Op op("add", a, "a");
  const long n = a.numel();
  TORCH_CHECK(n % 8 == 0, "add: shapes");
  auto g = op.guard();
  bfly::launch_add(op.flat<bf16>(a, "a", n), op.flat<bf16>(b, "b", n), op.flat<bf16>(out, "out", n), n, cur_stream());
}

void init_hash(Tensor& out, int64_t grow0, int64_t gcol0, int64_t gcols, int64_t seed, double amp) {
  const Op op("init_hash", out, "out");
  const Rows<bf16> o = op.rows<bf16>(out, "out", {-1, -1});
  auto g = op.guard();
  bfly::launch_init_hash(o.p, out.size(0), out.size(1), o.ld, grow0, gcol0, gcols, (uint32_t)seed, (float)amp,
                         cur_stream());
}

void embed(const Tensor& ids, const Tensor& table, Tensor& out, int64_t vstart) {
  const Op op("embed", ids, "ids");
  const bf16* tp = op.shaped<bf16>(table, "table", {-1, -1});
  const int T = ids.numel(), dim = table.size(1);
  TORCH_CHECK(dim % 8 == 0, "embed: shapes");
  auto g = op.guard();
  bfly::launch_embed(op.flat<int>(ids, "ids", T), tp, op.flat<bf16>(out, "out", (long)T * dim), T, dim, vstart,
                     table.size(0), cur_stream());
}

// zero a device buffer with the runtime's fill (no torch elementwise kernel in a trace)
void zero_(Tensor& t) {
  const Op op("zero_", t, "t");
  void* p = op.flat_any(t, "t", {});
  auto g = op.guard();
  if (t.numel() > 0)
    TORCH_CHECK(hipMemsetAsync(p, 0, t.numel() * t.element_size(), cur_stream()) == hipSuccess,
                "zero_: hipMemsetAsync failed");
}

// fill a 4-byte-element device buffer with one 32-bit pattern (runtime memset, no torch kernel)
void fill32_(Tensor& t, int64_t value) {
  const Op op("fill32_", t, "t");
  void* p = op.flat_any(t, "t", {});
  TORCH_CHECK(t.element_size() == 4, "fill32_: t must have 4-byte elements");
  auto g = op.guard();
  if (t.numel() > 0)
    TORCH_CHECK(hipMemsetD32Async(static_cast<hipDeviceptr_t>(p), (int)value, t.numel(), cur_stream()) == hipSuccess,
                "fill32_: hipMemsetD32Async failed");
}

void gather_rows(const Tensor& src, const Tensor& idx, Tensor& out) {
  const Op op("gather_rows", src, "src");
  const Rows<void> s = op.rows_any(src, "src", {}, {-1, -1});
  const void* ip = op.flat_any(idx, "idx", {at::kInt, at::kLong});
  TORCH_CHECK(idx.dim() == 1, "gather_rows: idx must be 1-D");
  const Rows<void> o = op.rows_any(out, "out", {src.scalar_type()}, {idx.numel(), src.size(1)});
  const long es = src.element_size();
  TORCH_CHECK((src.size(1) * es) % 4 == 0 && (s.ld * es) % 4 == 0 && (o.ld * es) % 4 == 0,
              "gather_rows: rows must be whole 4-byte words");
  auto g = op.guard();
  bfly::launch_gather_rows(s.p, s.ld * es / 4, ip, idx.scalar_type() == at::kLong, o.p, o.ld * es / 4,
                           (int)(src.size(1) * es / 4), out.size(0), src.size(0), cur_stream());
}

void sample_pack(const Tensor& scores, const Tensor& ids, Tensor& pair) {
  const Op op("sample_pack", scores, "scores");
  const long n = scores.numel();
  auto g = op.guard();
  bfly::launch_sample_pack(op.flat<float>(scores, "scores", n), op.flat<int>(ids, "ids", n),
                           op.flat<float>(pair, "pair", 2 * n), n, cur_stream());
}

void sample_merge(const Tensor& allp, Tensor& out) {
  const Op op("sample_merge", allp, "allp");
  const float* ap = op.shaped<float>(allp, "allp", {-1, -1, 2});
  auto g = op.guard();
  bfly::launch_sample_merge(ap, allp.size(0), allp.size(1), op.flat<int>(out, "out", allp.size(1)), cur_stream());
}

void sample(const Tensor& logits, const OptTensor& temps, const OptTensor& seeds, int64_t vstart, Tensor& out_ids,
            Tensor& out_scores, Tensor& workspace, const OptTensor& thresh, bool check_finite) {
  const Op op("sample", logits, "logits");
  const Rows<bf16> lg = logits_rows(op, logits);
  const int rows = logits.size(0), V = logits.size(1);
  auto g = op.guard();
  bfly::launch_sample(lg.p, lg.ld, rows, V, vstart, op.flat<float>(temps, "temps", rows),
                      op.flat<long>(seeds, "seeds", rows),
                      op.flat_min<uint64_t>(workspace, "workspace", (long)rows * bfly::kSampleMaxChunks),
                      op.flat<int>(out_ids, "out_ids", rows), op.flat<float>(out_scores, "out_scores", rows),
                      cur_stream(), op.flat<float>(thresh, "thresh", rows), check_finite ? 1 : 0);
}

// Per-token logprobs (logprobs.hip): one shard's record [rows, 3 + 2n] f32.
int64_t logprobs_workspace_size(int64_t rows, int64_t V, int64_t n) {
  return (int64_t)bfly::logprobs_workspace_words(rows, (int)V, (int)n);
}

void logprobs_partial(const Tensor& logits, const Tensor& ids, int64_t n, int64_t vstart, Tensor& record,
                      Tensor& workspace) {
  const Op op("logprobs_partial", logits, "logits");
  const Rows<bf16> lg = logits_rows(op, logits);
  const int64_t rows = logits.size(0), V = logits.size(1);
  TORCH_CHECK(n >= 0 && n <= bfly::kLogprobsMaxN, "logprobs_partial: n must be in 0..", bfly::kLogprobsMaxN);
  TORCH_CHECK(V <= (int64_t)bfly::kLogprobsChunk * bfly::kLogprobsMaxChunks, "logprobs_partial: at most ",
              bfly::kLogprobsChunk * bfly::kLogprobsMaxChunks, " columns");
  TORCH_CHECK(vstart >= 0 && vstart + V < (1ll << 24), "logprobs_partial: token ids must stay below 2^24");
  auto g = op.guard();
  bfly::launch_logprobs_partial(lg.p, lg.ld, rows, V, vstart, op.flat<int>(ids, "ids", rows), n,
                                op.flat_min<uint64_t>(workspace, "workspace", logprobs_workspace_size(rows, V, n)),
                                op.shaped<float>(record, "record", {rows, 3 + 2 * n}), cur_stream());
}

void logprobs_merge(const Tensor& records, Tensor& chosen_lp, Tensor& top_ids, Tensor& top_lp) {
  const Op op("logprobs_merge", records, "records");
  const float* rp = op.shaped<float>(records, "records", {-1, -1, -1});
  TORCH_CHECK(records.size(2) >= 3 && (records.size(2) - 3) % 2 == 0, "logprobs_merge: records [tp, rows, 3 + 2n] f32");
  const int64_t tp = records.size(0), rows = records.size(1), n = (records.size(2) - 3) / 2;
  TORCH_CHECK(tp >= 1 && n <= bfly::kLogprobsMaxN && tp * n <= bfly::kLogprobsMaxChunks * bfly::kLogprobsMaxN,
              "logprobs_merge: tp >= 1, n <= ", bfly::kLogprobsMaxN, ", tp * n <= ",
              bfly::kLogprobsMaxChunks * bfly::kLogprobsMaxN);
  auto g = op.guard();
  bfly::launch_logprobs_merge(rp, tp, rows, n, op.flat<float>(chosen_lp, "chosen_lp", rows),
                              op.flat<int>(top_ids, "top_ids", rows * n), op.flat<float>(top_lp, "top_lp", rows * n),
                              cur_stream());
}

// Presence / frequency / repetition penalties (penalties.hip): out [rows, V] bf16 = penalised logits.
void apply_penalties(const Tensor& logits, int64_t vstart, Tensor& hist, const Tensor& slots, const Tensor& lens,
                     const Tensor& prompt_lens, const Tensor& last, const Tensor& params, Tensor& out) {
  const Op op("apply_penalties", logits, "logits");
  const Rows<bf16> lg = logits_rows(op, logits);
  const int64_t rows = logits.size(0), V = logits.size(1);
  TORCH_CHECK(vstart >= 0 && vstart + V < (1ll << 24), "apply_penalties: token ids must stay below 2^24");
  const Rows<bf16> o = op.rows<bf16>(out, "out", {rows, V}, kAlign16 | kLd8);
  int* hp = op.shaped<int>(hist, "hist", {-1, -1}, kAlign16);
  TORCH_CHECK(hist.size(1) % 4 == 0 && hist.size(1) < 65536 && hist.size(0) < (1ll << 31),
              "apply_penalties: hist [slots, width] int32, width % 4 == 0 and < 65536");
  auto g = op.guard();
  bfly::launch_apply_penalties(lg.p, lg.ld, rows, V, vstart, hp, hist.size(1), hist.size(0),
                               op.flat<int>(slots, "slots", rows), op.flat<int>(lens, "lens", rows),
                               op.flat<int>(prompt_lens, "prompt_lens", rows), op.flat<int>(last, "last", rows),
                               op.shaped<float>(params, "params", {rows, 4}, kAlign16), o.p, o.ld, cur_stream());
}

void tkp_begin(const Tensor& logits, const Tensor& temps, const Tensor& top_k, const Tensor& top_p, Tensor& ws) {
  const Op op("tkp_begin", logits, "logits");
  const Rows<bf16> lg = logits_rows(op, logits);
  const int rows = logits.size(0);
  const Op::Tkp v = op.tkp_workspace(ws, "ws", rows);
  auto g = op.guard();
  bfly::launch_tkp_begin(lg.p, lg.ld, rows, logits.size(1), op.flat<float>(temps, "temps", rows),
                         op.flat<int>(top_k, "top_k", rows), op.flat<float>(top_p, "top_p", rows), v.state, v.smax,
                         cur_stream());
}

void tkp_pass(const Tensor& logits, const Tensor& temps, Tensor& ws, int64_t pass, int64_t phase) {
  const Op op("tkp_pass", logits, "logits");
  const Rows<bf16> lg = logits_rows(op, logits);
  TORCH_CHECK(pass >= 0 && pass < 4 && (phase == 0 || phase == 1), "tkp_pass: pass 0-3, phase 0/1");
  const int rows = logits.size(0);
  const Op::Tkp v = op.tkp_workspace(ws, "ws", rows);
  auto g = op.guard();
  bfly::launch_tkp_pass(lg.p, lg.ld, rows, logits.size(1), op.flat<float>(temps, "temps", rows), v.state, v.smax,
                        v.hist, (int)pass, (int)phase, cur_stream());
}

void tkp_select(const Tensor& top_p, Tensor& ws, int64_t rows, int64_t pass, int64_t phase) {
  const Op op("tkp_select", top_p, "top_p");
  TORCH_CHECK(rows >= 0 && pass >= 0 && pass < 4 && (phase == 0 || phase == 1), "tkp_select: pass 0-3, phase 0/1");
  const Op::Tkp v = op.tkp_workspace(ws, "ws", rows);
  auto g = op.guard();
  bfly::launch_tkp_select(op.flat<float>(top_p, "top_p", rows), v.state, v.hist, rows, (int)pass, (int)phase,
                          cur_stream());
}

void tkp_final(Tensor& ws, int64_t rows, Tensor& thresh) {
  const Op op("tkp_final", ws, "ws");
  TORCH_CHECK(rows >= 0, "tkp_final: rows");
  const Op::Tkp v = op.tkp_workspace(ws, "ws", rows);
  auto g = op.guard();
  bfly::launch_tkp_final(v.state, rows, op.flat<float>(thresh, "thresh", rows), cur_stream());
}

int64_t gemm_workspace_size(int64_t M, int64_t N, int64_t K) {
  return (int64_t)bfly::gemm_workspace_bytes(M, N, K);
}

std::vector<int64_t> gemm_plan(int64_t M, int64_t N, int64_t K) {
  const bfly::GemmPlan p = bfly::plan_gemm(M, N, K);
  return {p.kind, p.mt, p.nt, p.bm, p.bn, p.sk, p.wk};
}

// bias [N] of the EPI_BIAS epilogue (required with it, ignored otherwise)
const bf16* gemm_bias(const Op& op, const OptTensor& bias, int64_t epilogue, int N) {
  if (epilogue != bfly::EPI_BIAS) return nullptr;
  TORCH_CHECK(bias.has_value(), op.name, ": bias required by the bias epilogue");
  return op.flat<bf16>(bias, "bias", N);
}

// gemm(), and gemm_rs() with the consumer RMSNorm row scale (X rows = x * g of rms_norm_rows)
void gemm_impl(const Op& op, const Tensor& x, const Tensor& w, Tensor& out, const OptTensor& bias, int64_t epilogue,
               const OptTensor& workspace, const Tensor* ssp, double eps) {
  const GemmOperands a = gemm_operands(op, x, w, "w", out, kTileWeight, epilogue == bfly::EPI_SILU);
  const bf16* bp = gemm_bias(op, bias, epilogue, a.N);
  const Workspace ws = workspace_of(op, workspace);
  bfly::RowScale rs{};
  if (ssp != nullptr) rs = row_scale(op, *ssp, eps, a.M, a.K);
  auto g = op.guard();
  const int rc = bfly::launch_gemm(a.x.p, a.x.ld, a.w.p, a.w.ld, a.M, a.N, a.K, epilogue, bp, a.out.p, a.out.ld, ws.p,
                                   ws.bytes, cur_stream(), ssp != nullptr ? &rs : nullptr);
  TORCH_CHECK(rc == 0, op.name, ": unsupported shape M=", a.M, " N=", a.N, " K=", a.K, " (rc=", rc, ")");
}

void gemm(const Tensor& x, const Tensor& w, Tensor& out, const OptTensor& bias, int64_t epilogue,
          const OptTensor& workspace) {
  gemm_impl(Op("gemm", x, "x"), x, w, out, bias, epilogue, workspace, nullptr, 0.0);
}

void gemm_rs(const Tensor& x, const Tensor& w, Tensor& out, const OptTensor& bias, int64_t epilogue,
             const OptTensor& workspace, const Tensor& ssp, double eps) {
  gemm_impl(Op("gemm_rs", x, "x"), x, w, out, bias, epilogue, workspace, &ssp, eps);
}

// GEMM whose split-K reduce is left to the consumer: returns the split count (slabs in the
// workspace) or 1 (out written). gemm_deferred_rs: with the consumer RMSNorm row scale.
int64_t gemm_deferred_impl(const Op& op, const Tensor& x, const Tensor& w, Tensor& out, Tensor& workspace,
                           const Tensor* ssp, double eps) {
  const GemmOperands a = gemm_operands(op, x, w, "w", out, kTileWeight, false, true);
  const Workspace ws = workspace_of(op, workspace);
  bfly::RowScale rs{};
  if (ssp != nullptr) rs = row_scale(op, *ssp, eps, a.M, a.K);
  auto g = op.guard();
  const int rc = bfly::launch_gemm_deferred(a.x.p, a.x.ld, a.w.p, a.w.ld, a.M, a.N, a.K, a.out.p, a.out.ld, ws.p,
                                            ws.bytes, cur_stream(), ssp != nullptr ? &rs : nullptr);
  TORCH_CHECK(rc > 0, op.name, ": unsupported shape M=", a.M, " N=", a.N, " K=", a.K, " (rc=", rc, ")");
  return rc;
}

int64_t gemm_deferred(const Tensor& x, const Tensor& w, Tensor& out, Tensor& workspace) {
  return gemm_deferred_impl(Op("gemm_deferred", x, "x"), x, w, out, workspace, nullptr, 0.0);
}

int64_t gemm_deferred_rs(const Tensor& x, const Tensor& w, Tensor& out, Tensor& workspace, const Tensor& ssp,
                         double eps) {
  return gemm_deferred_impl(Op("gemm_deferred_rs", x, "x"), x, w, out, workspace, &ssp, eps);
}

// out[M, N/2] = moe_gate_scale(silu(gate) * up): the dense MoE decode gate/up GEMM over the
// concatenated local experts with the routing weights gates[M, E] applied in its epilogue.
void gemm_silu_gate(const Tensor& x, const Tensor& w, Tensor& out, const Tensor& gates, int64_t e0,
                    int64_t num_local) {
  const Op op("gemm_silu_gate", x, "x");
  const GemmOperands a = gemm_operands(op, x, w, "w", out, kTileWeight, true);
  const float* gp = gates_of(op, gates, a.M);
  TORCH_CHECK(num_local > 0 && (a.N / 2) % num_local == 0 && e0 >= 0 && e0 + num_local <= gates.size(1),
              "gemm_silu_gate: experts");
  const int F = (a.N / 2) / num_local;
  auto g = op.guard();
  const int rc = bfly::launch_gemm_silu_gate(a.x.p, a.x.ld, a.w.p, a.w.ld, a.M, a.N, a.K, a.out.p, a.out.ld, gp,
                                             (int)gates.size(1), (int)e0, F, cur_stream());
  TORCH_CHECK(rc == 0, "gemm_silu_gate: unsupported shape M=", a.M, " N=", a.N, " K=", a.K, " F=", F, " (rc=", rc, ")");
}

// Decode GEMM over the K-tile-blocked copy `wp` ([N/256][K/64][256][64] viewed as [N, K]) of a
// weight; optional RMSNorm row scale (ssp, eps) and MoE gate (gates, e0, num_local: epilogue 3).
// Returns 0 when it ran, < 0 when the shape's plan has no packed form (nothing launched).
int64_t gemm_packed(const Tensor& x, const Tensor& wp, Tensor& out, int64_t epilogue, const OptTensor& ssp, double eps,
                    const OptTensor& gates, int64_t e0, int64_t num_local, const OptTensor& workspace, bool defer) {
  const Op op("gemm_packed", x, "x");
  TORCH_CHECK(epilogue != bfly::EPI_BIAS, "gemm_packed: no bias epilogue");
  const bool silu = epilogue == bfly::EPI_SILU || epilogue == bfly::EPI_SILU_GATE;
  const GemmOperands a = gemm_operands(op, x, wp, "wp", out, kPackedWeight, silu);
  bfly::RowScale rs{nullptr, 0, 0.f, 0.f};
  if (ssp.has_value()) rs = row_scale(op, *ssp, eps, a.M, a.K);
  if (epilogue == bfly::EPI_SILU_GATE) {
    TORCH_CHECK(gates.has_value(), "gemm_packed: gates required by the gate epilogue");
    rs.gate = gates_of(op, *gates, a.M);
    TORCH_CHECK(num_local > 0 && (a.N / 2) % num_local == 0 && e0 + num_local <= gates->size(1), "gemm_packed: experts");
    rs.gld = (int)gates->size(1);
    rs.ge0 = (int)e0;
    rs.gF = (int)((a.N / 2) / num_local);
    if (rs.gF % 16 != 0) return -5;
  }
  const bool any = ssp.has_value() || epilogue == bfly::EPI_SILU_GATE;
  const Workspace ws = workspace_of(op, workspace);
  auto g = op.guard();
  return bfly::launch_gemm_packed(a.x.p, a.x.ld, a.w.p, a.M, a.N, a.K, (int)epilogue, a.out.p, a.out.ld, cur_stream(),
                                  any ? &rs : nullptr, ws.p, ws.bytes, defer);
}

// FP8 e4m3 weight-only linear layers (gemm_w8.hip). Codes are torch.float8_e4m3fn or uint8.
void quant_fp8_rows(const Tensor& w, Tensor& code, Tensor& scale) {
  const Op op("quant_fp8_rows", w, "w");
  const Rows<bf16> wr = op.rows<bf16>(w, "w", {-1, -1}, kAlign16);
  const int64_t N = w.size(0), K = w.size(1);
  TORCH_CHECK(K < (1LL << 31) && N < (1LL << 31), "quant_fp8_rows: shape");
  auto g = op.guard();
  bfly::launch_quant_fp8_rows(wr.p, wr.ld, N, (int)K, op.codes(code, "code", {N, K}), op.flat<float>(scale, "scale", N),
                              cur_stream());
}

void dequant_fp8(const Tensor& code, const OptTensor& scale, Tensor& out) {
  const Op op("dequant_fp8", code, "code");
  const uint8_t* cp = op.codes(code, "code", {-1, -1});
  const int64_t N = code.size(0), K = code.size(1);
  TORCH_CHECK(K < (1LL << 31), "dequant_fp8: shape");
  const Rows<bf16> o = op.rows<bf16>(out, "out", {N, K}, kAlign16 | kLd8);
  auto g = op.guard();
  bfly::launch_dequant_fp8(cp, op.flat<float>(scale, "scale", N), N, (int)K, o.p, o.ld, cur_stream());
}

void w8_scale_cols(const Tensor& y, const Tensor& scale, Tensor& out, int64_t epilogue) {
  const Op op("w8_scale_cols", y, "y");
  TORCH_CHECK(epilogue == bfly::EPI_NONE || epilogue == bfly::EPI_SILU, "w8_scale_cols: epilogue none / silu");
  const Rows<bf16> yr = op.rows<bf16>(y, "y", {-1, -1}, kAlign16 | kLd8);
  const int M = y.size(0), N = y.size(1);
  TORCH_CHECK(N % 32 == 0, "w8_scale_cols: N % 32");
  const Rows<bf16> o = op.rows<bf16>(out, "out", {M, epilogue == bfly::EPI_SILU ? N / 2 : N}, kAlign16 | kLd8);
  auto g = op.guard();
  bfly::launch_w8_scale_cols(yr.p, yr.ld, op.flat<float>(scale, "scale", N, kAlign16), M, N, (int)epilogue, o.p, o.ld,
                             cur_stream());
}

void gemm_w8(const Tensor& x, const Tensor& code, const Tensor& scale, Tensor& out, int64_t epilogue,
             const OptTensor& workspace, bool any_m, int64_t force_sk) {
  const Op op("gemm_w8", x, "x");
  TORCH_CHECK(epilogue == bfly::EPI_NONE || epilogue == bfly::EPI_SILU, "gemm_w8: epilogue none / silu");
  const Rows<bf16> xr = op.rows<bf16>(x, "x", {-1, -1}, kAlign16 | kLd8);
  const int M = x.size(0), K = x.size(1);
  const uint8_t* cp = op.codes(code, "code", {-1, K});
  const int N = code.size(0);
  const Rows<bf16> o = op.rows<bf16>(out, "out", {M, epilogue == bfly::EPI_SILU ? N / 2 : N}, kAlign8 | kLd4);
  const Workspace ws = workspace_of(op, workspace, kAlign16);
  auto g = op.guard();
  const int rc = bfly::launch_gemm_w8(xr.p, xr.ld, cp, op.flat<float>(scale, "scale", N, kAlign16), M, N, K,
                                      (int)epilogue, o.p, o.ld, ws.p, ws.bytes, cur_stream(), any_m, (int)force_sk);
  TORCH_CHECK(rc == 0, "gemm_w8: shape / plan not taken by the native kernel M=", M, " N=", N, " K=", K,
              " (rc=", rc, ")");
}

// OCP MXFP4 weight-only linear layers (gemm_w4.hip): uint8 codes [N, K / 2] (two e2m1 codes per
// byte), uint8 e8m0 scales [N, K / 32].
void quant_mxfp4(const Tensor& w, Tensor& code, Tensor& scale) {
  const Op op("quant_mxfp4", w, "w");
  const Rows<bf16> wr = op.rows<bf16>(w, "w", {-1, -1}, kAlign16 | kLd8);
  const int64_t N = w.size(0), K = w.size(1);
  TORCH_CHECK(K % 32 == 0 && K < (1LL << 31) && N < (1LL << 31), "quant_mxfp4: K % 32, shape");
  uint8_t* cp = op.shaped<uint8_t>(code, "code", {N, K / 2}, kAlign16);
  uint8_t* sp = op.shaped<uint8_t>(scale, "scale", {N, K / 32});
  auto g = op.guard();
  bfly::launch_quant_mxfp4(wr.p, wr.ld, N, (int)K, cp, sp, cur_stream());
}

void dequant_mxfp4(const Tensor& code, const Tensor& scale, Tensor& out) {
  const Op op("dequant_mxfp4", code, "code");
  const uint8_t* cp = op.shaped<uint8_t>(code, "code", {-1, -1}, kAlign16);
  const int64_t N = code.size(0), K = 2 * code.size(1);
  TORCH_CHECK(K % 32 == 0 && K < (1LL << 31), "dequant_mxfp4: K % 32, shape");
  const uint8_t* sp = op.shaped<uint8_t>(scale, "scale", {N, K / 32});
  const Rows<bf16> o = op.rows<bf16>(out, "out", {N, K}, kAlign16 | kLd8);
  auto g = op.guard();
  bfly::launch_dequant_mxfp4(cp, sp, N, (int)K, o.p, o.ld, cur_stream());
}

void gemm_w4(const Tensor& x, const Tensor& code, const Tensor& scale, Tensor& out, int64_t epilogue,
             const OptTensor& workspace, bool any_m, int64_t force_sk) {
  const Op op("gemm_w4", x, "x");
  TORCH_CHECK(epilogue == bfly::EPI_NONE || epilogue == bfly::EPI_SILU, "gemm_w4: epilogue none / silu");
  const Rows<bf16> xr = op.rows<bf16>(x, "x", {-1, -1}, kAlign16 | kLd8);
  const int M = x.size(0), K = x.size(1);
  TORCH_CHECK(K % 32 == 0, "gemm_w4: K % 32");
  const uint8_t* cp = op.shaped<uint8_t>(code, "code", {-1, K / 2}, kAlign16);
  const int N = code.size(0);
  const uint8_t* sp = op.shaped<uint8_t>(scale, "scale", {N, K / 32}, kAlign16);
  const Rows<bf16> o = op.rows<bf16>(out, "out", {M, epilogue == bfly::EPI_SILU ? N / 2 : N}, kAlign8 | kLd4);
  const Workspace ws = workspace_of(op, workspace, kAlign16);
  auto g = op.guard();
  const int rc = bfly::launch_gemm_w4(xr.p, xr.ld, cp, sp, M, N, K, (int)epilogue, o.p, o.ld, ws.p, ws.bytes,
                                      cur_stream(), any_m, (int)force_sk);
  TORCH_CHECK(rc == 0, "gemm_w4: shape / plan not taken by the native kernel M=", M, " N=", N, " K=", K,
              " (rc=", rc, ")");
}

// Multi-LoRA delta (lora.hip): part [KS, T, J] f32 takes the shrink's K-split partial sums, KS
// being the caller's choice (lora_splitk: the one ops.lora_add_ takes).
void lora_shrink(const Tensor& x, const Tensor& a, const Tensor& idx, Tensor& part) {
  const Op op("lora_shrink", x, "x");
  const Rows<bf16> xr = op.rows<bf16>(x, "x", {-1, -1}, kAlign16 | kLd8);
  const int64_t T = x.size(0), K = x.size(1);
  const bf16* ap = op.shaped<bf16>(a, "a", {-1, -1, K}, kAlign16);
  const int64_t S = a.size(0), J = a.size(1);
  TORCH_CHECK(K % 32 == 0 && K > 0 && K < (1LL << 31) && T < (1LL << 27), "lora_shrink: K % 32, shape");
  TORCH_CHECK(S >= 1 && S < (1LL << 20) && J >= 8 && J % 8 == 0 && J <= 192, "lora_shrink: a [S >= 1, J = 8 .. 192 (J % 8), K]");
  const int* ip = op.flat<int>(idx, "idx", T);
  float* pp = op.shaped<float>(part, "part", {-1, T, J}, kAlign16);
  const int64_t KS = part.size(0);
  TORCH_CHECK(KS >= 1 && KS <= bfly::kLoraMaxSplitK, "lora_shrink: part [KS = 1 .. ", bfly::kLoraMaxSplitK, ", T, J]");
  auto g = op.guard();
  bfly::launch_lora_shrink(xr.p, xr.ld, ap, ip, pp, (int)KS, (int)T, (int)K, (int)J, (int)S, cur_stream());
}

void lora_expand(Tensor& y, const Tensor& part, const Tensor& b, const Tensor& seg, const Tensor& scale,
                 const Tensor& idx) {
  const Op op("lora_expand", y, "y");
  const Rows<bf16> yr = op.rows<bf16>(y, "y", {-1, -1}, kAlign8 | kLd4);
  const int64_t T = y.size(0), N = y.size(1);
  const float* pp = op.shaped<float>(part, "part", {-1, T, -1}, kAlign16);
  const int64_t KS = part.size(0), J = part.size(2);
  const bf16* bp = op.shaped<bf16>(b, "b", {-1, N, -1}, kAlign16);
  const int64_t S = b.size(0), R = b.size(2);
  TORCH_CHECK(N < (1LL << 31) && T < (1LL << 27) && bfly::lora_check(32, (int)J, (int)N, (int)R) == 0,
              "lora_expand: N % 16, R of 8 / 16 / 32 / 64, J = nseg R with nseg 1 .. 3; got N=", N, " R=", R, " J=", J);
  TORCH_CHECK(S >= 1 && S < (1LL << 20) && KS >= 1 && KS <= bfly::kLoraMaxSplitK, "lora_expand: b [S >= 1, N, R], part [KS = 1 .. ",
              bfly::kLoraMaxSplitK, ", T, J]");
  const uint8_t* sp = op.shaped<uint8_t>(seg, "seg", {N});
  const float* cp = op.shaped<float>(scale, "scale", {S});
  const int* ip = op.flat<int>(idx, "idx", T);
  auto g = op.guard();
  bfly::launch_lora_expand(yr.p, yr.ld, pp, (int)KS, (int)T, (int)J, bp, (int)N, (int)R, sp, cp, ip, (int)S,
                           cur_stream());
}

// 0 when the plan for (M, N, K, epilogue) has a packed-weight form
int64_t gemm_packed_check(int64_t M, int64_t N, int64_t K, int64_t epilogue) {
  return bfly::gemm_packed_check((int)M, (int)N, (int)K, (int)epilogue);
}

// Dry run of an explicit plan [kind, mt, nt, wk, bm, bn, sk]: 0 when it can run the shape.
int64_t gemm_plan_check(std::vector<int64_t> plan, int64_t M, int64_t N, int64_t K, int64_t epilogue, bool packed) {
  return bfly::gemm_plan_check(plan_of("gemm_plan_check", plan), (int)M, (int)N, (int)K, (int)epilogue, packed);
}

// Benchmark / tuning entry: run an explicit plan [kind, mt, nt, wk, bm, bn, sk]. `packed`: `w` is
// the weight's pack_w256 copy (plans with a packed form only).
void gemm_with_plan(const Tensor& x, const Tensor& w, Tensor& out, std::vector<int64_t> plan, int64_t epilogue,
                    const OptTensor& workspace, const OptTensor& bias, bool packed) {
  const Op op("gemm_with_plan", x, "x");
  const bfly::GemmPlan p = plan_of(op.name, plan);
  const GemmOperands a =
      gemm_operands(op, x, w, "w", out, packed ? kPackedWeight : kPlanWeight, epilogue == bfly::EPI_SILU);
  TORCH_CHECK(!packed || (a.N % 256 == 0 && a.K % 64 == 0), "gemm_with_plan: packed weight");
  const Workspace ws = workspace_of(op, workspace);
  TORCH_CHECK(!bias.has_value() || epilogue == bfly::EPI_BIAS, "gemm_with_plan: bias without the bias epilogue");
  const bf16* bp = gemm_bias(op, bias, epilogue, a.N);
  auto g = op.guard();
  const int rc = bfly::launch_gemm_plan(p, a.x.p, a.x.ld, a.w.p, a.w.ld, a.M, a.N, a.K, epilogue, bp, a.out.p,
                                        a.out.ld, ws.p, ws.bytes, cur_stream(), packed);
  TORCH_CHECK(rc == 0, "gemm_with_plan: plan rejected (rc=", rc, ")");
}

// Row-split add + RMSNorm for a row-scaling consumer GEMM: out = x * w (un-normalised),
// ssp [rows, chunks] = per-chunk sums of squares. x: bf16 [rows, dim] or f32 slabs [sk, rows, dim].
void rms_norm_rows(const Tensor& x, const Tensor& w, Tensor& out, Tensor& ssp, const OptTensor& residual) {
  const Op op("rms_norm_rows", x, "x");
  Rows<bf16> xr{nullptr, 0};
  Slabs sl{nullptr, 0};
  if (x.scalar_type() == at::kFloat)
    sl = slabs_of(op, x, "x", -1, -1);
  else
    xr = op.rows<bf16>(x, "x", {-1, -1}, kAlign16 | kLd8);
  const int rows = x.size(x.dim() - 2), dim = x.size(x.dim() - 1);
  TORCH_CHECK(dim % 8 == 0, "rms_norm_rows: dim must be a multiple of 8");
  bf16* res = op.shaped<bf16>(residual, "residual", {rows, dim});
  auto g = op.guard();
  const int rc = bfly::launch_rmsnorm_rows(xr.p, xr.ld, res, op.flat<bf16>(w, "w", dim),
                                           op.shaped<bf16>(out, "out", {rows, dim}),
                                           op.shaped<float>(ssp, "ssp", {rows, bfly::rmsnorm_rows_chunks(dim)}), rows,
                                           dim, res != nullptr, cur_stream(), sl.p, sl.sk);
  TORCH_CHECK(rc == 0, "rms_norm_rows: launch failed (rc=", rc, ")");
}

void splitk_reduce(const Tensor& slabs, Tensor& out) {
  const Op op("splitk_reduce", slabs, "slabs");
  const Slabs sl = slabs_of(op, slabs, "slabs", -1, -1);
  const int M = slabs.size(1), N = slabs.size(2);
  bf16* o = op.shaped<bf16>(out, "out", {M, N});
  if (M == 0 || N == 0) return;   // the launcher has no empty-grid return
  auto g = op.guard();
  bfly::launch_splitk_reduce(sl.p, sl.sk, M, N, o, N, cur_stream());
}

void rms_norm_partial(const Tensor& slabs, const Tensor& w, double eps, Tensor& out, const OptTensor& residual) {
  const Op op("rms_norm_partial", slabs, "slabs");
  const Slabs sl = slabs_of(op, slabs, "slabs", -1, -1);
  const int rows = slabs.size(1), dim = slabs.size(2);
  TORCH_CHECK(dim % 8 == 0 && dim <= 16384, "rms_norm_partial: dim");
  bf16* res = op.shaped<bf16>(residual, "residual", {rows, dim});
  auto g = op.guard();
  bfly::launch_rmsnorm(nullptr, dim, res, op.flat<bf16>(w, "w", dim), op.shaped<bf16>(out, "out", {rows, dim}), dim,
                       rows, dim, (float)eps, res != nullptr, cur_stream(), sl.p, sl.sk);
}

// rms_norm_partial + MoE routing of the normalised rows (router_w [E, dim], E = 4 or 8)
void rms_norm_partial_route(const Tensor& slabs, const Tensor& w, double eps, Tensor& out, Tensor& residual,
                            const Tensor& router_w, int64_t top_k, Tensor& gates, Tensor& topk_ids, Tensor& topk_w) {
  const Op op("rms_norm_partial_route", slabs, "slabs");
  const Slabs sl = slabs_of(op, slabs, "slabs", -1, -1);
  const int rows = slabs.size(1), dim = slabs.size(2);
  TORCH_CHECK(dim % 8 == 0, "rms_norm_partial_route: dim");
  const bf16* rw = op.shaped<bf16>(router_w, "router_w", {-1, dim});
  const int E = router_w.size(0);
  const TopK tk = topk_outputs(op, topk_ids, topk_w, rows, top_k);
  auto g = op.guard();
  const int rc = bfly::launch_rmsnorm_route(sl.p, sl.sk, op.shaped<bf16>(residual, "residual", {rows, dim}),
                                            op.flat<bf16>(w, "w", dim), op.shaped<bf16>(out, "out", {rows, dim}), rows,
                                            dim, (float)eps, true, rw, E, (int)top_k,
                                            gates_of(op, gates, rows, E), tk.ids, tk.w,
                                            cur_stream());
  TORCH_CHECK(rc == 0, "rms_norm_partial_route: unsupported (E=", E, ", dim=", dim, ", rc=", rc, ")");
}

int64_t rms_norm_route_ok(int64_t E, int64_t dim) { return (E == 4 || E == 8) && dim % 8 == 0 && dim <= 16384 ? 1 : 0; }

int64_t attn_decode_splits(int64_t max_ctx, int64_t part_tokens) {
  return bfly::attn_decode_splits(max_ctx, part_tokens);
}

int64_t attn_decode_part_tokens(int64_t B, int64_t Hkv, int64_t max_ctx) {
  return bfly::attn_decode_part_tokens(B, Hkv, max_ctx);
}

void attn_decode(const Tensor& q, const Tensor& k_cache, const Tensor& v_cache, const Tensor& block_tables,
                 const Tensor& ctx_lens, double scale, int64_t max_ctx, int64_t part_tokens, Tensor& out,
                 const OptTensor& part_o, const OptTensor& part_ml) {
  const Op op("attn_decode", q, "q");
  const Rows<bf16> qr = op.heads<bf16>(q, "q", {-1, -1, -1});
  const int B = q.size(0), Hq = q.size(1), D = q.size(2);
  const KvCaches kv = kv_caches(op, k_cache, v_cache, -1, D);
  const Rows<int> bt = op.rows<int>(block_tables, "block_tables", {-1, -1});
  TORCH_CHECK(block_tables.size(0) >= B, "attn_decode: block_tables has fewer rows than q");
  TORCH_CHECK((long)block_tables.size(1) * kv.BS >= max_ctx, "attn_decode: block table too narrow for max_ctx");
  if (part_tokens <= 0) part_tokens = bfly::attn_decode_part_tokens(B, kv.Hkv, max_ctx);
  const int nsplit = bfly::attn_decode_splits(max_ctx, part_tokens);
  float *po = nullptr, *pml = nullptr;
  if (nsplit > 1) {
    TORCH_CHECK(part_o.has_value() && part_ml.has_value(), "attn_decode: partial buffers required");
    po = op.flat_min<float>(*part_o, "part_o", (long)B * kv.Hkv * nsplit * 16 * D);
    pml = op.flat_min<float>(*part_ml, "part_ml", (long)B * kv.Hkv * nsplit * 16 * 2);
  }
  auto g = op.guard();
  const int rc = bfly::launch_attn_decode(qr.p, qr.ld, kv.k, kv.v, bt.p, bt.ld, op.flat_min<int>(ctx_lens, "ctx_lens", B),
                                          B, Hq, kv.Hkv, D, kv.BS, (float)scale, max_ctx, part_tokens,
                                          op.flat<bf16>(out, "out", (long)B * Hq * D), po, pml, cur_stream(), kv.fp8);
  TORCH_CHECK(rc == 0, "attn_decode: unsupported configuration (rc=", rc, ")");
}

// Multi-query paged decode attention of a speculative verify step (attention_verify.hip):
// q [B, QN, Hq, D] (rows may be strided, as a view into fused QKV rows), out [B, QN, Hq, D]
// dense. Row t of sequence b sees keys [0, ctx_lens[b] + min(t, q_lens[b] - 1)); max_ctx bounds
// ctx_lens. Splits: attn_decode_part_tokens / attn_decode_splits over max_ctx + QN - 1 keys.
int64_t attn_verify_tiles(int64_t QN, int64_t G) { return bfly::attn_verify_tiles((int)QN, (int)G); }

void attn_verify(const Tensor& q, const Tensor& k_cache, const Tensor& v_cache, const Tensor& block_tables,
                 const Tensor& ctx_lens, const Tensor& q_lens, double scale, int64_t max_ctx, int64_t part_tokens,
                 Tensor& out, const OptTensor& part_o, const OptTensor& part_ml) {
  const Op op("attn_verify", q, "q");
  op.check(q, "q", {at::kBFloat16});
  op.check_shape(q, "q", {-1, -1, -1, -1});
  const int64_t B = q.size(0), QN = q.size(1), Hq = q.size(2), D = q.size(3);
  TORCH_CHECK(QN >= 1 && B < (1LL << 20) && B * QN < (1LL << 24), "attn_verify: q [B, QN >= 1, Hq, D]");
  TORCH_CHECK(QN == 1 || B <= 1 || q.stride(0) == QN * q.stride(1), "attn_verify: q rows b * QN + t must be evenly strided, got strides ",
              q.strides());
  const Rows<bf16> qr = op.heads<bf16>(at::as_strided(q, {B * QN, Hq, D}, {QN == 1 ? q.stride(0) : q.stride(1), q.stride(2), q.stride(3)}),
                                       "q", {B * QN, Hq, D}, kAlign16 | kLd8);
  const KvCaches kv = kv_caches(op, k_cache, v_cache, -1, D);
  TORCH_CHECK(D == 128 && kv.BS == 32, "attn_verify: head_dim 128 and 32-token pages, got D=", D, " BS=", kv.BS);
  TORCH_CHECK(kv.Hkv > 0 && Hq % kv.Hkv == 0 && QN * (Hq / kv.Hkv) <= 64, "attn_verify: QN * (Hq / Hkv) must be <= 64, got QN=", QN,
              " Hq=", Hq, " Hkv=", kv.Hkv);
  TORCH_CHECK(max_ctx >= 0 && max_ctx < (1LL << 30), "attn_verify: max_ctx");
  const int keys = (int)(max_ctx + QN - 1);
  const Rows<int> bt = op.rows<int>(block_tables, "block_tables", {-1, -1});
  TORCH_CHECK(block_tables.size(0) >= B, "attn_verify: block_tables has fewer rows than q");
  TORCH_CHECK((long)block_tables.size(1) * kv.BS >= keys, "attn_verify: block table too narrow for max_ctx + QN - 1");
  if (part_tokens <= 0) part_tokens = bfly::attn_decode_part_tokens(B, kv.Hkv, keys);
  TORCH_CHECK(part_tokens % kv.BS == 0, "attn_verify: part_tokens must be a multiple of the page size");
  const int nsplit = bfly::attn_decode_splits(keys, part_tokens);
  const int NC = 16 * bfly::attn_verify_tiles(QN, Hq / kv.Hkv);
  float *po = nullptr, *pml = nullptr;
  if (nsplit > 1) {
    TORCH_CHECK(part_o.has_value() && part_ml.has_value(), "attn_verify: partial buffers required");
    po = op.flat_min<float>(*part_o, "part_o", (long)B * kv.Hkv * nsplit * NC * D);
    pml = op.flat_min<float>(*part_ml, "part_ml", (long)B * kv.Hkv * nsplit * NC * 2);
  }
  const int* cl = op.flat_min<int>(ctx_lens, "ctx_lens", B);
  const int* qlp = op.flat_min<int>(q_lens, "q_lens", B);
  bf16* o = op.shaped<bf16>(out, "out", {B, QN, Hq, D});
  auto g = op.guard();
  const int rc = bfly::launch_attn_verify(qr.p, qr.ld, kv.k, kv.v, bt.p, bt.ld, cl, qlp, B, QN, Hq, kv.Hkv, D, kv.BS,
                                          (float)scale, max_ctx, part_tokens, o, po, pml, cur_stream(), kv.fp8);
  TORCH_CHECK(rc == 0, "attn_verify: unsupported configuration (rc=", rc, ")");
}

// Chunked prefill over the paged cache (attention_paged.hip): q [T, Hq, D] rows grouped per
// sequence by cu_q, positions [T] their absolute positions, tables [nseq, max_blocks].
void attn_prefill_paged(const Tensor& q, const Tensor& k_cache, const Tensor& v_cache, const Tensor& tables,
                        const Tensor& cu_q, const Tensor& positions, int64_t max_q, double scale, Tensor& out) {
  const Op op("attn_prefill_paged", q, "q");
  const Rows<bf16> qr = op.heads<bf16>(q, "q", {-1, -1, -1});
  const int T = q.size(0), Hq = q.size(1), D = q.size(2);
  const Rows<bf16> o = op.heads<bf16>(out, "out", {T, Hq, D});
  const KvCaches kv = kv_caches(op, k_cache, v_cache, -1, D);
  const int* cu = op.flat_min<int>(cu_q, "cu_q", 1);
  const int nseq = cu_q.numel() - 1;
  const Rows<int> bt = op.rows<int>(tables, "tables", {-1, -1});
  TORCH_CHECK(tables.size(0) >= nseq, "attn_prefill_paged: tables has fewer rows than sequences");
  auto g = op.guard();
  const int rc = bfly::launch_attn_prefill_paged(qr.p, qr.ld, kv.k, kv.v, bt.p, bt.ld, cu,
                                                 op.flat_min<int>(positions, "positions", T), nseq, (int)max_q, Hq,
                                                 kv.Hkv, D, kv.BS, (float)scale, o.p, o.ld, cur_stream(), kv.fp8);
  TORCH_CHECK(rc == 0, "attn_prefill_paged: unsupported configuration (rc=", rc, ")");
}

void attn_prefill(const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& cu_seqlens, int64_t max_seqlen,
                  double scale, bool causal, Tensor& out, const OptTensor& cu_seqlens_k, const OptTensor& lse) {
  const Op op("attn_prefill", q, "q");
  const Rows<bf16> qr = op.heads<bf16>(q, "q", {-1, -1, -1}, kLd8);
  const int T = q.size(0), Hq = q.size(1), D = q.size(2);
  const Rows<bf16> kr = op.heads<bf16>(k, "k", {-1, -1, D}, kLd8);
  const int Hkv = k.size(1);
  const Rows<bf16> vr = op.heads<bf16>(v, "v", {-1, Hkv, D}, kLd8);
  const Rows<bf16> o = op.heads<bf16>(out, "out", {T, Hq, D}, kLd8);
  const int* cu = op.flat_min<int>(cu_seqlens, "cu_seqlens", 1);
  const int nseq = cu_seqlens.numel() - 1;
  // keys from another chunk (context-parallel ring step)
  const int* cuk = op.flat<int>(cu_seqlens_k, "cu_seqlens_k", nseq + 1);
  TORCH_CHECK(cuk == nullptr || !causal, "attn_prefill: separate key offsets are only defined for non-causal attention");
  auto g = op.guard();
  const int rc = bfly::launch_attn_prefill(qr.p, qr.ld, kr.p, kr.ld, vr.p, vr.ld, cu, nseq, max_seqlen, Hq, Hkv, D,
                                           (float)scale, causal, o.p, o.ld, cur_stream(), cuk,
                                           op.flat<float>(lse, "lse", (long)T * Hq));
  TORCH_CHECK(rc == 0, "attn_prefill: unsupported configuration (rc=", rc, ")");
}

void attn_lse_merge(Tensor& acc_o, Tensor& acc_lse, const Tensor& o, const Tensor& lse) {
  const Op op("attn_lse_merge", acc_o, "acc_o");
  float* ao = op.shaped<float>(acc_o, "acc_o", {-1, -1, 128});
  const int T = acc_o.size(0), H = acc_o.size(1);
  const Rows<bf16> orow = op.heads<bf16>(o, "o", {T, H, 128});
  auto g = op.guard();
  const int rc = bfly::launch_attn_lse_merge(ao, op.flat<float>(acc_lse, "acc_lse", (int64_t)T * H), orow.p, orow.ld,
                                             op.flat<float>(lse, "lse", (int64_t)T * H), T, H, 128, cur_stream());
  TORCH_CHECK(rc == 0, "attn_lse_merge: rejected (", rc, ")");
}

void moe_route(const Tensor& x, const Tensor& wr, int64_t top_k, Tensor& gates, Tensor& topk_ids, Tensor& topk_w) {
  const Op op("moe_route", x, "x");
  const Rows<bf16> xr = op.rows<bf16>(x, "x", {-1, -1}, kLd8);
  const int T = x.size(0), H = x.size(1);
  const bf16* wp = op.shaped<bf16>(wr, "wr", {-1, H});
  const int E = wr.size(0);
  const TopK tk = topk_outputs(op, topk_ids, topk_w, T, top_k);
  auto g = op.guard();
  const int rc = bfly::launch_moe_route(xr.p, xr.ld, wp, T, H, E, top_k, gates_of(op, gates, T, E),
                                        tk.ids, tk.w, cur_stream());
  TORCH_CHECK(rc == 0, "moe_route: unsupported (E <= 64, k <= 8, H % 8 == 0)");
}

int64_t moe_max_tiles(int64_t TK, int64_t El, int64_t bm) { return bfly::moe_max_tiles(TK, El, (int)bm); }

void moe_align(const Tensor& topk_ids, int64_t e0, int64_t num_local, Tensor& rows, Tensor& slot_of, Tensor& tiles,
               Tensor& count, int64_t bm, const OptTensor& bcnt, int64_t bcap) {
  TORCH_CHECK(bm == 64 || bm == 128 || bm == 256, "moe_align: tile rows 64, 128 or 256");
  const Op op("moe_align", topk_ids, "topk_ids");
  const int* ids = op.shaped<int>(topk_ids, "topk_ids", {-1, -1});
  const int T = topk_ids.size(0), K = topk_ids.size(1);
  TORCH_CHECK(num_local > 0 && num_local <= 64, "moe_align: 1..64 local experts");
  int4* tp = op.tiles(tiles, "tiles");
  TORCH_CHECK(tiles.size(0) >= bfly::moe_max_tiles(T * K, num_local, (int)bm), "moe_align: tiles [max_tiles, 4]");
  const int* bc = block_counts(op, bcnt, bcap, T);
  auto g = op.guard();
  const int rc = bfly::launch_moe_align(ids, T, K, e0, num_local, (int)bm, op.flat_min<int>(rows, "rows", (long)T * K),
                                        op.flat<int>(slot_of, "slot_of", (long)T * K), tp,
                                        op.flat<int>(count, "count", 1), cur_stream(), bc, (int)bcap);
  TORCH_CHECK(rc == 0, "moe_align: rejected (", rc, ")");
}

void moe_grouped_gemm(const Tensor& x, const Tensor& w, Tensor& out, const OptTensor& rows, const Tensor& tiles,
                      const Tensor& count, int64_t w_estride, int64_t n, int64_t k, int64_t num_experts,
                      int64_t epilogue, int64_t bm, const OptTensor& part) {
  const Op op("moe_grouped_gemm", x, "x");
  const Rows<bf16> xr = op.rows<bf16>(x, "x", {-1, -1}, kLd8);
  TORCH_CHECK(x.size(1) >= k, "moe_grouped_gemm: x has fewer than k columns");
  const Rows<bf16> wr = op.rows<bf16>(w, "w", {-1, -1}, kLd8);
  TORCH_CHECK(n % 128 == 0 && k % 64 == 0, "moe_grouped_gemm: N % 128, K % 64");
  TORCH_CHECK(epilogue == bfly::EPI_NONE || epilogue == bfly::EPI_SILU, "moe_grouped_gemm: epilogue");
  const long last = (num_experts - 1) * w_estride + (n - 1) * wr.ld + k;
  TORCH_CHECK(num_experts > 0 && last <= w.numel(), "moe_grouped_gemm: expert slices exceed w");
  const Rows<bf16> o = op.rows<bf16>(out, "out", {-1, epilogue == bfly::EPI_SILU ? n / 2 : n});
  const int slots = out.size(0);
  const int* rp = nullptr;
  if (rows.has_value())
    rp = op.flat_min<int>(*rows, "rows", 0);
  else
    TORCH_CHECK(x.size(0) >= slots, "moe_grouped_gemm: slot rows");
  const int4* tp = op.tiles(tiles, "tiles");
  const int* cp = op.flat_min<int>(count, "count", 1);
  Slabs pt{nullptr, 1};   // split-K: f32 slabs [sk][slots][n], reduced by moe_combine_slabs
  if (part.has_value()) {
    TORCH_CHECK(epilogue == bfly::EPI_NONE, "moe_grouped_gemm: part slabs take no epilogue");
    pt = slabs_of(op, *part, "part", slots, n);
  }
  if (slots == 0) return;   // the launcher sizes its grid by the tile list alone
  auto g = op.guard();
  const int rc = bfly::launch_gemm_grouped(xr.p, xr.ld, wr.p, wr.ld, w_estride, n, k, epilogue, rp, tp, cp,
                                           tiles.size(0), o.p, o.ld, cur_stream(), (int)bm, slots, pt.sk, pt.p);
  TORCH_CHECK(rc == 0, "moe_grouped_gemm: rejected (", rc, ")");
}

void moe_combine(const Tensor& y, const Tensor& slot_of, const Tensor& topk_w, Tensor& out, const OptTensor& bcnt,
                 int64_t bcap) {
  const Op op("moe_combine", y, "y");
  const CombineArgs c = combine_args(op, slot_of, topk_w, out, bcnt, bcap);
  auto g = op.guard();
  const int rc = bfly::launch_moe_combine(op.shaped<bf16>(y, "y", {-1, c.H}), c.slot_of, c.w, c.T, c.K, c.H, c.out,
                                          cur_stream(), c.bcnt, (int)bcap);
  TORCH_CHECK(rc == 0, "moe_combine: H % 8");
}

void moe_combine_slabs(const Tensor& part, const Tensor& slot_of, const Tensor& topk_w, Tensor& out,
                       const OptTensor& bcnt, int64_t bcap) {
  const Op op("moe_combine_slabs", part, "part");
  const CombineArgs c = combine_args(op, slot_of, topk_w, out, bcnt, bcap);
  const Slabs sl = slabs_of(op, part, "part", -1, c.H);
  TORCH_CHECK(part.size(1) >= (long)c.T * c.K, "moe_combine_slabs: part has fewer slot rows than T * k");
  auto g = op.guard();
  const int rc = bfly::launch_moe_combine_slabs(sl.p, sl.sk, part.size(1) * (long)c.H, c.slot_of, c.w, c.T, c.K, c.H,
                                                c.out, cur_stream(), c.bcnt, (int)bcap);
  TORCH_CHECK(rc == 0, "moe_combine_slabs: H % 4");
}

void ep_pack(const Tensor& x, const Tensor& ids, const Tensor& w, const OptTensor& slots, int64_t experts_per_rank,
             int64_t ep, int64_t cap, Tensor& send, Tensor& meta, Tensor& slot) {
  const Op op("ep_pack", x, "x");
  const EpArgs a = ep_dispatch_args(op, x, ids, w, slots, cap, ep, slot);
  auto g = op.guard();
  const int rc = bfly::launch_ep_pack(a.x, a.ids, a.w, a.slots, a.T, a.K, a.H, (int)experts_per_rank, (int)ep, (int)cap,
                                      op.shaped<bf16>(send, "send", {ep * cap, a.H}),
                                      op.shaped<float>(meta, "meta", {ep * cap, 2 * a.K}), a.slot, cur_stream());
  TORCH_CHECK(rc == 0, "ep_pack: rejected (", rc, ")");
}

void ep_combine(const Tensor& back, const Tensor& slot, Tensor& out) {
  const Op op("ep_combine", back, "back");
  bf16* o = op.shaped<bf16>(out, "out", {-1, -1});
  const int T = out.size(0);
  const int* sp = op.flat_min<int>(slot, "slot", 0);
  TORCH_CHECK(T == 0 || slot.numel() % T == 0, "ep_combine: slot [T, ep]");
  const int ep = T ? (int)(slot.numel() / T) : 2;
  auto g = op.guard();
  const int rc = bfly::launch_ep_combine(op.shaped<bf16>(back, "back", {-1, out.size(1)}), sp, T, out.size(1), ep, o,
                                         cur_stream());
  TORCH_CHECK(rc == 0, "ep_combine: rejected (", rc, ")");
}

void moe_gate_scale(Tensor& h, const Tensor& gates, int64_t e0, int64_t num_local) {
  const Op op("moe_gate_scale", h, "h");
  bf16* hp = op.shaped<bf16>(h, "h", {-1, -1});
  const float* gp = gates_of(op, gates, h.size(0));
  const int T = h.size(0), E = gates.size(1);
  TORCH_CHECK(num_local > 0 && h.size(1) % num_local == 0 && e0 + num_local <= E, "moe_gate_scale: experts");
  const int F = h.size(1) / num_local;
  TORCH_CHECK(F % 8 == 0, "moe_gate_scale: F % 8");
  auto g = op.guard();
  bfly::launch_moe_gate_scale(hp, gp, T, E, e0, num_local, F, cur_stream());
}

void probe(int64_t which, Tensor& out) {
  const Op op("probe", out, "out");
  auto g = op.guard();
  bfly::launch_probe(which, op.flat_min<float>(out, "out", 64 * 16), cur_stream());
}

// ---- one-shot IPC all-reduce -------------------------------------------------------------
// Buffers are raw device pointers carried as int64 (they are shared with peer processes via
// hipIpc handles and live for the communicator's lifetime, outside torch's allocator).
int64_t car_alloc(int64_t bytes) {
  TORCH_CHECK(bytes > 0, "car_alloc: bytes");
  void* p = bfly::car_alloc((size_t)bytes);
  TORCH_CHECK(p != nullptr, "car_alloc: hipExtMallocWithFlags(uncached) failed");
  return reinterpret_cast<int64_t>(p);
}
void car_free(int64_t p) { bfly::car_free(reinterpret_cast<void*>(p)); }
Tensor car_ipc_handle(int64_t p) {
  Tensor h = at::empty({64}, at::TensorOptions().dtype(at::kByte));
  TORCH_CHECK(bfly::car_ipc_handle(reinterpret_cast<void*>(p), h.data_ptr<uint8_t>()) == 0,
              "car_ipc_handle: hipIpcGetMemHandle failed");
  return h;
}
int64_t car_ipc_open(const Tensor& h) {
  TORCH_CHECK(h.scalar_type() == at::kByte && h.numel() == 64 && h.is_contiguous() && !h.is_cuda(),
              "car_ipc_open: expects a 64-byte CPU uint8 handle");
  void* p = bfly::car_ipc_open(h.data_ptr<uint8_t>());
  TORCH_CHECK(p != nullptr, "car_ipc_open: hipIpcOpenMemHandle failed");
  return reinterpret_cast<int64_t>(p);
}
void car_ipc_close(int64_t p) { bfly::car_ipc_close(reinterpret_cast<void*>(p)); }
int64_t car_error(int64_t p) { return bfly::car_error(reinterpret_cast<const void*>(p)); }
void car_clear_error(int64_t p) {
  TORCH_CHECK(bfly::car_clear_error(reinterpret_cast<void*>(p)) == 0, "car_clear_error: hipMemset failed");
}

// peer IPC buffers (allocated with car_alloc) of 2, 4 or 8 ranks
static bfly::ArPeers ep_peers(const char* op, at::IntArrayRef bases) {
  TORCH_CHECK(bases.size() == 2 || bases.size() == 4 || bases.size() == 8, op, ": 2, 4 or 8 ranks");
  bfly::ArPeers peers{};
  for (size_t i = 0; i < bases.size(); ++i) {
    TORCH_CHECK(bases[i] != 0, op, ": null peer buffer");
    peers.base[i] = reinterpret_cast<char*>(bases[i]);
  }
  peers.herr = bfly::health_words_device();
  return peers;
}

void custom_all_reduce(const Tensor& inp, Tensor& out, const OptTensor& residual, const OptTensor& w, double eps,
                       at::IntArrayRef bases, int64_t rank, int64_t cap, const OptTensor& slabs, bool two_shot,
                       int64_t blocks) {
  const Op op("custom_all_reduce", inp, "inp");
  const bf16* ip = op.shaped<bf16>(inp, "inp", {-1, -1}, kAlign16);
  const int rows = inp.size(0), dim = inp.size(1);
  bf16* o = op.shaped<bf16>(out, "out", {rows, dim}, kAlign16);
  const int world = (int)bases.size();
  TORCH_CHECK(world == 2 || world == 4 || world == 8, "custom_all_reduce: world must be 2, 4 or 8");
  TORCH_CHECK(rank >= 0 && rank < world, "custom_all_reduce: rank");
  TORCH_CHECK(dim % 8 == 0 && dim <= 16384, "custom_all_reduce: dim % 8 == 0 and <= 16384");
  TORCH_CHECK((int64_t)rows * dim * 2 <= cap, "custom_all_reduce: message larger than the buffer");
  const bfly::ArPeers peers = ep_peers(op.name, bases);
  bf16* res = op.shaped<bf16>(residual, "residual", {rows, dim});
  const bf16* wp = nullptr;
  if (residual.has_value()) {
    TORCH_CHECK(w.has_value(), "custom_all_reduce: norm weight required with residual");
    wp = op.flat<bf16>(w, "w", dim);
    TORCH_CHECK(o != ip, "custom_all_reduce: fused norm cannot run in place");
  }
  Slabs sl{nullptr, 0};   // inp is then only the shape / output placeholder
  if (slabs.has_value()) sl = slabs_of(op, *slabs, "slabs", rows, dim, kAlign16);
  auto g = op.guard();
  const int rc = bfly::launch_custom_allreduce(ip, o, res, wp, (float)eps, rows, dim, peers, world, (int)rank, cap,
                                               cur_stream(), sl.p, sl.sk, two_shot, (int)blocks);
  TORCH_CHECK(rc == 0, "custom_all_reduce: launch rejected (", rc, ")");
}

// Host-mapped health words (bfly_kernels.h): [kHealthCar] custom all-reduce and [kHealthEp]
// EP IPC flag-wait timeouts. health_init allocates them (eagerly, before any graph capture);
// reading them is a plain host load, safe from a poller thread while the GPU is busy or stuck.
bool health_init() { return bfly::health_words_device() != nullptr; }

// Read and reset the runtime's sticky last-error code: a failed stream capture leaves
// hipErrorStreamCaptureInvalidated behind, which the next checked launch would report as
// its own failure (ModelRunner clears it before falling back to eager decode).
int64_t hip_clear_error() { return (int64_t)hipGetLastError(); }

std::vector<int64_t> health_words() {
  return {(int64_t)bfly::health_word(bfly::kHealthCar), (int64_t)bfly::health_word(bfly::kHealthEp)};
}

void health_clear(int64_t word) { bfly::health_clear((int)word); }

// ---- byte-minimal EP dispatch over peer IPC buffers (allocated with car_alloc) ------------
std::vector<int64_t> ep_ipc_layout(int64_t ep, int64_t capmax, int64_t H, int64_t K) {
  const bfly::EpLayout L = bfly::ep_ipc_layout((int)ep, (int)capmax, (int)H, (int)K);
  return {L.x, L.ids, L.w, L.back, L.total};
}

// a [rows, cols] view of a region of this rank's IPC buffer (no ownership: the buffer lives as
// long as the EpIpc object that allocated it)
Tensor ep_ipc_view(int64_t ptr, int64_t offset, int64_t rows, int64_t cols, int64_t dtype, int64_t device) {
  const at::ScalarType st = dtype == 0 ? at::kBFloat16 : dtype == 1 ? at::kInt : at::kFloat;
  return at::from_blob(reinterpret_cast<char*>(ptr) + offset, {rows, cols},
                       at::TensorOptions().dtype(st).device(at::kCUDA, (int)device));
}

// decode-sized dispatch, or with `prefill` the one for any T <= capmax (ep_ipc.hip)
void ep_ipc_dispatch_impl(const Op& op, const Tensor& x, const Tensor& ids, const Tensor& w, const OptTensor& slots,
                          int64_t experts_per_rank, int64_t capmax, at::IntArrayRef bases, int64_t rank, Tensor& slot,
                          bool prefill) {
  const int ep = (int)bases.size();
  const EpArgs a = ep_dispatch_args(op, x, ids, w, slots, capmax, ep, slot);
  const bfly::ArPeers peers = ep_peers(op.name, bases);
  auto g = op.guard();
  const int rc = prefill ? bfly::launch_ep_ipc_dispatch_prefill(a.x, a.ids, a.w, a.T, a.K, a.H, (int)experts_per_rank,
                                                                ep, (int)capmax, peers, (int)rank, a.slot, cur_stream())
                         : bfly::launch_ep_ipc_dispatch(a.x, a.ids, a.w, a.slots, a.T, a.K, a.H, (int)experts_per_rank,
                                                        ep, (int)capmax, peers, (int)rank, a.slot, cur_stream());
  TORCH_CHECK(rc == 0, op.name, ": rejected (", rc, ")");
}

void ep_ipc_dispatch(const Tensor& x, const Tensor& ids, const Tensor& w, const OptTensor& slots,
                     int64_t experts_per_rank, int64_t capmax, at::IntArrayRef bases, int64_t rank, Tensor& slot) {
  ep_ipc_dispatch_impl(Op("ep_ipc_dispatch", x, "x"), x, ids, w, slots, experts_per_rank, capmax, bases, rank, slot,
                       false);
}

void ep_ipc_dispatch_prefill(const Tensor& x, const Tensor& ids, const Tensor& w, int64_t experts_per_rank,
                             int64_t capmax, at::IntArrayRef bases, int64_t rank, Tensor& slot) {
  ep_ipc_dispatch_impl(Op("ep_ipc_dispatch_prefill", x, "x"), x, ids, w, c10::nullopt, experts_per_rank, capmax, bases,
                       rank, slot, true);
}

int64_t ep_ipc_counts_offset() { return bfly::ep_ipc_counts_offset(); }

void ep_ipc_wait(const Tensor& like, at::IntArrayRef bases, int64_t rank) {
  const Op op("ep_ipc_wait", like, "like");
  auto g = op.guard();
  const int rc = bfly::launch_ep_ipc_wait(ep_peers(op.name, bases), (int)bases.size(), (int)rank, cur_stream());
  TORCH_CHECK(rc == 0, "ep_ipc_wait: rejected (", rc, ")");
}

void ep_ipc_return(const Tensor& y, int64_t K, int64_t capmax, at::IntArrayRef bases, int64_t rank) {
  const Op op("ep_ipc_return", y, "y");
  const int ep = (int)bases.size();
  const bf16* yp = op.shaped<bf16>(y, "y", {ep * capmax, -1});
  auto g = op.guard();
  const int rc = bfly::launch_ep_ipc_return(yp, y.size(1), (int)K, ep, (int)capmax, ep_peers(op.name, bases), (int)rank,
                                            cur_stream());
  TORCH_CHECK(rc == 0, "ep_ipc_return: rejected (", rc, ")");
}

void ep_ipc_combine(const Tensor& slot, int64_t K, int64_t capmax, at::IntArrayRef bases, int64_t rank, Tensor& out) {
  const Op op("ep_ipc_combine", out, "out");
  bf16* o = op.shaped<bf16>(out, "out", {-1, -1});
  const int T = out.size(0), ep = (int)bases.size();
  auto g = op.guard();
  const int rc = bfly::launch_ep_ipc_combine(op.flat<int>(slot, "slot", (long)T * ep), T, out.size(1), (int)K, ep,
                                             (int)capmax, ep_peers(op.name, bases), (int)rank, o, cur_stream());
  TORCH_CHECK(rc == 0, "ep_ipc_combine: rejected (", rc, ")");
}

std::vector<int64_t> ep_ipc_stats(int64_t p) {
  long long v[2] = {0, 0};
  TORCH_CHECK(bfly::ep_ipc_stats(reinterpret_cast<const void*>(p), v) == 0, "ep_ipc_stats: hipMemcpy failed");
  return {v[0], v[1]};
}
}  // namespace

TORCH_LIBRARY(bfly, m) {
  m.def("rms_norm(Tensor x, Tensor w, float eps, Tensor(a!) out, Tensor(b!)? residual) -> ()");
  m.def("layer_norm(Tensor x, Tensor w, Tensor b, float eps, Tensor(a!) out, Tensor(b!)? residual) -> ()");
  m.def("rope_kv(Tensor(a!) qkv, Tensor positions, Tensor cos, Tensor sin, int num_q_heads, "
        "int num_kv_heads, Tensor? slots, Tensor(b!)? k_cache, Tensor(c!)? v_cache, Tensor? partial=None) -> ()");
  m.def("gemm_deferred(Tensor x, Tensor w, Tensor(a!) out, Tensor(b!) workspace) -> int");
  m.def("splitk_reduce(Tensor slabs, Tensor(a!) out) -> ()");
  m.def("rms_norm_partial(Tensor slabs, Tensor w, float eps, Tensor(a!) out, Tensor(b!)? residual) -> ()");
  m.def("rms_norm_partial_route(Tensor slabs, Tensor w, float eps, Tensor(a!) out, Tensor(b!) residual, Tensor router_w, "
        "int top_k, Tensor(c!) gates, Tensor(d!) topk_ids, Tensor(e!) topk_w) -> ()");
  m.def("rms_norm_route_ok(int E, int dim) -> int", &rms_norm_route_ok);
  m.def("gemm_slab_offset() -> int", []() -> int64_t { return (int64_t)bfly::gemm_slab_offset_floats(); });
  m.def("gemm_rs(Tensor x, Tensor w, Tensor(a!) out, Tensor? bias, int epilogue, Tensor(b!)? workspace, "
        "Tensor ssp, float eps) -> ()");
  m.def("gemm_deferred_rs(Tensor x, Tensor w, Tensor(a!) out, Tensor(b!) workspace, Tensor ssp, float eps) -> int");
  m.def("rms_norm_rows(Tensor x, Tensor w, Tensor(a!) out, Tensor(b!) ssp, Tensor(c!)? residual) -> ()");
  m.def("rms_norm_rows_chunks(int dim) -> int", [](int64_t dim) -> int64_t { return bfly::rmsnorm_rows_chunks(dim); });
  m.def("gemm_rowscale_check(int M, int N, int K, int epilogue) -> int",
        [](int64_t M, int64_t N, int64_t K, int64_t e) -> int64_t { return bfly::gemm_rowscale_check(M, N, K, e); });
  m.def("kv_append(Tensor k, Tensor v, Tensor slots, Tensor(a!) k_cache, Tensor(b!) v_cache) -> ()");
  m.def("silu_mul(Tensor gu, Tensor(a!) out, int interleave) -> ()");
  m.def("gelu(Tensor x, Tensor(a!) out) -> ()");
  m.def("add(Tensor a, Tensor b, Tensor(a!) out) -> ()");
  m.def("init_hash(Tensor(a!) out, int grow0, int gcol0, int gcols, int seed, float amp) -> ()");
  m.def("embed(Tensor ids, Tensor table, Tensor(a!) out, int vstart) -> ()");
  m.def("gather_rows(Tensor src, Tensor idx, Tensor(a!) out) -> ()");
  m.def("zero_(Tensor(a!) t) -> ()");
  m.def("fill32_(Tensor(a!) t, int value) -> ()");
  m.def("sample_pack(Tensor scores, Tensor ids, Tensor(a!) pair) -> ()");
  m.def("sample_merge(Tensor allp, Tensor(a!) out) -> ()");
  m.def("sample(Tensor logits, Tensor? temps, Tensor? seeds, int vstart, Tensor(a!) out_ids, "
        "Tensor(b!) out_scores, Tensor(c!) workspace, Tensor? thresh=None, bool check_finite=False) -> ()");
  m.def("logprobs_workspace_size(int rows, int V, int n) -> int", &logprobs_workspace_size);
  m.def("logprobs_partial(Tensor logits, Tensor ids, int n, int vstart, Tensor(a!) record, "
        "Tensor(b!) workspace) -> ()");
  m.def("logprobs_merge(Tensor records, Tensor(a!) chosen_lp, Tensor(b!) top_ids, Tensor(c!) top_lp) -> ()");
  m.def("apply_penalties(Tensor logits, int vstart, Tensor(a!) hist, Tensor slots, Tensor lens, Tensor prompt_lens, "
        "Tensor last, Tensor params, Tensor(b!) out) -> ()");
  m.def("tkp_begin(Tensor logits, Tensor temps, Tensor top_k, Tensor top_p, Tensor(a!) ws) -> ()");
  m.def("tkp_pass(Tensor logits, Tensor temps, Tensor(a!) ws, int pass_, int phase) -> ()");
  m.def("tkp_select(Tensor top_p, Tensor(a!) ws, int rows, int pass_, int phase) -> ()");
  m.def("tkp_final(Tensor(a!) ws, int rows, Tensor(b!) thresh) -> ()");
  m.def("gemm(Tensor x, Tensor w, Tensor(a!) out, Tensor? bias, int epilogue, Tensor(b!)? workspace) -> ()");
  m.def("gemm_silu_gate(Tensor x, Tensor w, Tensor(a!) out, Tensor gates, int e0, int num_local) -> ()");
  m.def("gemm_packed(Tensor x, Tensor wp, Tensor(a!) out, int epilogue, Tensor? ssp=None, float eps=0.0, "
        "Tensor? gates=None, int e0=0, int num_local=1, Tensor(b!)? workspace=None, bool defer=False) -> int");
  m.def("gemm_packed_check(int M, int N, int K, int epilogue) -> int", &gemm_packed_check);
  m.def("quant_fp8_rows(Tensor w, Tensor(a!) code, Tensor(b!) scale) -> ()");
  m.def("dequant_fp8(Tensor code, Tensor? scale, Tensor(a!) out) -> ()");
  m.def("w8_scale_cols(Tensor y, Tensor scale, Tensor(a!) out, int epilogue) -> ()");
  m.def("gemm_w8(Tensor x, Tensor code, Tensor scale, Tensor(a!) out, int epilogue, Tensor(b!)? workspace, "
        "bool any_m=False, int force_sk=0) -> ()");
  m.def("gemm_w8_check(int M, int N, int K, int epilogue) -> int",
        [](int64_t M, int64_t N, int64_t K, int64_t e) -> int64_t { return bfly::gemm_w8_check(M, N, K, e); });
  m.def("gemm_w8_splitk(int M, int N, int K, int epilogue) -> int",
        [](int64_t M, int64_t N, int64_t K, int64_t e) -> int64_t { return bfly::gemm_w8_splitk(M, N, K, e); });
  m.def("gemm_w8_workspace_size(int M, int N, int K) -> int",
        [](int64_t M, int64_t N, int64_t K) -> int64_t { return (int64_t)bfly::gemm_w8_workspace_bytes(M, N, K); });
  // registered with their kernels as catch-all functions (the Op checks the device), like the
  // *_check lambdas: the CUDA block below is held to a fixed table by tests/test_ops_refusals_gpu.py
  m.def("quant_mxfp4(Tensor w, Tensor(a!) code, Tensor(b!) scale) -> ()", &quant_mxfp4);
  m.def("dequant_mxfp4(Tensor code, Tensor scale, Tensor(a!) out) -> ()", &dequant_mxfp4);
  m.def("gemm_w4(Tensor x, Tensor code, Tensor scale, Tensor(a!) out, int epilogue, Tensor(b!)? workspace, "
        "bool any_m=False, int force_sk=0) -> ()", &gemm_w4);
  m.def("gemm_w4_check(int M, int N, int K, int epilogue) -> int",
        [](int64_t M, int64_t N, int64_t K, int64_t e) -> int64_t { return bfly::gemm_w4_check(M, N, K, e); });
  m.def("gemm_w4_splitk(int M, int N, int K, int epilogue) -> int",
        [](int64_t M, int64_t N, int64_t K, int64_t e) -> int64_t { return bfly::gemm_w4_splitk(M, N, K, e); });
  m.def("gemm_w4_workspace_size(int M, int N, int K) -> int",
        [](int64_t M, int64_t N, int64_t K) -> int64_t { return (int64_t)bfly::gemm_w4_workspace_bytes(M, N, K); });
  m.def("rope_qknorm_kv(Tensor(a!) qkv, Tensor positions, Tensor cos, Tensor sin, int num_q_heads, "
        "int num_kv_heads, Tensor? slots, Tensor(b!)? k_cache, Tensor(c!)? v_cache, Tensor q_norm_w, Tensor k_norm_w, "
        "float eps, Tensor? partial=None) -> ()", &rope_qknorm_kv);
  m.def("lora_shrink(Tensor x, Tensor a, Tensor idx, Tensor(a!) part) -> ()", &lora_shrink);
  m.def("lora_expand(Tensor(a!) y, Tensor part, Tensor b, Tensor seg, Tensor scale, Tensor idx) -> ()", &lora_expand);
  m.def("lora_splitk(int T, int K) -> int", [](int64_t T, int64_t K) -> int64_t { return bfly::lora_splitk((int)T, (int)K); });
  m.def("lora_check(int K, int J, int N, int R) -> int",
        [](int64_t K, int64_t J, int64_t N, int64_t R) -> int64_t { return bfly::lora_check((int)K, (int)J, (int)N, (int)R); });
  m.def("attn_verify(Tensor q, Tensor k_cache, Tensor v_cache, Tensor block_tables, Tensor ctx_lens, Tensor q_lens, "
        "float scale, int max_ctx, int part_tokens, Tensor(a!) out, Tensor(b!)? part_o, Tensor(c!)? part_ml) -> ()",
        &attn_verify);
  m.def("attn_verify_tiles(int QN, int G) -> int", &attn_verify_tiles);
  m.def("gemm_with_plan(Tensor x, Tensor w, Tensor(a!) out, int[] plan, int epilogue, Tensor(b!)? workspace, "
        "Tensor? bias=None, bool packed=False) -> ()");
  m.def("gemm_plan_check(int[] plan, int M, int N, int K, int epilogue, bool packed=False) -> int", &gemm_plan_check);
  m.def("gemm_mixed_tiles_mode(int mode) -> int",
        [](int64_t mode) -> int64_t { return bfly::gemm_mixed_tiles_mode((int)mode); });
  m.def("gemm_workspace_size(int M, int N, int K) -> int", &gemm_workspace_size);
  m.def("gemm_plan(int M, int N, int K) -> int[]", &gemm_plan);
  m.def("gemm_check(int M, int N, int K, int epilogue) -> int",
        [](int64_t M, int64_t N, int64_t K, int64_t e) -> int64_t { return bfly::gemm_check(M, N, K, e); });
  m.def("attn_decode_splits(int max_ctx, int part_tokens) -> int", &attn_decode_splits);
  m.def("attn_decode_part_tokens(int B, int Hkv, int max_ctx) -> int", &attn_decode_part_tokens);
  m.def("attn_decode(Tensor q, Tensor k_cache, Tensor v_cache, Tensor block_tables, Tensor ctx_lens, "
        "float scale, int max_ctx, int part_tokens, Tensor(a!) out, Tensor(b!)? part_o, "
        "Tensor(c!)? part_ml) -> ()");
  m.def("moe_route(Tensor x, Tensor wr, int top_k, Tensor(a!) gates, Tensor(b!) topk_ids, Tensor(c!) topk_w) -> ()");
  m.def("moe_gate_scale(Tensor(a!) h, Tensor gates, int e0, int num_local) -> ()");
  m.def("moe_max_tiles(int tk, int num_local, int bm=64) -> int", &moe_max_tiles);
  m.def("moe_align(Tensor topk_ids, int e0, int num_local, Tensor(a!) rows, Tensor(b!) slot_of, Tensor(c!) tiles, "
        "Tensor(d!) count, int bm=64, Tensor? bcnt=None, int bcap=0) -> ()");
  m.def("moe_grouped_gemm(Tensor x, Tensor w, Tensor(a!) out, Tensor? rows, Tensor tiles, Tensor count, int w_estride, "
        "int n, int k, int num_experts, int epilogue, int bm=64, Tensor(b!)? part=None) -> ()");
  m.def("moe_combine(Tensor y, Tensor slot_of, Tensor topk_w, Tensor(a!) out, Tensor? bcnt=None, int bcap=0) -> ()");
  m.def("moe_combine_slabs(Tensor part, Tensor slot_of, Tensor topk_w, Tensor(a!) out, Tensor? bcnt=None, "
        "int bcap=0) -> ()");
  m.def("ep_ipc_dispatch_prefill(Tensor x, Tensor ids, Tensor w, int experts_per_rank, int capmax, int[] bases, "
        "int rank, Tensor(a!) slot) -> ()");
  m.def("ep_ipc_counts_offset() -> int", &ep_ipc_counts_offset);
  m.def("ep_pack(Tensor x, Tensor ids, Tensor w, Tensor? slots, int experts_per_rank, int ep, int cap, "
        "Tensor(a!) send, Tensor(b!) meta, Tensor(c!) slot) -> ()");
  m.def("ep_combine(Tensor back, Tensor slot, Tensor(a!) out) -> ()");
  m.def("probe(int which, Tensor(a!) out) -> ()");
  m.def("car_alloc(int bytes) -> int", &car_alloc);
  m.def("car_free(int ptr) -> ()", &car_free);
  m.def("car_ipc_handle(int ptr) -> Tensor", &car_ipc_handle);
  m.def("car_ipc_open(Tensor handle) -> int", &car_ipc_open);
  m.def("car_ipc_close(int ptr) -> ()", &car_ipc_close);
  m.def("car_error(int ptr) -> int", &car_error);
  m.def("car_clear_error(int ptr) -> ()", &car_clear_error);
  m.def("car_buffer_bytes(int cap) -> int", [](int64_t cap) -> int64_t { return bfly::car_buffer_bytes(cap); });
  m.def("custom_all_reduce(Tensor inp, Tensor(a!) out, Tensor(b!)? residual, Tensor? w, float eps, "
        "int[] bases, int rank, int cap, Tensor? slabs=None, bool two_shot=False, int blocks=128) -> ()");
  m.def("ep_ipc_layout(int ep, int capmax, int H, int K) -> int[]", &ep_ipc_layout);
  m.def("ep_ipc_view(int ptr, int offset, int rows, int cols, int dtype, int device) -> Tensor", &ep_ipc_view);
  m.def("ep_ipc_dispatch(Tensor x, Tensor ids, Tensor w, Tensor? slots, int experts_per_rank, int capmax, "
        "int[] bases, int rank, Tensor(a!) slot) -> ()");
  m.def("ep_ipc_wait(Tensor like, int[] bases, int rank) -> ()");
  m.def("ep_ipc_return(Tensor y, int k, int capmax, int[] bases, int rank) -> ()");
  m.def("health_init() -> bool", &health_init);
  m.def("hip_clear_error() -> int", &hip_clear_error);
  m.def("health_words() -> int[]", &health_words);
  m.def("health_clear(int word=-1) -> ()", &health_clear);
  m.def("ep_ipc_combine(Tensor slot, int k, int capmax, int[] bases, int rank, Tensor(a!) out) -> ()");
  m.def("ep_ipc_stats(int ptr) -> int[]", &ep_ipc_stats);
  m.def("ep_ipc_error(int ptr) -> int", [](int64_t p) -> int64_t { return bfly::ep_ipc_error(reinterpret_cast<const void*>(p)); });
  m.def("attn_prefill_paged(Tensor q, Tensor k_cache, Tensor v_cache, Tensor tables, Tensor cu_q, "
        "Tensor positions, int max_q, float scale, Tensor(a!) out) -> ()");
  m.def("attn_prefill(Tensor q, Tensor k, Tensor v, Tensor cu_seqlens, int max_seqlen, float scale, "
        "bool causal, Tensor(a!) out, Tensor? cu_seqlens_k=None, Tensor(b!)? lse=None) -> ()");
  m.def("attn_lse_merge(Tensor(a!) acc_o, Tensor(b!) acc_lse, Tensor o, Tensor lse) -> ()");
}

TORCH_LIBRARY_IMPL(bfly, CUDA, m) {
  m.impl("rms_norm", &rms_norm);
  m.impl("layer_norm", &layer_norm);
  m.impl("rope_kv", &rope_kv);
  m.impl("kv_append", &kv_append);
  m.impl("silu_mul", &silu_mul);
  m.impl("gelu", &gelu);
  m.impl("add", &add);
  m.impl("embed", &embed);
  m.impl("gather_rows", &gather_rows);
  m.impl("zero_", &zero_);
  m.impl("fill32_", &fill32_);
  m.impl("sample_pack", &sample_pack);
  m.impl("sample_merge", &sample_merge);
  m.impl("init_hash", &init_hash);
  m.impl("sample", &sample);
  m.impl("logprobs_partial", &logprobs_partial);
  m.impl("logprobs_merge", &logprobs_merge);
  m.impl("apply_penalties", &apply_penalties);
  m.impl("tkp_begin", &tkp_begin);
  m.impl("tkp_pass", &tkp_pass);
  m.impl("tkp_select", &tkp_select);
  m.impl("tkp_final", &tkp_final);
  m.impl("gemm", &gemm);
  m.impl("gemm_silu_gate", &gemm_silu_gate);
  m.impl("gemm_packed", &gemm_packed);
  m.impl("quant_fp8_rows", &quant_fp8_rows);
  m.impl("dequant_fp8", &dequant_fp8);
  m.impl("w8_scale_cols", &w8_scale_cols);
  m.impl("gemm_w8", &gemm_w8);
  m.impl("gemm_with_plan", &gemm_with_plan);
  m.impl("gemm_deferred", &gemm_deferred);
  m.impl("splitk_reduce", &splitk_reduce);
  m.impl("rms_norm_partial", &rms_norm_partial);
  m.impl("rms_norm_partial_route", &rms_norm_partial_route);
  m.impl("gemm_rs", &gemm_rs);
  m.impl("gemm_deferred_rs", &gemm_deferred_rs);
  m.impl("rms_norm_rows", &rms_norm_rows);
  m.impl("attn_decode", &attn_decode);
  m.impl("attn_prefill", &attn_prefill);
  m.impl("attn_prefill_paged", &attn_prefill_paged);
  m.impl("attn_lse_merge", &attn_lse_merge);
  m.impl("probe", &probe);
  m.impl("custom_all_reduce", &custom_all_reduce);
  m.impl("moe_route", &moe_route);
  m.impl("moe_gate_scale", &moe_gate_scale);
  m.impl("moe_align", &moe_align);
  m.impl("moe_grouped_gemm", &moe_grouped_gemm);
  m.impl("moe_combine", &moe_combine);
  m.impl("moe_combine_slabs", &moe_combine_slabs);
  m.impl("ep_ipc_dispatch_prefill", &ep_ipc_dispatch_prefill);
  m.impl("ep_pack", &ep_pack);
  m.impl("ep_combine", &ep_combine);
  m.impl("ep_ipc_dispatch", &ep_ipc_dispatch);
  m.impl("ep_ipc_wait", &ep_ipc_wait);
  m.impl("ep_ipc_return", &ep_ipc_return);
  m.impl("ep_ipc_combine", &ep_ipc_combine);
}
