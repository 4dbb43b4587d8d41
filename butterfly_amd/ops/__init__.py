"""butterfly_amd ops: hand-written HIP/CDNA4 kernels bound as torch.ops.bfly.*.

GPU tensors always run the HIP kernels from the in-tree `butterfly_amd/_C.so`; if that
library is missing or fails to load, every GPU call raises (no silent eager fallback).
CPU tensors run `ops.reference` (the CPU/gloo plumbing path and the numerics oracle).

Workspaces (split-K GEMM partials, split-KV decode partials, sampling partials) come from a
per-device arena that the engine sizes before hipGraph capture (`reserve_workspace`), so
captured steps never allocate.
"""
from __future__ import annotations

import os
import threading
from typing import Optional
from pathlib import Path

import torch

from . import reference as ref
from .reference import SILU_INTERLEAVE, interleave_gate_up, rope_tables, split_gate_up  # noqa: F401

_LIB_PATH = Path(__file__).resolve().parent.parent / "_C.so"
_loaded = False
_load_error: str | None = None

EPILOGUES = {"none": 0, "bias": 1, "silu": 2}
DECODE_PART_TOKENS = 0   # 0 = pick the context split per call (attn_decode_part_tokens)


def load_library(path: str | os.PathLike | None = None) -> bool:
    """Load the HIP kernel library (idempotent). Returns True on success."""
    global _loaded, _load_error
    if _loaded:
        return True
    # BFLY_KERNEL_LIB: another build of the kernel library (same-box A/B runs of kernel changes)
    p = Path(path) if path else Path(os.environ.get("BFLY_KERNEL_LIB") or _LIB_PATH)
    if not p.exists():
        _load_error = f"{p} not built (run `python -m butterfly_amd._build`)"
        return False
    try:
        torch.ops.load_library(str(p))
        _loaded = True
        _load_error = None
    except Exception as e:  # pragma: no cover - depends on the environment
        _load_error = f"failed to load {p}: {e}"
    return _loaded


def require_library() -> None:
    """Raise unless the HIP kernel library is loaded (GPU-only features call this)."""
    if not load_library():
        raise RuntimeError(f"butterfly_amd HIP kernels unavailable: {_load_error}")


def native_available() -> bool:
    return load_library()


def library_path() -> str:
    return str(_LIB_PATH)


_FORCE_REF = False


class reference_mode:
    """Route every op to its fp32 PyTorch reference (ops/reference.py) even for GPU tensors:
    tests build an fp32 reference model on the same GPU as the kernel model (full-size layers
    whose CPU reference would take minutes). Not thread-scoped; tests only."""

    def __enter__(self):
        global _FORCE_REF
        self._prev, _FORCE_REF = _FORCE_REF, True
        return self

    def __exit__(self, *exc):
        global _FORCE_REF
        _FORCE_REF = self._prev
        return False


def _gpu(t: torch.Tensor) -> bool:
    if not t.is_cuda or _FORCE_REF:
        return False
    if not load_library():
        raise RuntimeError(f"butterfly_amd HIP kernels unavailable: {_load_error}")
    return True


# ---------------------------------------------------------------------------------------
# Workspace arena
# ---------------------------------------------------------------------------------------
class _Arena:
    """Named scratch buffers reused by every kernel call (split-K slabs, decode-attention
    partials, MoE slot maps and tile lists, sampling pairs). Buffers are shared by the threads
    of a process (an engine built on one thread and stepped on another reuses them) unless a
    thread sets its own scope (`arena_scope`): several ranks driven from threads of ONE process
    (the loopback backend, parallel/fake.py) must never share e.g. a MoE tile list, or one
    rank's moe_align would steer the other's grouped GEMM outside its own activations."""

    def __init__(self):
        self.bufs: dict[tuple, torch.Tensor] = {}
        self.frozen = False
        # buffers replaced by a larger one stay allocated: a hipGraph captured earlier still
        # reads / writes the old address (freeing it would hand that memory to someone else)
        self.retired: list = []

    def get(self, device, name: str, numel: int, dtype, zero: bool = False) -> torch.Tensor:
        key = (str(device), name, dtype, getattr(_scope, "name", None))
        buf = self.bufs.get(key)
        if buf is None or buf.numel() < numel:
            if self.frozen or (torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()):
                raise RuntimeError(
                    f"workspace '{name}' needs {numel} elements but is frozen/capturing; "
                    "call ops.reserve_workspace() before capture")
            if buf is not None:
                self.retired.append(buf)
            buf = torch.empty(max(numel, 1), dtype=dtype, device=device)
            if zero:
                zero_(buf)
            self.bufs[key] = buf
        return buf


def zero_(t: torch.Tensor) -> torch.Tensor:
    """t.zero_() through the runtime's memset on the GPU (keeps torch kernels out of traces)."""
    if t.is_cuda and load_library():
        torch.ops.bfly.zero_(t)
    else:
        t.zero_()
    return t


# Output poisoning (`set_poison`): every op output is allocated filled with NaN
# (floating point) or a negative sentinel (integers) instead of left uninitialised, so an
# element a kernel forgot to write shows up in the comparison against the unpoisoned run.
_POISON = os.environ.get("BFLY_POISON_OUTPUTS", "0").strip().lower() in ("1", "true", "yes", "on")
# MoE prefill expert GEMMs on the 256x256 8-phase tile (BFLY_MOE_BIG_TILE=0: the 64/128-row tile)
_BIG_MOE = os.environ.get("BFLY_MOE_BIG_TILE", "1").strip().lower() not in ("0", "false", "no", "off")
# Host-side index checks of ops whose kernels cannot raise (BFLY_DEBUG_CHECKS; each costs a sync)
_DEBUG_CHECKS = os.environ.get("BFLY_DEBUG_CHECKS", "0").strip().lower() in ("1", "true", "yes", "on")


def set_poison(on: bool) -> None:
    """Allocate op outputs poisoned (debug / tests; costs one fill per output)."""
    global _POISON
    _POISON = bool(on)


def _poisoned(t: torch.Tensor) -> torch.Tensor:
    if t.dtype == torch.uint8:      # MXFP4 codes / scales: the sentinel must fit a byte
        return t.fill_(0xA5)
    return t.fill_(float("nan") if t.is_floating_point() else -7777777)


def _empty(*shape, **kw) -> torch.Tensor:
    t = torch.empty(*shape, **kw)
    return _poisoned(t) if _POISON else t


def _empty_like(x: torch.Tensor, **kw) -> torch.Tensor:
    t = torch.empty_like(x, **kw)
    return _poisoned(t) if _POISON else t


_scope = threading.local()
_arena = _Arena()


def arena_scope(name) -> None:
    """Give this host thread its own workspace buffers (None: the process-wide set)."""
    _scope.name = name


def reserve_w8_workspace(device, max_tokens: int, w8_shapes, weight_dtype: str = "fp8") -> None:
    """The weight-only GEMM's buffers for quantised projections of logical shapes `w8_shapes`
    (N, K) at up to `max_tokens` rows: the native kernel's split-K slabs and, when some row
    count or shape takes the dequantise route, a bf16 scratch of the largest projection and
    (FP8 only) of the largest unscaled GEMM result (SwiGLU projections). `weight_dtype`: "fp8"
    or "mxfp4"; the MXFP4 scratch holds the final weights, so it needs no second buffer."""
    if not load_library():
        return
    L = torch.ops.bfly
    check, size, slot = ((L.gemm_w4_check, L.gemm_w4_workspace_size, "gemm_w4") if weight_dtype == "mxfp4"
                         else (L.gemm_w8_check, L.gemm_w8_workspace_size, "gemm_w8"))
    w8 = {(int(n), int(k)) for n, k in w8_shapes}
    if w8:
        slab, deq, tmp = 0, 0, 0
        for m in sorted(set(range(1, 257)) | {max_tokens}):
            if m > max_tokens:
                continue
            for n, k in w8:
                if any(check(m, n, k, e) != 0 for e in (0, 2)):
                    deq = max(deq, n * k)
                    tmp = max(tmp, m * n)
                else:
                    slab = max(slab, size(m, n, k))
        if slab:
            _arena.get(device, slot, slab // 4 + 1, torch.float32)
        if deq:
            _arena.get(device, "w8_deq", deq, torch.bfloat16)
            if weight_dtype != "mxfp4":
                _arena.get(device, "w8_tmp", tmp, torch.bfloat16)


def reserve_workspace(device, max_tokens: int, max_n: int, max_k: int, max_batch: int = 0,
                      max_ctx: int = 0, num_kv_heads: int = 0, head_dim: int = 128, shapes=(),
                      w8_shapes=(), vocab: int = 0, weight_dtype: str = "fp8") -> None:
    """Pre-size every workspace for problems up to the given bounds (call before capture).
    `shapes`: the model's GEMM weight shapes (N, K); the split-K slab need is the max over them
    and every token-count bucket of the plan table (a tuned plan may split a small projection
    more than the largest one is split). `w8_shapes`: the logical (N, K) of the projections
    quantised to `weight_dtype` ("fp8" | "mxfp4"): sizes the native weight-only GEMM's split-K
    slabs and, for token counts (or shapes) that take the dequantise route, the bf16 scratch of
    the largest of them. `vocab`: columns of the logits
    shard; sizes the logprobs partials for `max_batch` rows with the most alternatives."""
    if not load_library():
        return
    reserve_w8_workspace(device, max_tokens, w8_shapes, weight_dtype)
    ws = 0
    nk = {(int(max_n), int(max_k))} | {(int(n), int(k)) for n, k in shapes}
    for m in sorted({1, 16, 32, 48, 64, 128, 256, 512, max_tokens}):
        if m > max_tokens:
            continue
        for n, k in nk:
            ws = max(ws, torch.ops.bfly.gemm_workspace_size(m, n, k))
    _arena.get(device, "gemm", ws // 4 + 1, torch.float32, zero=True)
    if max_batch and max_ctx:
        ns = max(torch.ops.bfly.attn_decode_splits(max_ctx, torch.ops.bfly.attn_decode_part_tokens(b, num_kv_heads, max_ctx))
                 for b in range(1, max_batch + 1))
        _arena.get(device, "attn_o", max_batch * num_kv_heads * ns * 16 * head_dim, torch.float32)
        _arena.get(device, "attn_ml", max_batch * num_kv_heads * ns * 16 * 2, torch.float32)
    _arena.get(device, "sample", max(max_batch, max_tokens, 1) * 64, torch.int64)
    _arena.get(device, "tkp", max(max_batch, max_tokens, 1) * 521, torch.float32)
    if vocab:
        _arena.get(device, "logprobs", torch.ops.bfly.logprobs_workspace_size(max(max_batch, 1), vocab, LOGPROBS_MAX_N),
                   torch.int64)


# ---------------------------------------------------------------------------------------
# Ops
# ---------------------------------------------------------------------------------------
class Partial:
    """Output of a split-K GEMM whose reduce was deferred to its consumer (`linear(...,
    defer=True)`): `slabs` [sk, M, N] f32 live in the shared GEMM workspace and must be consumed
    (rms_norm / rope_kv fuse the reduce) or `materialize()`d before the next GEMM runs.
    `out` is the bf16 [M, N] buffer the result belongs in."""

    __slots__ = ("slabs", "out")

    def __init__(self, slabs: torch.Tensor, out: torch.Tensor):
        self.slabs, self.out = slabs, out

    @property
    def shape(self):
        return self.out.shape

    def materialize(self) -> torch.Tensor:
        torch.ops.bfly.splitk_reduce(self.slabs, self.out)
        return self.out


def materialize(x):
    return x.materialize() if isinstance(x, Partial) else x


class RowNormed:
    """RMSNorm output whose 1/rms row scale is left to the consuming GEMM (`rms_norm(...,
    rows=True)`, norm.hip rmsnorm_rows_kernel): `y` [M, dim] bf16 = x * w, `ssp` [M, chunks] f32
    partial sums of squares of x. `linear(RowNormed, ...)` scales row m of its result by
    rsqrt(sum(ssp[m]) / dim + eps) in the GEMM epilogue (before bias / SiLU / split-K slabs)."""

    __slots__ = ("y", "ssp", "eps")

    def __init__(self, y: torch.Tensor, ssp: torch.Tensor, eps: float):
        self.y, self.ssp, self.eps = y, ssp, eps

    @property
    def shape(self):
        return self.y.shape


_rowscale_ok: dict = {}


def rowscale_ok(M: int, N: int, K: int, epilogue: str = "none") -> bool:
    """True if the GEMM plan for this shape applies a RowScale (tile / decode-ring kernels)."""
    key = (M, N, K, epilogue)
    ok = _rowscale_ok.get(key)
    if ok is None:
        ok = load_library() and torch.ops.bfly.gemm_rowscale_check(M, N, K, EPILOGUES[epilogue]) == 0
        _rowscale_ok[key] = ok
    return ok


def rms_norm(x, w, eps: float, out=None, residual=None, rows: bool = False):
    """y = x * rsqrt(mean(x^2) + eps) * w; with `residual`: residual += x first (in place)
    and y is the norm of the updated residual (the fused add+norm of every block). `x` may be
    a deferred split-K GEMM output (`Partial`): its reduce is fused into this kernel.
    `rows=True` (GPU): return a `RowNormed` for a row-scaling consumer GEMM instead."""
    if rows and (isinstance(x, Partial) or _gpu(x)):
        src = x.slabs if isinstance(x, Partial) else x
        M, dim = src.shape[-2], src.shape[-1]
        if out is None:
            out = _empty(M, dim, dtype=w.dtype, device=w.device)
        ssp = _empty(M, torch.ops.bfly.rms_norm_rows_chunks(dim), dtype=torch.float32, device=w.device)
        torch.ops.bfly.rms_norm_rows(src, w, out, ssp, residual)
        return RowNormed(out, ssp, eps)
    if isinstance(x, Partial):
        if out is None:
            out = _empty_like(x.out)
        torch.ops.bfly.rms_norm_partial(x.slabs, w, eps, out, residual)
        return out
    if not _gpu(x):
        return ref.rms_norm(x, w, eps, out, residual)
    if out is None:
        out = _empty_like(x)
    torch.ops.bfly.rms_norm(x, w, eps, out, residual)
    return out


def rms_norm_route(x, w, eps: float, residual, router_w, top_k: int):
    """The fused add + RMSNorm of a MoE layer's FFN input that also routes the rows it
    normalises (norm.hip rmsnorm_partial_kernel<NV, E>): returns (y, (gates, topk_ids, topk_w))
    as `rms_norm` then `moe_route(y, router_w, top_k)` would, in one launch. Needs a deferred
    split-K input (`Partial`), a residual and 4 or 8 experts; otherwise returns (rms_norm(...),
    None) and the caller routes separately."""
    if (isinstance(x, Partial) and residual is not None
            and torch.ops.bfly.rms_norm_route_ok(router_w.shape[0], router_w.shape[1]) == 1):
        T = x.out.shape[0]
        E = router_w.shape[0]
        out = _empty_like(x.out)
        gates = _empty(T, E, dtype=torch.float32, device=out.device)
        ids = _empty(T, top_k, dtype=torch.int32, device=out.device)
        tw = _empty(T, top_k, dtype=torch.float32, device=out.device)
        torch.ops.bfly.rms_norm_partial_route(x.slabs, w, eps, out, residual, router_w, top_k, gates, ids, tw)
        return out, (gates, ids, tw)
    return rms_norm(x, w, eps, residual=residual), None


def layer_norm(x, w, b, eps: float, out=None, residual=None):
    if not _gpu(x):
        return ref.layer_norm(x, w, b, eps, out, residual)
    if out is None:
        out = _empty_like(x)
    torch.ops.bfly.layer_norm(x, w, b, eps, out, residual)
    return out


def rope_kv(qkv, positions, cos, sin, n_q: int, n_kv: int, slots=None, k_cache=None,
            v_cache=None, q_norm=None, k_norm=None, eps: float = 0.0):
    """In-place RoPE on the Q/K heads of a fused QKV row; optional paged KV append. Returns the
    (bf16) QKV rows; `qkv` may be a deferred split-K GEMM output whose reduce is fused here.
    With `q_norm` / `k_norm` ([head_dim] weights, Qwen3) every Q / K head is RMS-normalised and
    scaled in front of the rotation, in the same kernel (rope.hip, QKNORM)."""
    if (q_norm is None) != (k_norm is None):
        raise ValueError("rope_kv: q_norm and k_norm go together")
    if q_norm is not None:
        if isinstance(qkv, Partial):
            torch.ops.bfly.rope_qknorm_kv(qkv.out, positions, cos, sin, n_q, n_kv, slots, k_cache, v_cache,
                                          q_norm, k_norm, eps, qkv.slabs)
            return qkv.out
        if not _gpu(qkv):
            return ref.rope_kv(qkv, positions, cos, sin, n_q, n_kv, slots, k_cache, v_cache, q_norm, k_norm, eps)
        torch.ops.bfly.rope_qknorm_kv(qkv, positions, cos, sin, n_q, n_kv, slots, k_cache, v_cache,
                                      q_norm, k_norm, eps)
        return qkv
    if isinstance(qkv, Partial):
        torch.ops.bfly.rope_kv(qkv.out, positions, cos, sin, n_q, n_kv, slots, k_cache, v_cache, qkv.slabs)
        return qkv.out
    if not _gpu(qkv):
        return ref.rope_kv(qkv, positions, cos, sin, n_q, n_kv, slots, k_cache, v_cache)
    torch.ops.bfly.rope_kv(qkv, positions, cos, sin, n_q, n_kv, slots, k_cache, v_cache)
    return qkv


def kv_append(k, v, slots, k_cache, v_cache):
    if not _gpu(k):
        return ref.kv_append(k, v, slots, k_cache, v_cache)
    torch.ops.bfly.kv_append(k, v, slots, k_cache, v_cache)


def silu_mul(gu, out=None, interleave: int = 0):
    if not _gpu(gu):
        return ref.silu_mul(gu, out, interleave)
    if out is None:
        out = _empty(*gu.shape[:-1], gu.shape[-1] // 2, dtype=gu.dtype, device=gu.device)
    torch.ops.bfly.silu_mul(gu, out, interleave)
    return out


def gelu(x, out=None):
    if not _gpu(x):
        return ref.gelu(x, out)
    if out is None:
        out = _empty_like(x)
    torch.ops.bfly.gelu(x, out)
    return out


def add(a, b, out=None):
    b = materialize(b)
    if not _gpu(a):
        return ref.add(a, b, out)
    if out is None:
        out = _empty_like(a)
    torch.ops.bfly.add(a, b, out)
    return out


def embed(ids, table, vstart: int = 0, out=None):
    if not _gpu(ids):
        return ref.embed(ids, table, vstart, out)
    if out is None:
        out = _empty(ids.numel(), table.shape[1], dtype=table.dtype, device=table.device)
    torch.ops.bfly.embed(ids, table, out, vstart)
    return out


def gather_rows(src, idx, out=None):
    """out[i] = src[idx[i]] (rows of a 2-D tensor; `idx` int32 / int64). Rows whose idx is < 0
    keep what `out` holds (pass a pre-filled `out`). Our row-gather kernel on the GPU, not
    torch's index_select (elementwise.hip gather_rows_kernel)."""
    if out is None:
        out = _empty(idx.numel(), *src.shape[1:], dtype=src.dtype, device=src.device)
    if not _gpu(src):
        return ref.gather_rows(src, idx, out)
    s2 = src if src.dim() == 2 else src.view(src.shape[0], -1)
    o2 = out if out.dim() == 2 else out.view(out.shape[0], -1)
    if _DEBUG_CHECKS and not torch.cuda.is_current_stream_capturing() and idx.numel():
        hi = int(idx.max())
        if hi >= src.shape[0]:
            raise IndexError(f"gather_rows: index {hi} out of range for {src.shape[0]} source rows")
    torch.ops.bfly.gather_rows(s2, idx, o2)
    return out


def sample_pack(scores, ids):
    """Per-shard sampling winners -> [rows, 2] f32 (score, id) pairs for the TP all-gather."""
    if not _gpu(scores):
        return ref.sample_pack(scores, ids)
    pair = _empty(scores.numel(), 2, dtype=torch.float32, device=scores.device)
    torch.ops.bfly.sample_pack(scores.contiguous(), ids.contiguous(), pair)
    return pair


def sample_merge(allp):
    """All-gathered pairs [tp, rows, 2] -> int32 ids of the best score per row (lowest rank on
    ties: torch.argmax's first maximum)."""
    if not _gpu(allp):
        return ref.sample_merge(allp)
    out = _empty(allp.shape[1], dtype=torch.int32, device=allp.device)
    torch.ops.bfly.sample_merge(allp.contiguous(), out)
    return out


def sample(logits, temps=None, seeds=None, vstart: int = 0, out_ids=None, out_scores=None, thresh=None,
           check_finite: bool = False):
    """Greedy / Gumbel-max sampling over a (vocab-shard of) logits -> (ids int32, scores f32).
    `thresh` [rows] f32: per-row lower bound on logit / temperature (top-k / top-p filter).
    `check_finite`: rows with an Inf / NaN logit get id -1 and score +inf (the NaN guard)."""
    if not _gpu(logits):
        return ref.sample(logits, temps, seeds, vstart, thresh, check_finite)
    rows = logits.shape[0]
    if out_ids is None:
        out_ids = _empty(rows, dtype=torch.int32, device=logits.device)
    if out_scores is None:
        out_scores = _empty(rows, dtype=torch.float32, device=logits.device)
    ws = _arena.get(logits.device, "sample", rows * 64, torch.int64)
    torch.ops.bfly.sample(logits, temps, seeds, vstart, out_ids, out_scores, ws, thresh, check_finite)
    return out_ids, out_scores


LOGPROBS_MAX_N = 20


def logprobs_partial(logits, ids, n: int, vstart: int = 0):
    """One vocab shard's logprob record [R, 3 + 2n] f32 (logprobs.hip; layout in
    ops.reference.logprobs_partial): the shard's log-softmax statistics, the logit of the chosen
    global id `ids[r]` (int32; -inf when it lies outside the shard) and the shard's `n` (0..20)
    largest logits with their global ids. `logits`: bf16 [R, V_local], a column slice of the
    padded logits is fine (row stride a multiple of 8)."""
    n = int(n)
    if not 0 <= n <= LOGPROBS_MAX_N:
        raise ValueError(f"logprobs: n must be in 0..{LOGPROBS_MAX_N}, got {n}")
    if not _gpu(logits):
        return ref.logprobs_partial(logits, ids, n, vstart)
    R, V = logits.shape
    rec = _empty(R, 3 + 2 * n, dtype=torch.float32, device=logits.device)
    ws = _arena.get(logits.device, "logprobs", torch.ops.bfly.logprobs_workspace_size(R, V, n), torch.int64)
    torch.ops.bfly.logprobs_partial(logits, ids.contiguous(), n, int(vstart), rec, ws)
    return rec


def logprobs_merge(records):
    """Shard records [tp, R, 3 + 2n] (tp = 1 too) -> (chosen_lp [R] f32, top_ids [R, n] int32,
    top_lp [R, n] f32): log_softmax over the whole vocabulary at the chosen token and at the n
    most likely ones (logit descending, global id ascending on ties; id -1 / -inf = none)."""
    if not _gpu(records):
        return ref.logprobs_merge(records)
    _, R, L = records.shape
    n = (L - 3) // 2
    # one buffer of 4-byte words behind the three outputs, so they reach the host in one copy
    packed = _empty(R * (1 + 2 * n), dtype=torch.float32, device=records.device)
    chosen, top_ids, top_lp = _logprobs_views(packed, R, n)
    torch.ops.bfly.logprobs_merge(records.contiguous(), chosen, top_ids, top_lp)
    return Logprobs(chosen, top_ids, top_lp, packed)


class Logprobs(tuple):
    """(chosen_lp, top_ids, top_lp) of `logprobs_merge`; `packed`: the one f32 buffer the three
    are views of (None on the reference path)."""

    def __new__(cls, chosen, top_ids, top_lp, packed=None):
        self = super().__new__(cls, (chosen, top_ids, top_lp))
        self.packed = packed
        return self


def _logprobs_views(packed, R: int, n: int):
    return (packed[:R], packed[R + R * n:].view(torch.int32).view(R, n), packed[R:R + R * n].view(R, n))


def logprobs_to_host(lp, non_blocking: bool = False):
    """Host copies of a `logprobs_merge` result: GPU results travel as one copy of their shared
    buffer, into pinned memory and asynchronous on the current stream when `non_blocking` (the
    caller orders its reads with an event)."""
    packed = getattr(lp, "packed", None)
    if packed is None or not packed.is_cuda:
        return tuple(t.cpu() for t in lp)
    R, n = lp[1].shape
    host = torch.empty(packed.shape, dtype=packed.dtype, pin_memory=non_blocking)
    host.copy_(packed, non_blocking=non_blocking)
    return _logprobs_views(host, R, n)


PENALTY_MAX_HISTORY = 65535   # tokens of one history (penalties.hip counts in 16-bit halves)


def penalty_params(params) -> torch.Tensor:
    """Host rows [R, 4] f32 (rep, 1 / rep, freq, pres) for `apply_penalties` from (repetition,
    frequency, presence) triples; the f32 reciprocal is taken here, on the host."""
    return ref.penalty_params(params)


def apply_penalties(logits, hist, slots, lens, prompt_lens, last, params, vstart: int = 0):
    """Presence / frequency / repetition penalties over a (vocab-shard of) logits [R, V], out of
    place (penalties.hip; semantics in ops.reference.apply_penalties). hist [slots, width] int32
    token histories (width a multiple of 4, below 65536); slots / lens / prompt_lens / last [R]
    int32; params [R, 4] f32 (`penalty_params`). Stores last[r] to hist[slot, len - 1]. Rows with
    slot < 0 are copied. The result is a view of an arena buffer: the next call overwrites it.
    `logits`: a column slice of the padded logits is fine (row stride a multiple of 8)."""
    if not _gpu(logits):
        return ref.apply_penalties(logits, hist, slots, lens, prompt_lens, last, params, vstart)
    R, V = logits.shape
    stride = (V + 7) // 8 * 8
    buf = _arena.get(logits.device, "penalties", R * stride, logits.dtype)[:R * stride]
    if _POISON:
        _poisoned(buf)
    out = buf.view(R, stride)[:, :V]
    torch.ops.bfly.apply_penalties(logits, int(vstart), hist, slots, lens, prompt_lens, last, params, out)
    return out


def topkp_threshold(logits, temps, top_k, top_p, reduce_sum=None, reduce_max=None,
                    use_k: bool = True, use_p: bool = True):
    """Exact per-row top-k / top-p threshold on logit / temperature by radix select (4 passes
    of 8 bits per filter, sample.hip tkp_*). `reduce_sum(t)` / `reduce_max(t)`: in-place
    all-reduces over the TP group applied to every histogram / the row maxima, so vocab shards
    select together (None: unsharded). `use_k` / `use_p`: skip a filter no row uses. Returns
    thresh [R] f32 (-inf = unfiltered row), the `thresh` argument of `sample`."""
    if not _gpu(logits):
        return ref.topkp_threshold(logits, temps, top_k, top_p, reduce_sum, reduce_max, use_k, use_p)
    R = logits.shape[0]
    L = torch.ops.bfly
    ws = _arena.get(logits.device, "tkp", R * 521, torch.float32)[: R * 521]
    zero_(ws)
    # the row-max slot starts at the smallest ordered key (INT_MIN = below signed_ordered(-inf)):
    # a zero would read as +0.0 and clamp the max of an all-negative row
    L.fill32_(ws[R * 8:R * 9], -2 ** 31)
    L.tkp_begin(logits, temps, top_k, top_p, ws)
    if reduce_max is not None:
        reduce_max(ws[R * 8:R * 9].view(torch.int32))
    hist = ws[R * 9:].view(R, 512)
    for phase, on in ((0, use_k), (1, use_p)):
        if not on:
            continue
        for p in range(4):
            L.tkp_pass(logits, temps, ws, p, phase)
            if reduce_sum is not None:
                reduce_sum(hist)
            L.tkp_select(top_p, ws, R, p, phase)
    thr = _empty(R, dtype=torch.float32, device=logits.device)
    L.tkp_final(ws, R, thr)
    return thr


def pack_w256(w: torch.Tensor) -> torch.Tensor:
    """A [N, K] weight in the K-tile-blocked layout [N/256][K/64][256][64] (returned viewed as
    [N, K]) that the packed decode GEMM reads (gemm.hip launch_gemm_packed)."""
    N, K = w.shape
    return w.view(N // 256, 256, K // 64, 64).permute(0, 2, 1, 3).contiguous().view(N, K)


def linear(x, w, bias=None, epilogue: str = "none", out=None, defer: bool = False, packed=None):
    """y = x @ w.T (+ bias) with optional fused SwiGLU epilogue ('silu': w rows gate/up
    interleaved in 16-row groups, output width w.shape[0] // 2). `defer=True` (no bias /
    epilogue): when the plan splits K, return a `Partial` whose reduce the consumer fuses.
    `packed`: the weight's pack_w256 copy: used when the shape's plan has a packed form (decode
    tile plans), else `w`."""
    rn = None
    if isinstance(x, RowNormed):   # consumer of a row-split RMSNorm: the GEMM applies 1/rms
        rn, x = x, x.y
    if not _gpu(x):
        return ref.linear(x, w, bias, epilogue, out)
    if packed is not None and bias is None and epilogue in ("none", "silu") and not (defer and epilogue != "none"):
        M, N = x.shape[0], w.shape[0]
        if out is None:
            out = _empty(M, N // 2 if epilogue == "silu" else N, dtype=x.dtype, device=x.device)
        need = torch.ops.bfly.gemm_workspace_size(M, N, x.shape[1])
        ws = _arena.get(x.device, "gemm", need // 4 + 1, torch.float32, zero=True) if need else None
        sk = torch.ops.bfly.gemm_packed(x, packed, out, EPILOGUES[epilogue], rn.ssp if rn is not None else None,
                                        rn.eps if rn is not None else 0.0, None, 0, 1, ws, bool(defer))
        if sk == 1:
            return out
        if sk > 1:     # deferred split-K slabs for the consumer
            off = torch.ops.bfly.gemm_slab_offset()
            return Partial(ws[off:off + sk * M * N].view(sk, M, N), out)
    if defer and bias is None and epilogue == "none":
        M, N = x.shape[0], w.shape[0]
        if out is None:
            out = _empty(M, N, dtype=x.dtype, device=x.device)
        need = torch.ops.bfly.gemm_workspace_size(M, N, x.shape[1])
        ws = _arena.get(x.device, "gemm", need // 4 + 1, torch.float32, zero=True)
        if rn is not None:
            sk = torch.ops.bfly.gemm_deferred_rs(x, w, out, ws, rn.ssp, rn.eps)
        else:
            sk = torch.ops.bfly.gemm_deferred(x, w, out, ws)
        if sk == 1:
            return out
        off = torch.ops.bfly.gemm_slab_offset()
        return Partial(ws[off:off + sk * M * N].view(sk, M, N), out)
    epi = EPILOGUES["bias"] if (bias is not None and epilogue == "none") else EPILOGUES[epilogue]
    if epilogue == "silu" and bias is not None:
        raise ValueError("bias + silu epilogue not supported")
    M, N = x.shape[0], w.shape[0]
    nout = N // 2 if epilogue == "silu" else N
    if out is None:
        out = _empty(M, nout, dtype=x.dtype, device=x.device)
    need = torch.ops.bfly.gemm_workspace_size(M, N, x.shape[1])
    # zero-initialised once: its head holds the split-K arrival counters, which every GEMM
    # leaves re-armed at zero
    ws = _arena.get(x.device, "gemm", need // 4 + 1, torch.float32, zero=True) if need else None
    if rn is not None:
        torch.ops.bfly.gemm_rs(x, w, out, bias, epi, ws, rn.ssp, rn.eps)
    else:
        torch.ops.bfly.gemm(x, w, out, bias, epi, ws)
    return out


def quantize_fp8(w):
    """FP8 e4m3 weight-only quantisation of a [N, K] weight (ops.reference.quantize_fp8 has the
    format): returns (code torch.float8_e4m3fn [N, K], scale f32 [N])."""
    if not _gpu(w):
        return ref.quantize_fp8(w)
    if w.dim() != 2 or w.dtype != torch.bfloat16:
        raise ValueError("quantize_fp8: a 2-D bf16 weight")
    if w.stride(1) != 1 or w.stride(0) % 8 != 0 or w.data_ptr() % 16 != 0:
        w = w.contiguous()
    code = _empty(w.shape[0], w.shape[1], dtype=torch.float8_e4m3fn, device=w.device)
    scale = _empty(w.shape[0], dtype=torch.float32, device=w.device)
    torch.ops.bfly.quant_fp8_rows(w, code, scale)
    return code, scale


def dequantize_fp8(code, scale, dtype=None, out=None):
    """dtype(float(code) * scale[:, None]) (GPU: bf16, dequant_fp8_kernel)."""
    if not _gpu(code):
        y = ref.dequantize_fp8(code, scale, dtype or torch.float32)
        return y if out is None else out.copy_(y)
    if dtype not in (None, torch.bfloat16):
        raise ValueError("dequantize_fp8: the GPU kernel writes bf16")
    if out is None:
        out = _empty(code.shape[0], code.shape[1], dtype=torch.bfloat16, device=code.device)
    torch.ops.bfly.dequant_fp8(code, scale, out)
    return out


def linear_w8(x, code, scale, epilogue: str = "none", out=None):
    """y = (x @ float(code).T) * scale with optional fused SwiGLU epilogue: the FP8 e4m3
    weight-only counterpart of `linear` (no bias). Shapes and row counts the native kernel
    takes (gemm_w8_check) stream the codes once (gemm_w8.hip, wq_gemm_kernel<W8Fmt>); every other one
    widens the codes into the arena's bf16 scratch, runs `linear` on it and scales the result."""
    if not _gpu(x):
        return ref.linear_w8(x, code, scale, epilogue, out)
    if epilogue not in ("none", "silu"):
        raise ValueError(f"linear_w8: epilogue {epilogue!r} not supported (no bias)")
    M, K = x.shape
    N = code.shape[0]
    epi = EPILOGUES[epilogue]
    if torch.ops.bfly.gemm_w8_check(M, N, K, epi) == 0:
        if out is None:
            out = _empty(M, N // 2 if epilogue == "silu" else N, dtype=x.dtype, device=x.device)
        need = torch.ops.bfly.gemm_w8_workspace_size(M, N, K)
        ws = _arena.get(x.device, "gemm_w8", need // 4 + 1, torch.float32) if need else None
        torch.ops.bfly.gemm_w8(x, code, scale, out, epi, ws, False)
        return out
    # bare codes are exact in bf16: the bf16 GEMM runs on them and the scale multiplies its
    # result (as the native kernel scales its accumulators), then SwiGLU
    wd = _arena.get(x.device, "w8_deq", N * K, torch.bfloat16)[:N * K].view(N, K)
    torch.ops.bfly.dequant_fp8(code, None, wd)
    if out is None:
        out = _empty(M, N // 2 if epilogue == "silu" else N, dtype=x.dtype, device=x.device)
    if epilogue == "silu":
        y = _arena.get(x.device, "w8_tmp", M * N, torch.bfloat16)[:M * N].view(M, N)
        linear(x, wd, out=y)
    else:
        y = linear(x, wd, out=out)
    if M:
        torch.ops.bfly.w8_scale_cols(y, scale, out, epi)
    return out


def quantize_mxfp4(w):
    """OCP MXFP4 weight-only quantisation of a [N, K] weight, K % 32 == 0
    (ops.reference.quantize_mxfp4 has the format): returns (code uint8 [N, K / 2], two e2m1
    codes per byte, scale uint8 [N, K / 32], one e8m0 byte per 32 elements)."""
    if not _gpu(w):
        return ref.quantize_mxfp4(w)
    if w.dim() != 2 or w.dtype != torch.bfloat16 or w.shape[1] % ref.MXFP4_BLOCK != 0:
        raise ValueError("quantize_mxfp4: a 2-D bf16 weight with K % 32 == 0")
    if w.stride(1) != 1 or w.stride(0) % 8 != 0 or w.data_ptr() % 16 != 0:
        w = w.contiguous()
    N, K = w.shape
    code = _empty(N, K // 2, dtype=torch.uint8, device=w.device)
    scale = _empty(N, K // ref.MXFP4_BLOCK, dtype=torch.uint8, device=w.device)
    torch.ops.bfly.quant_mxfp4(w, code, scale)
    return code, scale


def dequantize_mxfp4(code, scale, dtype=None, out=None):
    """dtype(value(code) * 2^(scale - 127)) [N, K], exact (GPU: bf16, dequant_mxfp4_kernel).
    Scale bytes must lie in 2 .. 252, the range `quantize_mxfp4` writes (every result a normal
    bf16); other bytes are invalid input: the GPU kernels give 0 for byte 0 and infinity for 255."""
    if not _gpu(code):
        y = ref.dequantize_mxfp4(code, scale, dtype or torch.float32)
        return y if out is None else out.copy_(y)
    if dtype not in (None, torch.bfloat16):
        raise ValueError("dequantize_mxfp4: the GPU kernel writes bf16")
    if out is None:
        out = _empty(code.shape[0], 2 * code.shape[1], dtype=torch.bfloat16, device=code.device)
    torch.ops.bfly.dequant_mxfp4(code, scale, out)
    return out


def linear_w4(x, code, scale, epilogue: str = "none", out=None):
    """y = linear(x, dequantize_mxfp4(code, scale), epilogue): the MXFP4 weight-only
    counterpart of `linear` (no bias). Shapes and row counts the native kernel takes
    (gemm_w4_check) stream the codes once (gemm_w4.hip, wq_gemm_kernel<W4Fmt>); every other one writes
    the dequantised weights, which bf16 holds exactly, into the arena's scratch and runs
    `linear` on them with the same epilogue. Scale bytes must lie in 2 .. 252 (`dequantize_mxfp4`)."""
    if not _gpu(x):
        return ref.linear_w4(x, code, scale, epilogue, out)
    if epilogue not in ("none", "silu"):
        raise ValueError(f"linear_w4: epilogue {epilogue!r} not supported (no bias)")
    M, K = x.shape
    N = code.shape[0]
    epi = EPILOGUES[epilogue]
    if out is None:
        out = _empty(M, N // 2 if epilogue == "silu" else N, dtype=x.dtype, device=x.device)
    if torch.ops.bfly.gemm_w4_check(M, N, K, epi) == 0:
        need = torch.ops.bfly.gemm_w4_workspace_size(M, N, K)
        ws = _arena.get(x.device, "gemm_w4", need // 4 + 1, torch.float32) if need else None
        torch.ops.bfly.gemm_w4(x, code, scale, out, epi, ws, False)
        return out
    wd = _arena.get(x.device, "w8_deq", N * K, torch.bfloat16)[:N * K].view(N, K)
    torch.ops.bfly.dequant_mxfp4(code, scale, wd)
    return linear(x, wd, epilogue=epilogue, out=out)


LORA_RANKS = ref.LORA_RANKS
LORA_MAX_SPLITK = 16     # kLoraMaxSplitK


def _lora_part(x, J: int, splitk, arena: bool):
    T, K = x.shape
    ks = int(splitk) if splitk else torch.ops.bfly.lora_splitk(T, K)
    n = ks * T * J
    if arena:
        part = _arena.get(x.device, "lora_t", n, torch.float32)[:n]
        return (_poisoned(part) if _POISON else part).view(ks, T, J)
    # stand-alone result: rows without an adapter are not written
    return torch.zeros(ks, T, J, dtype=torch.float32, device=x.device)


def lora_shrink(x, a, idx, splitk: int = 0):
    """t [T, J] f32 = the rows' adapters' `a` times x (lora.hip; semantics in
    ops.reference.lora_shrink): x [T, K], a [S, J, K], idx [T] int32, an index outside [0, S)
    meaning no adapter (a zero row). `splitk`: the kernel's K split (0: its own choice); the
    partial sums are added here in split order. The hot path is `lora_add_`."""
    if not _gpu(x):
        return ref.lora_shrink(x, a, idx)
    part = _lora_part(x, a.shape[1], splitk, arena=False)
    torch.ops.bfly.lora_shrink(x, a, idx, part)
    t = part[0]
    for k in range(1, part.shape[0]):
        t = t + part[k]
    return t


def lora_expand_(y, t, b, seg, scale, idx):
    """In place: y [T, N] += scale[s] * (t [T, J] f32 times b [S, N, R] of the rows' adapters),
    seg [N] uint8 naming the rank slice of each output row, rows without an adapter untouched
    (lora.hip; semantics in ops.reference.lora_expand_)."""
    if not _gpu(y):
        return ref.lora_expand_(y, t, b, seg, scale, idx)
    torch.ops.bfly.lora_expand(y, t.view(1, *t.shape), b, seg, scale, idx)
    return y


def lora_add_(y, x, a, b, seg, scale, idx, splitk: int = 0):
    """y += the LoRA delta of x under each row's adapter: shrink into the arena's `lora_t` slab
    (K-split partial sums, reduced by the expand kernel), then expand in place. Two launches, no
    allocation once the arena holds the slab (`reserve_lora_workspace`)."""
    if not _gpu(y):
        return ref.lora_add_(y, x, a, b, seg, scale, idx)
    part = _lora_part(x, a.shape[1], splitk, arena=True)
    torch.ops.bfly.lora_shrink(x, a, idx, part)
    torch.ops.bfly.lora_expand(y, part, b, seg, scale, idx)
    return y


def reserve_lora_workspace(device, max_tokens: int, max_j: int) -> None:
    """Size the `lora_t` slab for up to `max_tokens` rows of `max_j` rank columns (before capture)."""
    if load_library() and torch.device(device).type == "cuda":
        # lora_splitk(T, K) <= min(16, 512 / tiles): split x rows stays below 8192 or is T itself
        rows = max(max_tokens, min(LORA_MAX_SPLITK * max(max_tokens, 1), 8192))
        _arena.get(device, "lora_t", rows * max_j, torch.float32)


def linear_silu_gate(x, w, gates, e0: int, num_local: int, packed=None):
    """The dense MoE decode gate/up GEMM over the concatenated local experts: SwiGLU, then every
    expert's column block scaled by its routing weight gates[:, e0 + e] — `linear(x, w, 'silu')`
    followed by `moe_gate_scale_`, bit for bit, in one launch (the tile kernel's epilogue).
    `packed`: the weight's pack_w256 copy (used when the plan has a packed form)."""
    if isinstance(x, RowNormed) or not _gpu(x):
        h = linear(x, w, epilogue="silu")
        return moe_gate_scale_(h, gates, e0, num_local)
    out = _empty(x.shape[0], w.shape[0] // 2, dtype=x.dtype, device=x.device)
    if packed is not None and torch.ops.bfly.gemm_packed(x, packed, out, 3, None, 0.0, gates, e0, num_local) > 0:
        return out
    torch.ops.bfly.gemm_silu_gate(x, w, out, gates, e0, num_local)
    return out


# plan kind names by number; "mixed": tile plan with column tiles of two widths (bn wide, wk narrow)
GEMM_KINDS = ("skinny", "tile", "big", "dec", "big8", "mid8", "big4", "mid4", "mixed")


def gemm_plan(M: int, N: int, K: int) -> dict:
    load_library()
    k, mt, nt, bm, bn, sk, wk = torch.ops.bfly.gemm_plan(M, N, K)
    return {"kind": GEMM_KINDS[k], "mt": mt, "nt": nt, "wk": wk, "bm": bm, "bn": bn, "splitk": sk}


def attn_prefill(q, k, v, cu_seqlens, max_seqlen: int, scale: float, causal: bool = True,
                 out=None, cu_seqlens_k=None, return_lse: bool = False):
    """Varlen flash attention (K3). `cu_seqlens_k`: keys of each sequence come from other
    rows than its queries (non-causal; context-parallel ring steps). `return_lse`: also return
    the per-(row, head) natural-log sum-exp of the scaled scores [T, Hq] f32 (-inf: no keys),
    which `attn_lse_merge_` uses to combine attention over key chunks."""
    if not _gpu(q):
        return ref.attn_prefill(q, k, v, cu_seqlens, max_seqlen, scale, causal, out, cu_seqlens_k, return_lse)
    if out is None:
        out = _empty(q.shape, dtype=q.dtype, device=q.device)
    lse = _empty(q.shape[0], q.shape[1], dtype=torch.float32, device=q.device) if return_lse else None
    torch.ops.bfly.attn_prefill(q, k, v, cu_seqlens, max_seqlen, scale, causal, out, cu_seqlens_k, lse)
    return (out, lse) if return_lse else out


def attn_prefill_paged(q, k_cache, v_cache, tables, cu_q, positions, max_q: int, scale: float, out=None):
    """Chunked prefill attention over the paged cache (attention_paged.hip): query rows
    [cu_q[s], cu_q[s+1]) of sequence s at `positions` attend causally to the sequence's cached
    keys through tables[s] — the cached prefix and the chunk itself (already appended by
    rope_kv) in one pass, no gather, no log-sum-exp merge. Caches bf16 or FP8."""
    if not _gpu(q):
        return ref.attn_prefill_paged(q, k_cache, v_cache, tables, cu_q, positions, max_q, scale, out)
    if out is None:
        out = _empty(q.shape, dtype=q.dtype, device=q.device)
    torch.ops.bfly.attn_prefill_paged(q, k_cache, v_cache, tables, cu_q, positions, int(max_q), float(scale), out)
    return out


def attn_lse_merge_(acc_o, acc_lse, o, lse):
    """K16: fold a partial attention result (o bf16 [T, H, D], lse [T, H]) into running f32
    accumulators (acc_o [T, H, D], acc_lse [T, H]) in place."""
    if not _gpu(acc_o):
        return ref.attn_lse_merge_(acc_o, acc_lse, o, lse)
    torch.ops.bfly.attn_lse_merge(acc_o, acc_lse, o, lse)
    return acc_o, acc_lse


def attn_decode(q, k_cache, v_cache, block_tables, ctx_lens, scale: float, max_ctx: int,
                part_tokens: int = DECODE_PART_TOKENS, out=None):
    """One query token per sequence against the paged cache. `max_ctx` bounds ctx_lens (it
    fixes the split-KV grid, so it is a static parameter under graph capture)."""
    if not _gpu(q):
        return ref.attn_decode(q, k_cache, v_cache, block_tables, ctx_lens, scale, max_ctx,
                               part_tokens, out)
    B, Hq, D = q.shape
    Hkv = k_cache.shape[1]
    if out is None:
        out = _empty(B, Hq, D, dtype=q.dtype, device=q.device)
    if part_tokens <= 0:
        part_tokens = torch.ops.bfly.attn_decode_part_tokens(B, Hkv, max_ctx)
    ns = torch.ops.bfly.attn_decode_splits(max_ctx, part_tokens)
    po = pml = None
    if ns > 1:
        po = _arena.get(q.device, "attn_o", B * Hkv * ns * 16 * D, torch.float32)
        pml = _arena.get(q.device, "attn_ml", B * Hkv * ns * 16 * 2, torch.float32)
    torch.ops.bfly.attn_decode(q, k_cache, v_cache, block_tables, ctx_lens, scale, max_ctx,
                               part_tokens, out, po, pml)
    return out


def attn_verify_partials(B: int, QN: int, Hq: int, Hkv: int, D: int, max_ctx: int, part_tokens: int = 0):
    """(part_tokens, splits, part_o elements, part_ml elements) of an attn_verify call."""
    keys = max_ctx + QN - 1
    if part_tokens <= 0:
        part_tokens = torch.ops.bfly.attn_decode_part_tokens(B, Hkv, keys)
    ns = torch.ops.bfly.attn_decode_splits(keys, part_tokens)
    nc = 16 * torch.ops.bfly.attn_verify_tiles(QN, Hq // Hkv)
    return part_tokens, ns, B * Hkv * ns * nc * D, B * Hkv * ns * nc * 2


def reserve_verify_workspace(device, max_batch: int, spec_tokens: int, max_rows: int, num_heads: int,
                             num_kv_heads: int, head_dim: int, max_ctx: int) -> None:
    """Size the split partials of every attn_verify shape an engine's verify steps can take: up
    to `max_batch` sequences of 2 .. spec_tokens + 1 rows, at most `max_rows` rows in all."""
    if not load_library():
        return
    n_o = n_ml = 0
    for qn in range(2, spec_tokens + 2):
        for b in range(1, min(max_batch, max_rows // qn) + 1):
            _, ns, o, ml = attn_verify_partials(b, qn, num_heads, num_kv_heads, head_dim, max_ctx)
            if ns > 1:
                n_o, n_ml = max(n_o, o), max(n_ml, ml)
    if n_o:
        _arena.get(device, "attn_o", n_o, torch.float32)
        _arena.get(device, "attn_ml", n_ml, torch.float32)


def attn_verify(q, k_cache, v_cache, block_tables, ctx_lens, q_lens, scale: float, max_ctx: int,
                part_tokens: int = DECODE_PART_TOKENS, out=None):
    """Multi-query paged decode attention of a speculative verify step (attention_verify.hip).
    q [B, QN, Hq, D]: row 0 of a sequence is its newest token, rows 1 .. q_lens[b] - 1 its draft
    tokens, whose K/V rope_kv has already appended. Row t sees keys
    [0, ctx_lens[b] + min(t, q_lens[b] - 1)) (ctx_lens as in attn_decode: what row 0 sees);
    rows t >= q_lens[b] are padding, computed with the last valid row's limit. `max_ctx` is the
    static bound (it fixes the split grid): max_ctx + QN - 1 bounds every sequence's largest
    limit ctx_lens[b] + q_lens[b] - 1, so max_ctx bounds ctx_lens where q_lens[b] = QN.
    QN * (Hq / Hkv) <= 64. The K/V pages are streamed once for all rows."""
    if not _gpu(q):
        return ref.attn_verify(q, k_cache, v_cache, block_tables, ctx_lens, q_lens, scale, max_ctx,
                               part_tokens, out)
    B, QN, Hq, D = q.shape
    Hkv = k_cache.shape[1]
    if out is None:
        out = _empty(B, QN, Hq, D, dtype=q.dtype, device=q.device)
    part_tokens, ns, n_o, n_ml = attn_verify_partials(B, QN, Hq, Hkv, D, int(max_ctx), int(part_tokens))
    po = pml = None
    if ns > 1:
        po = _arena.get(q.device, "attn_o", n_o, torch.float32)
        pml = _arena.get(q.device, "attn_ml", n_ml, torch.float32)
    torch.ops.bfly.attn_verify(q, k_cache, v_cache, block_tables, ctx_lens, q_lens, float(scale), int(max_ctx),
                               part_tokens, out, po, pml)
    return out


def init_hash_(out, grow0: int, gcol0: int, gcols: int, seed: int, amp: float):
    """Fill a 2-D (view of a) weight shard with partition-independent hashed uniform values."""
    if not _gpu(out):
        return ref.init_hash(out, grow0, gcol0, gcols, seed, amp)
    torch.ops.bfly.init_hash(out, grow0, gcol0, gcols, seed & 0xFFFFFFFF, amp)
    return out


def moe_route(x, wr, top_k: int, gates=None, topk_ids=None, topk_w=None):
    if not _gpu(x):
        return ref.moe_route(x, wr, top_k)
    T, E = x.shape[0], wr.shape[0]
    if gates is None:
        gates = _empty(T, E, dtype=torch.float32, device=x.device)
    if topk_ids is None:
        topk_ids = _empty(T, top_k, dtype=torch.int32, device=x.device)
    if topk_w is None:
        topk_w = _empty(T, top_k, dtype=torch.float32, device=x.device)
    torch.ops.bfly.moe_route(x, wr, top_k, gates, topk_ids, topk_w)
    return gates, topk_ids, topk_w


def moe_sparse_ffn(x, topk_ids, topk_w, gu_w, down_w, e0: int, num_local: int, ffn: int,
                   expected_slots: Optional[int] = None, block_counts: Optional[tuple] = None):
    """Routed expert FFN: permute the (token, k) pairs of the local experts into per-expert
    row slots (moe_align), grouped gate/up GEMM with fused SiLU over gathered token rows,
    grouped down GEMM, weighted combine back to token order. Only routed rows are computed
    (the dense path computes every local expert for every token).
    `block_counts` = (counts [nblk] int32 on the device, cap): the rows are nblk blocks of `cap`
    rows of which only the first counts[b] are valid (the EP IPC prefill receive buffer, sized
    for the worst case): the other rows get no expert work and no output row."""
    if not _gpu(x):
        if block_counts is not None:
            cnt, cap = block_counts
            r = torch.arange(x.shape[0]) % cap
            ok = r < cnt.cpu().long()[torch.arange(x.shape[0]) // cap]
            topk_ids = topk_ids.masked_fill(~ok.unsqueeze(1), -1)
        return ref.moe_sparse_ffn(x, topk_ids, topk_w, gu_w, down_w, e0, num_local, ffn)
    T, H = x.shape
    k = topk_ids.shape[1]
    TK = T * k
    if TK == 0:
        return zero_(torch.empty(T, H, dtype=x.dtype, device=x.device))
    L = torch.ops.bfly
    dev = x.device
    bcnt, bcap = block_counts if block_counts is not None else (None, 0)
    # tile rows from the expected rows per expert (all slots are local in the EP dispatch):
    # one 128-row tile reads each expert's weights once where two 64-row tiles would twice
    # `expected_slots`: (token, k) pairs expected to be local (the EP dispatch pads with
    # non-local / empty slots; they cost nothing but must not size the launch)
    exp = TK if expected_slots is None else max(1, min(TK, expected_slots))
    # prefill-scale expert batches (>= 256 rows per local expert on average): the 8-phase
    # 256x256 tile over the tile list (gemm.hip gemm_big8_kernel<GROUPED>)
    bm = 256 if (exp >= 256 * num_local and H % 256 == 0 and (2 * ffn) % 256 == 0 and _BIG_MOE) else \
        (128 if exp >= 96 * num_local else 64)
    rows = _arena.get(dev, "moe_rows", TK, torch.int32)[:TK]
    slot_of = _arena.get(dev, "moe_slot", TK, torch.int32)[:TK]
    nt = L.moe_max_tiles(TK, num_local, bm)
    tiles = _arena.get(dev, "moe_tiles", nt * 4, torch.int32)[:nt * 4].view(nt, 4)
    count = _arena.get(dev, "moe_count", 1, torch.int32)[:1]
    L.moe_align(topk_ids, e0, num_local, rows, slot_of, tiles, count, bm, bcnt, bcap)
    hmid = _empty(TK, ffn, dtype=x.dtype, device=dev)
    L.moe_grouped_gemm(x, gu_w, hmid, rows, tiles, count, 2 * ffn * H, 2 * ffn, H, num_local, EPILOGUES["silu"], bm)
    out = _empty(T, H, dtype=x.dtype, device=dev)
    sk = moe_down_splits(exp, num_local, H, ffn, bm)
    if sk > 1:
        # decode-sized expert batches: split K of the down projection over sk workgroups so the
        # chip fills; the slab reduce is folded into the weighted combine
        part = _arena.get(dev, "moe_part", sk * TK * H, torch.float32)[: sk * TK * H].view(sk, TK, H)
        L.moe_grouped_gemm(hmid, down_w, hmid.new_empty(TK, H), None, tiles, count, ffn, H, ffn, num_local,
                           EPILOGUES["none"], bm, part)
        L.moe_combine_slabs(part, slot_of, topk_w, out, bcnt, bcap)
        return out
    y = _empty(TK, H, dtype=x.dtype, device=dev)
    L.moe_grouped_gemm(hmid, down_w, y, None, tiles, count, ffn, H, ffn, num_local, EPILOGUES["none"], bm)
    L.moe_combine(y, slot_of, topk_w, out, bcnt, bcap)
    return out


def ep_pack(x, ids, w, slots, experts_per_rank: int, ep: int, cap: int):
    """Pack a fixed-capacity EP dispatch (see ops.reference.ep_pack for the layout)."""
    if not _gpu(x):
        return ref.ep_pack(x, ids, w, slots, experts_per_rank, ep, cap)
    T, H = x.shape
    k = ids.shape[1]
    send = _empty(ep * cap, H, dtype=x.dtype, device=x.device)
    meta = _empty(ep * cap, 2 * k, dtype=torch.float32, device=x.device)
    slot = _empty(T, ep, dtype=torch.int32, device=x.device)
    torch.ops.bfly.ep_pack(x.contiguous(), ids.contiguous(), w.contiguous(), slots, experts_per_rank, ep, cap,
                           send, meta, slot)
    return send, meta, slot


def ep_combine(back, slot):
    """Sum each token's returned partial outputs (one per rank it was sent to)."""
    if not _gpu(back):
        return ref.ep_combine(back, slot)
    out = _empty(slot.shape[0], back.shape[1], dtype=back.dtype, device=back.device)
    torch.ops.bfly.ep_combine(back, slot, out)
    return out


def moe_down_splits(TK: int, num_local: int, H: int, ffn: int, bm: int, cus: int = 256) -> int:
    """Split-K factor of the grouped down projection: enough workgroups for ~2 per CU, with
    at least 16 K-tiles (1024 columns) per split (none for the 256-row big tile)."""
    if bm == 256:
        return 1
    tiles = -(-TK // bm) + (num_local if TK >= num_local else 0)
    wgs = max(1, tiles) * (H // 128)
    sk = 1
    while wgs * sk * 2 <= 2 * cus and (ffn // 64) // (sk * 2) >= 16 and sk < 8:
        sk *= 2
    return sk


def moe_gate_scale_(h, gates, e0: int, num_local: int):
    if not _gpu(h):
        return ref.moe_gate_scale(h, gates, e0, num_local)
    torch.ops.bfly.moe_gate_scale(h, gates, e0, num_local)
    return h
