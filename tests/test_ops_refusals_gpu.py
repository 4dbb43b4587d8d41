"""Every torch.ops.bfly binding refuses a tensor argument it cannot hand to its kernel.

One table entry per op: a valid call at ZERO rows (tokens, M), weights and tables at small real
sizes. At that count the launcher returns before it launches (read in csrc/kernels for every
entry: the early return on rows / T / M / B / nseq / max_q <= 0, or the binding's own guard in
splitk_reduce and moe_grouped_gemm), so a check that is missing shows as "did not raise" and never
as a kernel reading a bad pointer. Two entries have no empty form and launch one tiny valid kernel
in their positive control (LAUNCHING): ep_pack still has to write the padding metadata of an
empty batch, probe has no size at all. Their mutated calls are refused before the launch like all
others.

Per tensor argument (optionals and outputs included) the call is repeated with
  cpu     a CPU copy (not for an op's only tensor: the dispatcher refuses an all-CPU call first),
  dtype   the same shape in a wider dtype,
  strided a same-shape non-contiguous view, where the launcher takes no stride for it,
  size    one extra row or element, where the size is checked by equality,
and must raise a RuntimeError that starts "<op>: <argument> ".

BFLY_REFUSALS_PARENT=1 (with BFLY_KERNEL_LIB naming a library built from an earlier commit) turns
the message match off and leaves out the entries that rely on a binding-level guard or launch,
so the same table lists which mutations that library let through
(profiles/ops_args/README.md)."""
import os
import re
from pathlib import Path

import pytest
import torch

from butterfly_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
PARENT = os.environ.get("BFLY_REFUSALS_PARENT") == "1"
BF, F32, F64, I32, I64, U8 = torch.bfloat16, torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8
WIDER = {BF: F32, F32: F64, I32: I64, I64: F64, U8: torch.int16}   # int64 has no wider integer: another 8-byte type


@pytest.fixture(autouse=True, scope="module")
def _kernels_loaded():
    assert ops.load_library(), "butterfly_amd/_C.so not built or failed to load"


class A:
    """A tensor argument of a zero-row call.

    dense: the launcher takes no stride for it (mutation `strided` applies)
    grow:  the dimension whose size is checked by equality and that no other size is derived
           from (mutation `size` adds one to it); None: no such dimension
    wider: the dtype of mutation `dtype` (None: the op takes any dtype)"""

    def __init__(self, *shape, dtype=BF, dense=True, grow=0, wider="auto"):
        self.shape, self.dtype, self.dense, self.grow = list(shape), dtype, dense, grow
        self.wider = WIDER[dtype] if wider == "auto" else wider

    def make(self, mutation=None):
        shape, dtype, device = list(self.shape), self.dtype, DEV
        if mutation == "cpu":
            device = "cpu"
        elif mutation == "dtype":
            dtype = self.wider
        elif mutation == "size":
            shape[self.grow] += 1
        if mutation == "strided":   # every other column of a buffer twice as wide
            if shape[-1] != 1:
                t = torch.zeros(shape[:-1] + [2 * shape[-1]], dtype=dtype, device=device)[..., ::2]
                assert t.stride(-1) == 2
            else:                   # one column: the stride of a size-1 dimension means nothing, so space the rows
                t = torch.zeros(shape[:-1] + [2], dtype=dtype, device=device)[..., :1]
                assert t.stride(-2) == 2 and shape[-2] != 1
            assert list(t.shape) == shape
            return t
        return torch.zeros(shape, dtype=dtype, device=device)

    def mutations(self, only_tensor):
        out = [] if only_tensor else ["cpu"]
        if self.wider is not None:
            out.append("dtype")
        if self.dense:
            out.append("strided")
        if self.grow is not None:
            out.append("size")
        return out


def R(*shape, dtype=BF, grow=None, **kw):
    """Rows passed with their stride; by default the argument other sizes are derived from."""
    return A(*shape, dtype=dtype, dense=False, grow=grow, **kw)


D, V, K, N = 64, 128, 64, 128          # hidden / vocab columns / GEMM K / GEMM N
KC = lambda: A(2, 1, 32, 128, grow=None)          # k_cache [blocks, Hkv, BS, D]; blocks is free
VC = lambda: A(2, 1, 128, 32)                     # v_cache [blocks, Hkv, D, BS]
LOGITS = lambda: R(0, V)
WS = lambda n=16: A(n, dtype=F32, grow=None)      # workspaces are sized by a lower bound
PLAN = [1, 3, 0, 2, 64, 128, 1]
GEMM3 = lambda nout=N: [R(0, K), R(N, K), R(0, nout, grow=0)]     # x, w, out


# op -> positional arguments of the valid zero-row call
TABLE = {
    "rms_norm": [R(0, D), A(D), 1e-5, R(0, D, grow=0), A(0, D)],
    "layer_norm": [A(0, D, grow=None), A(D), A(D), 1e-5, A(0, D), A(0, D)],
    "rope_kv": [A(0, 4 * D, grow=None), A(0, dtype=I32), A(16, D // 2, dtype=F32, grow=None), A(16, D // 2, dtype=F32),
                2, 1, A(0, dtype=I32), A(2, 1, 32, D, grow=None), A(2, 1, D, 32), A(1, 0, 4 * D, dtype=F32, grow=1)],
    "kv_append": [R(0, 1, D), R(0, 1, D, grow=0), A(0, dtype=I32), A(2, 1, 32, D, grow=None), A(2, 1, D, 32)],
    "silu_mul": [A(0, 2 * D), A(0, D, grow=None), 0],
    "gelu": [A(0, D, grow=None), A(0, D)],
    "add": [A(0, D, grow=None), A(0, D), A(0, D)],
    "embed": [A(0, dtype=I32, grow=None), A(16, D, grow=None), A(0, D), 0],
    "gather_rows": [R(4, D, wider=None), A(0, dtype=I32, grow=None, wider=torch.int16), R(0, D, grow=0)],
    "zero_": [A(0, dtype=F32, grow=None, wider=None)],
    "fill32_": [A(0, dtype=F32, grow=None), 0],
    "sample_pack": [A(0, dtype=F32, grow=None), A(0, dtype=I32), A(0, 2, dtype=F32)],
    "sample_merge": [A(2, 0, 2, dtype=F32, grow=None), A(0, dtype=I32)],
    "init_hash": [R(0, D), 0, 0, D, 1, 0.5],
    "sample": [LOGITS(), A(0, dtype=F32), A(0, dtype=I64), 0, A(0, dtype=I32), A(0, dtype=F32),
               A(64, dtype=I64, grow=None), A(0, dtype=F32), False],
    "logprobs_partial": [LOGITS(), A(0, dtype=I32), 2, 0, A(0, 7, dtype=F32), A(8, dtype=I64, grow=None)],
    "logprobs_merge": [A(2, 0, 7, dtype=F32, grow=None), A(0, dtype=F32), A(0, 2, dtype=I32), A(0, 2, dtype=F32)],
    "apply_penalties": [LOGITS(), 0, A(4, 8, dtype=I32, grow=None), A(0, dtype=I32), A(0, dtype=I32), A(0, dtype=I32),
                        A(0, dtype=I32), A(0, 4, dtype=F32), R(0, V, grow=0)],
    "tkp_begin": [LOGITS(), A(0, dtype=F32), A(0, dtype=I32), A(0, dtype=F32), WS(521)],
    "tkp_pass": [LOGITS(), A(0, dtype=F32), WS(521), 0, 0],
    "tkp_select": [A(0, dtype=F32), WS(521), 0, 0, 0],
    "tkp_final": [WS(521), 0, A(0, dtype=F32)],
    "gemm": GEMM3() + [A(N), 1, WS()],
    "gemm_silu_gate": GEMM3(N // 2) + [A(0, 4, dtype=F32), 0, 4],
    "gemm_packed": [R(0, K), A(256, K, grow=None), R(0, 128, grow=0), 3, A(0, 1, dtype=F32), 1e-5,
                    A(0, 4, dtype=F32), 0, 4, WS(), False],
    "quant_fp8_rows": [R(0, K), A(0, K, dtype=U8), A(0, dtype=F32)],
    "dequant_fp8": [A(0, K, dtype=U8, grow=None), A(0, dtype=F32), R(0, K, grow=0)],
    "w8_scale_cols": [R(0, N), A(N, dtype=F32), R(0, N, grow=0), 0],
    "gemm_w8": [R(0, 128), A(N, 128, dtype=U8, grow=None), A(N, dtype=F32), R(0, N, grow=0), 0, WS(), False, 0],
    "gemm_with_plan": GEMM3() + [PLAN, 1, WS(), A(N), False],
    "gemm_deferred": [R(0, K), R(N, K), A(0, N), WS()],
    "splitk_reduce": [A(2, 0, N, dtype=F32, grow=None), A(0, N)],
    "rms_norm_partial": [A(2, 0, D, dtype=F32, grow=None), A(D), 1e-5, A(0, D), A(0, D)],
    "rms_norm_partial_route": [A(2, 0, D, dtype=F32, grow=None), A(D), 1e-5, A(0, D), A(0, D), A(4, D, grow=None), 2,
                               A(0, 4, dtype=F32), A(0, 2, dtype=I32), A(0, 2, dtype=F32)],
    "gemm_rs": GEMM3() + [A(N), 1, WS(), A(0, 1, dtype=F32), 1e-5],
    "gemm_deferred_rs": [R(0, K), R(N, K), A(0, N), WS(), A(0, 1, dtype=F32), 1e-5],
    "rms_norm_rows": [R(0, D), A(D), A(0, D), A(0, 1, dtype=F32), A(0, D)],     # rms_norm_rows_chunks(64) = 1
    "attn_decode": [R(0, 2, 128), KC(), VC(), R(1, 4, dtype=I32), A(2, dtype=I32, grow=None), 0.1, 64, 32, A(0, 2, 128),
                    WS(), WS()],
    "attn_prefill": [R(0, 2, 128), R(0, 1, 128), R(0, 1, 128), A(2, dtype=I32, grow=None), 0, 0.1, False,
                     R(0, 2, 128, grow=0), A(2, dtype=I32), A(0, 2, dtype=F32)],
    "attn_prefill_paged": [R(0, 2, 128), KC(), VC(), R(1, 4, dtype=I32), A(2, dtype=I32, grow=None),
                           A(0, dtype=I32, grow=None), 0, 0.1, R(0, 2, 128, grow=0)],
    "attn_lse_merge": [A(0, 2, 128, dtype=F32, grow=None), A(0, 2, dtype=F32), R(0, 2, 128, grow=0), A(0, 2, dtype=F32)],
    "probe": [0, A(1024, dtype=F32, grow=None)],
    "moe_route": [R(0, D), A(4, D, grow=None), 2, A(0, 4, dtype=F32), A(0, 2, dtype=I32), A(0, 2, dtype=F32)],
    "moe_gate_scale": [A(0, D, grow=None), A(0, 4, dtype=F32), 0, 4],
    # count holds one element, so no view of it is strided
    "moe_align": [A(0, 2, dtype=I32, grow=None), 0, 4, A(0, dtype=I32, grow=None), A(0, dtype=I32),
                  A(4, 4, dtype=I32, grow=None), A(1, dtype=I32, dense=False), 64, A(2, dtype=I32, grow=None), 4],
    "moe_grouped_gemm": [R(0, K), R(4 * N, K), R(0, N), A(0, dtype=I32, grow=None), A(4, 4, dtype=I32, grow=None),
                         A(1, dtype=I32, dense=False, grow=None), N * K, N, K, 4, 0, 64, A(2, 0, N, dtype=F32, grow=1)],
    "moe_combine": [A(0, D, grow=None), A(0, dtype=I32), A(0, 2, dtype=F32, grow=None), A(0, D), A(2, dtype=I32, grow=None),
                    4],
    "moe_combine_slabs": [A(2, 0, D, dtype=F32, grow=None), A(0, dtype=I32), A(0, 2, dtype=F32, grow=None), A(0, D),
                          A(2, dtype=I32, grow=None), 4],
    "ep_pack": [A(0, D, grow=None), A(0, 2, dtype=I32), A(0, 2, dtype=F32), A(0, dtype=I32), 2, 2, 1, A(2, D),
                A(2, 4, dtype=F32), A(0, dtype=I32)],
    "ep_combine": [A(4, D, grow=None), A(0, dtype=I32, grow=None), A(0, D, grow=None)],
}

# Their launchers reach the peers' IPC buffers before any return on an empty batch.
EXCLUDED = {
    "custom_all_reduce": "every rank's workgroups publish to and spin on the peers' IPC buffers, rows or not",
    "ep_ipc_dispatch": "launches capmax workgroups that raise the peers' dispatch flags even for T = 0",
    "ep_ipc_dispatch_prefill": "its route and scatter kernels run for T = 0 and write the peers' totals and flags",
    "ep_ipc_wait": "takes no sized tensor; spins on the peers' flags",
    "ep_ipc_return": "launches capmax workgroups over the peers' receive blocks whatever the batch",
    "ep_ipc_combine": "launches one workgroup that waits on the peers' return flags for T = 0",
}

LAUNCHING = {"ep_pack", "probe"}                       # positive control runs one tiny valid kernel
GUARDED = {"splitk_reduce", "moe_grouped_gemm"}       # zero rows return in the binding, not in the launcher
if PARENT:
    for _op in LAUNCHING | GUARDED:
        TABLE.pop(_op)

# a scalar (or shape) check the bindings already had: op, what, {argument: refused value}
SCALARS = [
    ("tkp_pass", "pass 4", {"pass_": 4}),
    ("tkp_pass", "phase 2", {"phase": 2}),
    ("tkp_select", "pass 4", {"pass_": 4}),
    ("moe_align", "tile rows 32", {"bm": 32}),
    ("moe_align", "65 local experts", {"num_local": 65}),
    ("logprobs_partial", "n = 21", {"n": 21, "record": A(0, 45, dtype=F32)}),
    ("logprobs_partial", "ids reach 2^24", {"vstart": 1 << 24}),
    ("apply_penalties", "ids reach 2^24", {"vstart": 1 << 24}),
    ("apply_penalties", "hist width % 4", {"hist": A(4, 6, dtype=I32)}),
    ("gemm_with_plan", "plan of six", {"plan": PLAN[:6]}),
    ("gemm_with_plan", "bias without its epilogue", {"epilogue": 0}),
    ("gemm", "bias epilogue without bias", {"bias": None}),
    ("gemm", "K % 64", {"x": R(0, 96), "w": R(N, 96)}),
    ("gemm_deferred", "N % 128", {"w": R(64, K), "out": A(0, 64)}),
    ("gemm_packed", "bias epilogue", {"epilogue": 1}),
    ("gemm_silu_gate", "experts do not divide N / 2", {"num_local": 3}),
    ("gemm_w8", "bias epilogue", {"epilogue": 1}),
    ("w8_scale_cols", "bias epilogue", {"epilogue": 1}),
    ("w8_scale_cols", "N % 32", {"y": R(0, 48), "scale": A(48, dtype=F32), "out": R(0, 48)}),
    ("rope_kv", "heads do not divide the row", {"num_q_heads": 3}),
    ("rope_kv", "head_dim 32", {"num_q_heads": 6}),
    ("rope_kv", "slots without caches", {"k_cache": None}),
    ("kv_append", "head_dim 32", {"k": R(0, 1, 32), "v": R(0, 1, 32), "k_cache": A(2, 1, 32, 32), "v_cache": A(2, 1, 32, 32)}),
    ("rms_norm", "dim > 16384", {"x": R(0, 16392), "w": A(16392), "out": R(0, 16392), "residual": A(0, 16392)}),
    ("rms_norm", "dim % 8", {"x": R(0, 60), "w": A(60), "out": R(0, 60), "residual": A(0, 60)}),
    ("rms_norm_partial", "dim > 16384", {"slabs": A(2, 0, 16392, dtype=F32), "w": A(16392), "out": A(0, 16392),
                                         "residual": A(0, 16392)}),
    ("silu_mul", "interleave 4", {"interleave": 4}),
    ("gelu", "numel % 8", {"x": A(1, 4), "out": A(1, 4)}),
    ("moe_gate_scale", "experts do not divide the row", {"num_local": 3}),
    ("moe_grouped_gemm", "bias epilogue", {"epilogue": 1}),
    ("moe_grouped_gemm", "N % 128", {"n": 64}),
    ("moe_grouped_gemm", "expert slices exceed w", {"num_experts": 5}),
    ("attn_decode", "block table too narrow", {"max_ctx": 129}),
    ("attn_prefill", "key offsets with causal", {"causal": True}),
    ("attn_lse_merge", "head_dim 64", {"acc_o": A(0, 2, 64, dtype=F32), "o": R(0, 2, 64)}),
    ("logprobs_merge", "record width", {"records": A(2, 0, 6, dtype=F32)}),
    ("probe", "out too small", {"out": A(1023, dtype=F32)}),
    ("fill32_", "2-byte elements", {"t": A(0, dtype=BF)}),
    ("gather_rows", "odd 2-byte row", {"src": R(4, 63), "out": R(0, 63)}),
]
if PARENT:
    SCALARS = [s for s in SCALARS if s[0] in TABLE]


def _names(op):
    return [a.name for a in getattr(torch.ops.bfly, op).default._schema.arguments]


def _call(op, values):
    try:
        return getattr(torch.ops.bfly, op)(*[v.make() if isinstance(v, A) else v for v in values])
    finally:
        if PARENT:   # a host pointer that reached hipMemsetAsync leaves a sticky error to the next allocation
            torch.ops.bfly.hip_clear_error()


def _cases():
    out = []
    for op, specs in TABLE.items():
        tensors = [i for i, v in enumerate(specs) if isinstance(v, A)]
        for i in tensors:
            for m in specs[i].mutations(only_tensor=len(tensors) == 1):
                out.append(pytest.param(op, i, m, id=f"{op}-arg{i}-{m}"))
    return out


def test_table_and_exclusions_cover_every_registered_op():
    text = (Path(__file__).resolve().parent.parent / "csrc" / "bindings" / "ops.cpp").read_text()
    block = text[text.index("TORCH_LIBRARY_IMPL(bfly, CUDA, m)"):]
    registered = set(re.findall(r'm\.impl\("(\w+)"', block))
    assert len(registered) == 56
    table = set(TABLE) | (LAUNCHING | GUARDED if PARENT else set())
    assert not table & set(EXCLUDED)
    assert table | set(EXCLUDED) == registered
    # only ops over peer IPC buffers may be left out
    assert all(op == "custom_all_reduce" or op.startswith("ep_ipc_") for op in EXCLUDED)


@pytest.mark.parametrize("op", sorted(TABLE))
def test_zero_row_call_is_accepted(op):
    _call(op, TABLE[op])
    torch.cuda.synchronize()


@pytest.mark.parametrize("op,index,mutation", _cases())
def test_mutated_argument_is_refused(op, index, mutation):
    values = list(TABLE[op])
    arg = _names(op)[index]
    values[index] = values[index].make(mutation)
    match = None if PARENT else re.escape(f"{op}: {arg} ")
    with pytest.raises(RuntimeError, match=match):
        _call(op, values)


@pytest.mark.parametrize("op,what,override", [pytest.param(*s, id=f"{s[0]}-{s[1].replace(' ', '_')}") for s in SCALARS])
def test_refused_scalar(op, what, override):
    values, names = list(TABLE[op]), _names(op)
    for name, v in override.items():
        values[names.index(name)] = v
    with pytest.raises(RuntimeError, match=None if PARENT else re.escape(f"{op}: ")):
        _call(op, values)
