"""OCP MXFP4 weight-only quantisation on one MI355X: the quantise / dequantise kernels and the
native decode GEMM (csrc/kernels/gemm_w4.hip) against ops/reference.py, the dequantise route,
graph capture, the quantised model and engine end to end, and the bindings' refusals.

test_exact proves the layout: with random codes, scales of 2^0 .. 2^3 and small integer
activations every product is a multiple of .5 and every f32 sum exact in any order, so a swapped
nibble, a permuted k, a mis-indexed scale or an inexact conversion changes the bits of the
result. The tolerance tests use weights of random normal / sqrt(K) times per-row factors over
2^-6 .. 2^6 times per-block factors over 2^-4 .. 2^4: with near-equal scales a mis-indexed one
would pass unnoticed."""
import math
import re

import pytest
import torch

from butterfly_amd import ops
from butterfly_amd.config import EngineConfig, ModelConfig
from butterfly_amd.engine.batch import make_decode_batch, make_prefill_batch
from butterfly_amd.engine.engine import LLMEngine
from butterfly_amd.engine.sampler import SamplingParams
from butterfly_amd.models import build_model
from butterfly_amd.ops import reference as ref

from .test_ops_refusals_gpu import F32, U8, WS, A, R
from .test_w4_cpu import _clear_zero_sign, _unpack, edge_blocks

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [(256, 256), (1024, 256), (256, 512), (384, 640), (2048, 1024), (256, 4096)]
EXACT_SHAPES = [(256, 256), (384, 640), (2048, 1024), (256, 4096)]
NATIVE_M = [1, 5, 16, 17, 33, 64]                  # one 64-row tile, ragged last 16-row tiles
ROUTED_M = [65, 128, 200, 256, 300, 1024]          # row-tiled native kernel to its row limit, then dequantise
EPI = {"none": 0, "silu": 2}


@pytest.fixture(autouse=True, scope="module")
def _kernels_loaded():
    assert ops.load_library(), "butterfly_amd/_C.so not built or failed to load"


@pytest.fixture
def poisoned():
    prev = ops._POISON
    ops.set_poison(True)
    yield
    ops.set_poison(prev)


def _bf(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).to(DEV)


def _weight(N, K, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    rows = torch.logspace(-6, 6, N, base=2.0)[torch.randperm(N, generator=g)]
    nb = N * (K // 32)
    blocks = torch.logspace(-4, 4, nb, base=2.0)[torch.randperm(nb, generator=g)].view(N, K // 32)
    return (w * rows[:, None] * blocks.repeat_interleave(32, dim=1)).to(torch.bfloat16).to(DEV)


def _close(a, b, atol, rtol):
    a, b = a.float().cpu(), b.float().cpu()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = (~(err <= tol)).sum().item()     # NaN (an unwritten poisoned element) counts as bad
    assert bad == 0, f"{bad}/{a.numel()} mismatches, max err {err.max().item():.4g}"


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm()).item()


@pytest.mark.parametrize("N,K", [(256, 512), (1024, 256)])
def test_quantise_and_dequantise_kernels(N, K, poisoned):
    w = _weight(N, K, seed=3)
    blocks, want = edge_blocks()
    rows = [1, N // 2, N - 1]
    for i, n in enumerate(rows):               # the edge blocks at the start, inside and at the end of a row
        for j in range(blocks.shape[0]):
            b = (j + i * (K // 32 - blocks.shape[0]) // 2) % (K // 32)
            w[n, 32 * b:32 * b + 32] = blocks[j].to(DEV)
    code, scale = ops.quantize_mxfp4(w)
    assert code.dtype == torch.uint8 and code.shape == (N, K // 2) and code.is_cuda
    assert scale.dtype == torch.uint8 and scale.shape == (N, K // 32)
    rcode, rscale = ref.quantize_mxfp4(w.cpu())
    assert torch.equal(scale.cpu(), rscale)
    got, exp = _clear_zero_sign(_unpack(code.cpu())), _clear_zero_sign(_unpack(rcode))
    assert torch.equal(got, exp), f"{int((got != exp).sum())} codes differ"
    n, b = rows[0], 0                           # the planted blocks really are where the reference saw them
    for j, (E, mags) in want.items():
        assert int(scale[n, b + j]) == E + 127
        if mags is not None:
            assert (got[n, 32 * (b + j):32 * (b + j) + len(mags)] & 7).tolist() == mags
    deq = ops.dequantize_mxfp4(code, scale)
    assert deq.dtype == torch.bfloat16 and deq.shape == (N, K)
    want_deq = ref.dequantize_mxfp4(code.cpu(), scale.cpu(), torch.bfloat16)
    assert torch.equal(deq.cpu().float(), want_deq.float())          # NaN-free and equal (-0 == 0: zero signs)
    # every code and every scale the format has, through the dequantise kernel, bit for bit
    allc = torch.arange(256, dtype=torch.uint8).view(16, 16).repeat(251, 1)    # one block per row
    alls = torch.arange(2, 253, dtype=torch.uint8).repeat_interleave(16)[:, None]
    mag = (_unpack(allc) & 7) != 0
    d = ops.dequantize_mxfp4(allc.to(DEV), alls.to(DEV)).cpu()
    r = ref.dequantize_mxfp4(allc, alls, torch.bfloat16)
    assert torch.equal(d.view(torch.int16)[mag], r.view(torch.int16)[mag]) and bool((d[~mag] == 0).all())
    out = torch.full((N, K + 8), float("nan"), dtype=torch.bfloat16, device=DEV)
    assert ops.dequantize_mxfp4(code, scale, out=out[:, :K]) is not None       # strided rows of a wider buffer
    assert torch.equal(out[:, :K].cpu().float(), want_deq.float()) and bool(torch.isnan(out[:, K:]).all())


def test_plans():
    """Which route each tested shape takes: the native kernel up to its row limit wherever
    N % 128 == 0 and K % 128 == 0, split K on the long-K shapes, dequantise beyond."""
    L = torch.ops.bfly
    for N, K in SHAPES:
        for epi in (0, 2):
            assert all(L.gemm_w4_check(m, N, K, epi) == 0 for m in NATIVE_M), (N, K, epi)
    limit = max(m for m in (64, 128, 256, 512, 1024, 2048) if L.gemm_w4_check(m, 256, 256, 0) == 0)
    assert 64 <= limit < 1024                            # 1024 rows are the routed case of every test here
    assert L.gemm_w4_check(limit, 256, 256, 0) == 0 and L.gemm_w4_check(limit + 1, 256, 256, 0) != 0
    assert L.gemm_w4_check(16, 256, 192, 0) != 0 and L.gemm_w4_check(16, 192, 256, 0) != 0
    assert L.gemm_w4_check(16, 256, 256, 1) != 0       # no bias epilogue
    assert L.gemm_w4_check(0, 256, 256, 0) == 0
    assert all(L.gemm_w4_splitk(m, 256, 4096, 0) > 1 for m in NATIVE_M)
    assert L.gemm_w4_workspace_size(64, 256, 4096) == L.gemm_w4_splitk(64, 256, 4096, 0) * 64 * 256 * 4
    assert L.gemm_w4_splitk(1, 8192, 28672, 0) > 1     # 70B down projection at real size
    assert L.gemm_w4_workspace_size(1, 8192, 28672) == L.gemm_w4_splitk(1, 8192, 28672, 0) * 8192 * 4
    assert L.gemm_w4_splitk(16, 256, 192, 0) == 0 and L.gemm_w4_workspace_size(16, 256, 192) == 0
    # llama-tiny's projections
    assert L.gemm_w4_check(8, 1024, 256, 2) == 0 and L.gemm_w4_check(8, 256, 512, 0) == 0


@pytest.mark.parametrize("N,K", EXACT_SHAPES)
def test_exact(N, K, poisoned):
    g = torch.Generator(device="cpu").manual_seed(N * 7 + K)
    code = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.uint8)
    scale = torch.randint(127, 131, (N, K // 32), generator=g, dtype=torch.uint8)
    wd = ref.dequantize_mxfp4(code, scale, torch.float64).to(DEV)
    code, scale = code.to(DEV), scale.to(DEV)
    assert torch.equal(ops.dequantize_mxfp4(code, scale).double(), wd)
    for M in NATIVE_M + [200, 1024]:            # one 64-row tile, row-tiled native, dequantise route
        x = torch.randint(-2, 3, (M, K), generator=g).to(torch.bfloat16).to(DEV)
        assert (torch.ops.bfly.gemm_w4_check(M, N, K, 0) == 0) == (M != 1024)
        exact = x.double() @ wd.t()
        assert float(exact.abs().max()) * 2 < 2 ** 24
        y = ops.linear_w4(x, code, scale)
        want = exact.to(torch.bfloat16)
        assert y.shape == (M, N) and torch.equal(y, want), \
            f"M={M}: {int((y != want).sum())}/{y.numel()} outputs differ"


@pytest.mark.parametrize("epi", ["none", "silu"])
@pytest.mark.parametrize("N,K", SHAPES)
def test_linear_w4(N, K, epi, poisoned):
    w = _weight(N, K, seed=N + K)
    code, scale = ops.quantize_mxfp4(w)
    for M in NATIVE_M + ROUTED_M:
        x = _bf(M, K, seed=M)
        native = torch.ops.bfly.gemm_w4_check(M, N, K, EPI[epi]) == 0
        assert native or M > 64
        assert not native or M < 1024
        y = ops.linear_w4(x, code, scale, epilogue=epi)
        assert y.dtype == torch.bfloat16 and y.shape == (M, N // 2 if epi == "silu" else N)
        _close(y, ref.linear_w4(x, code, scale, epi), 2e-2, 2e-2)
        if M in (5, 200, 1024):
            out = torch.full_like(y, float("nan"))
            assert ops.linear_w4(x, code, scale, epilogue=epi, out=out) is out
            assert torch.equal(out, y)                 # the caller's buffer


def test_poisoned_arena(poisoned):
    """Neither route reads a slab or scratch element it has not written in the same call."""
    N, K = 256, 4096
    code, scale = ops.quantize_mxfp4(_weight(N, K, seed=2))
    for M in (16, 1024):
        x = _bf(M, K, seed=M)
        y = ops.linear_w4(x, code, scale)
        for name in ("gemm_w4", "w8_deq"):
            for key, buf in ops._arena.bufs.items():
                if key[1] == name and key[0].startswith("cuda"):
                    buf.fill_(float("nan"))
        assert torch.equal(ops.linear_w4(x, code, scale), y) and not torch.isnan(y.float()).any()


@pytest.mark.parametrize("M,N,K,epi", [(64, 57344, 8192, "silu"), (1, 8192, 28672, "none")])
def test_linear_w4_production(M, N, K, epi, poisoned):
    """Llama-3-70B gate/up and down at real size: index width and the full split-K grid."""
    g = torch.Generator(device=DEV).manual_seed(N)
    w = torch.randn(N, K, generator=g, device=DEV, dtype=torch.bfloat16)
    w *= (torch.logspace(-6, 6, N, base=2.0, device=DEV)[torch.randperm(N, generator=g, device=DEV)]
          / math.sqrt(K)).to(torch.bfloat16)[:, None]
    w.view(N, K // 32, 32).mul_(torch.logspace(-4, 4, K // 32, base=2.0, device=DEV)
                                [torch.randperm(K // 32, generator=g, device=DEV)].to(torch.bfloat16)[None, :, None])
    code, scale = ops.quantize_mxfp4(w)
    del w
    x = _bf(M, K, seed=5)
    assert torch.ops.bfly.gemm_w4_check(M, N, K, EPI[epi]) == 0
    y = ops.linear_w4(x, code, scale, epilogue=epi)
    wd = ops.dequantize_mxfp4(code, scale)           # bitwise the reference's (test_quantise_and_dequantise_kernels)
    _close(y, ref.linear(x, wd, None, epi), 2e-2, 2e-2)


def test_deterministic_and_graph_capture():
    N, K, M = 2048, 1024, 16
    code, scale = ops.quantize_mxfp4(_weight(N, K, seed=9))
    assert torch.ops.bfly.gemm_w4_splitk(M, N, K, 0) > 1       # the captured call uses the slabs
    x = _bf(M, K, seed=1)
    for epi in ("none", "silu"):
        assert torch.equal(ops.linear_w4(x, code, scale, epi), ops.linear_w4(x, code, scale, epi))
    ops.reserve_w8_workspace(DEV, M, [(N, K)], "mxfp4")
    out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.linear_w4(x, code, scale, out=out)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    frozen = ops._arena.frozen
    ops._arena.frozen = True                                   # any workspace growth raises
    try:
        with torch.cuda.graph(g):
            ops.linear_w4(x, code, scale, out=out)
    finally:
        ops._arena.frozen = frozen
    for seed in (2, 3):
        x.copy_(_bf(M, K, seed=seed))
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ops.linear_w4(x, code, scale))


def test_model_logits_match_dequantised_reference():
    cfg = ModelConfig.from_preset("llama-small")
    g = build_model(cfg, device="cuda", dtype=torch.bfloat16)
    g.init_random(seed=7)
    bf16_bytes = g.local_bytes()
    g.quantize_weights("mxfp4")
    assert g.local_bytes() < bf16_bytes and not g.defer_qkv and not g.defer_reduce and g.rowscale_rows == 0
    c = build_model(cfg, device="cpu", dtype=torch.float32)
    for k, v in g.p.items():
        if k in g.wscale:
            c.p[k].copy_(ref.dequantize_mxfp4(v.cpu(), g.wscale[k].cpu(), torch.float32))
        else:
            c.p[k].copy_(v.float().cpu())
    bs = 32
    prompts = [[3, 1, 4, 1, 5, 9, 2, 6] * 9, list(range(1, 40)), [7]]
    tables, slots, nxt = [], [], 0
    for p in prompts:
        nb = (len(p) + 8 + bs - 1) // bs
        tables.append(list(range(nxt, nxt + nb)))
        nxt += nb
        slots.append([tables[-1][j // bs] * bs + j % bs for j in range(len(p))])
    kg, kc = g.allocate_kv_cache(nxt + 1, bs), c.allocate_kv_cache(nxt + 1, bs)
    fb = make_prefill_batch(prompts, slots)
    lg, lc = g.forward(fb.to("cuda"), kg), c.forward(fb, kc)
    V = cfg.vocab_size
    e = _rel(lg[:, :V], lc[:, :V])
    print(f"prefill logits rel err {e:.4g}")
    assert e < 2e-2
    toks = [int(t) for t in lc[:, :V].argmax(-1)]
    pos = [len(p) for p in prompts]
    sl = [tables[i][pos[i] // bs] * bs + pos[i] % bs for i in range(len(prompts))]
    mb = max(len(t) for t in tables)
    db = make_decode_batch(toks, pos, sl, tables, mb, mb * bs)
    e = _rel(g.forward(db.to("cuda"), kg)[:, :V], c.forward(db, kc)[:, :V])
    print(f"decode logits rel err {e:.4g}")
    assert e < 3e-2


def test_engine_graphs_match_eager_and_sizing():
    cfg = ModelConfig.from_preset("llama-small")
    prompts = [[i + 1, 2 * i + 3, 5] * 7 for i in range(6)]
    outs = []
    for graphs in (False, True):
        ecfg = EngineConfig(max_batch=8, max_seq_len=256, kv_cache_tokens=4096, use_graphs=graphs,
                            graph_batch_sizes=[4, 8], seed=11, weight_dtype="mxfp4")
        eng = LLMEngine(cfg, engine_cfg=ecfg, device="cuda")
        assert eng.weight_dtype == "mxfp4" and eng.model.wscale and not eng.model.packed
        outs.append(eng.generate(prompts, SamplingParams(max_tokens=12, ignore_eos=True)))
        w4_bytes = eng.model.local_bytes()
    assert outs[0] == outs[1] and all(len(t) == 12 for t in outs[0])
    fp8 = LLMEngine(cfg, engine_cfg=EngineConfig(max_batch=8, max_seq_len=256, kv_cache_tokens=4096,
                                                 use_graphs=False, seed=11, weight_dtype="fp8"), device="cuda")
    assert fp8.weight_dtype == "fp8" and w4_bytes < fp8.model.local_bytes()
    sized = LLMEngine(cfg, engine_cfg=EngineConfig(max_batch=4, max_seq_len=128, kv_cache_tokens=None,
                                                   use_graphs=False, seed=11, weight_dtype="mxfp4"), device="cuda")
    assert sized.kv.num_blocks >= 4 * (128 // 32)
    assert len(sized.generate(prompts[:2], SamplingParams(max_tokens=4, ignore_eos=True))) == 2


# ---- refusals of the three bindings, in the manner of test_ops_refusals_gpu.py ---------------------
# (registered outside the CUDA block that test holds to its table; a valid call at zero rows
# returns in the launcher before any launch, so a missing check shows as "did not raise")
W4_TABLE = {
    "quant_mxfp4": [R(0, 64), A(0, 32, dtype=U8), A(0, 2, dtype=U8)],
    "dequant_mxfp4": [A(0, 32, dtype=U8, grow=None), A(0, 2, dtype=U8), R(0, 64, grow=0)],
    "gemm_w4": [R(0, 128), A(128, 64, dtype=U8, grow=None), A(128, 4, dtype=U8), R(0, 128, grow=0), 0, WS(), False, 0],
}
W4_SCALARS = [
    ("gemm_w4", "bias epilogue", {"epilogue": 1}),
    ("gemm_w4", "K % 32", {"x": R(0, 48), "code": A(128, 24, dtype=U8), "scale": A(128, 1, dtype=U8)}),
    ("quant_mxfp4", "K % 32", {"w": R(0, 48), "code": A(0, 24, dtype=U8), "scale": A(0, 1, dtype=U8)}),
    ("dequant_mxfp4", "K % 32", {"code": A(0, 24, dtype=U8), "scale": A(0, 1, dtype=U8), "out": R(0, 48)}),
]


def _names(op):
    return [a.name for a in getattr(torch.ops.bfly, op).default._schema.arguments]


def _call(op, values):
    return getattr(torch.ops.bfly, op)(*[v.make() if isinstance(v, A) else v for v in values])


def _cases():
    out = []
    for op, specs in W4_TABLE.items():
        for i in [i for i, v in enumerate(specs) if isinstance(v, A)]:
            for m in specs[i].mutations(only_tensor=False):
                out.append(pytest.param(op, i, m, id=f"{op}-arg{i}-{m}"))
    return out


def test_refusal_table_covers_the_w4_bindings():
    from pathlib import Path

    text = (Path(__file__).resolve().parent.parent / "csrc" / "bindings" / "ops.cpp").read_text()
    with_kernel = set(re.findall(r'm\.def\("(\w+)\((?:[^"]|"\s*")*",\s*&\w+\);', text))
    assert {op for op in with_kernel if "w4" in op or "mxfp4" in op} == set(W4_TABLE)
    assert WS().dtype == F32


@pytest.mark.parametrize("op", sorted(W4_TABLE))
def test_zero_row_call_is_accepted(op):
    _call(op, W4_TABLE[op])
    torch.cuda.synchronize()


@pytest.mark.parametrize("op,index,mutation", _cases())
def test_mutated_argument_is_refused(op, index, mutation):
    values = list(W4_TABLE[op])
    arg = _names(op)[index]
    values[index] = values[index].make(mutation)
    with pytest.raises(RuntimeError, match=re.escape(f"{op}: {arg} ")):
        _call(op, values)


@pytest.mark.parametrize("op,what,override", [pytest.param(*s, id=f"{s[0]}-{s[1].replace(' ', '_')}") for s in W4_SCALARS])
def test_refused_scalar(op, what, override):
    values, names = list(W4_TABLE[op]), _names(op)
    for name, v in override.items():
        values[names.index(name)] = v
    with pytest.raises(RuntimeError, match=re.escape(f"{op}: ")):
        _call(op, values)
