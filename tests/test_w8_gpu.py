"""FP8 e4m3 weight-only quantisation on one MI355X: the quantise / dequantise kernels and the
native decode GEMM (csrc/kernels/gemm_w8.hip) against ops/reference.py, the dequantise route,
graph capture, and the quantised model and engine end to end.

Weights are random normal / sqrt(K) with the rows multiplied by factors spread over 2^-6 .. 2^6:
with near-equal row scales a missing or mis-indexed scale would pass unnoticed."""
import math

import pytest
import torch

from butterfly_amd import ops
from butterfly_amd.config import EngineConfig, ModelConfig
from butterfly_amd.engine.batch import make_decode_batch, make_prefill_batch
from butterfly_amd.engine.engine import LLMEngine
from butterfly_amd.engine.sampler import SamplingParams
from butterfly_amd.models import build_model
from butterfly_amd.ops import reference as ref

from .test_w8_cpu import EXACT_SHAPES, exact_case

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [(256, 256), (1024, 256), (256, 512), (384, 640), (2048, 1024), (256, 4096)]
NATIVE_M = [1, 5, 16, 17, 33, 64]                  # one 64-row tile, ragged last 16-row tiles
ROUTED_M = [65, 128, 200, 256, 300, 1024]          # row-tiled native kernel to 256 rows, then dequantise
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


def _weight(N, K, seed, zero_row=None):
    g = torch.Generator(device="cpu").manual_seed(seed)
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    f = torch.logspace(-6, 6, N, base=2.0)[torch.randperm(N, generator=g)]
    w = (w * f[:, None]).to(torch.bfloat16)
    if zero_row is not None:
        w[zero_row] = 0
    return w.to(DEV)


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
def test_quantise_kernel(N, K, poisoned):
    w = _weight(N, K, seed=3, zero_row=N // 3)
    code, scale = ops.quantize_fp8(w)
    assert code.dtype == torch.float8_e4m3fn and code.is_cuda and scale.dtype == torch.float32
    rcode, rscale = ref.quantize_fp8(w.cpu())
    scale_c, q = scale.cpu(), code.cpu().float()
    torch.testing.assert_close(scale_c, rscale, rtol=1e-6, atol=0)
    assert scale_c[N // 3] == 1.0 and (q[N // 3] == 0).all()
    assert not torch.isnan(q).any()
    # against RNE of the GPU's own quotient: a fast-math reciprocal may flip exact ties only
    t = w.cpu().float() / scale_c[:, None]
    r = t.clamp(-448, 448).to(torch.float8_e4m3fn).float()
    off = q != r
    print(f"quantise [{N}, {K}]: {int(off.sum())} codes differ from RNE(w / scale), "
          f"{int((q != rcode.float()).sum())} from the reference codes")
    assert bool(((q - t).abs() <= (r - t).abs() * (1 + 1e-3)).all())
    deq = ops.dequantize_fp8(code, scale)
    assert deq.dtype == torch.bfloat16
    assert torch.equal(deq.cpu(), (q * scale_c[:, None]).to(torch.bfloat16))
    assert torch.equal(deq.cpu(), ref.dequantize_fp8(code.cpu(), scale_c, torch.bfloat16))


def test_plans():
    """Which route each tested shape takes: the native kernel up to its row limit (256) wherever
    N % 128 == 0 and K % 128 == 0, split K on the long-K shape, dequantise beyond."""
    L = torch.ops.bfly
    for N, K in SHAPES:
        for epi in (0, 2):
            assert all(L.gemm_w8_check(m, N, K, epi) == 0 for m in NATIVE_M), (N, K, epi)
    assert L.gemm_w8_check(256, 256, 256, 0) == 0 and L.gemm_w8_check(257, 256, 256, 0) != 0
    assert L.gemm_w8_check(16, 256, 192, 0) != 0 and L.gemm_w8_check(16, 192, 256, 0) != 0
    assert L.gemm_w8_check(16, 256, 256, 1) != 0       # no bias epilogue
    assert all(L.gemm_w8_splitk(m, 256, 4096, 0) > 1 for m in NATIVE_M)
    assert L.gemm_w8_workspace_size(64, 256, 4096) == L.gemm_w8_splitk(64, 256, 4096, 0) * 64 * 256 * 4
    assert L.gemm_w8_splitk(1, 8192, 28672, 0) > 1     # 70B down projection at real size
    # llama-tiny's projections
    assert L.gemm_w8_check(8, 1024, 256, 2) == 0 and L.gemm_w8_check(8, 256, 512, 0) == 0


@pytest.mark.parametrize("N,K", EXACT_SHAPES)
def test_exact(N, K, poisoned):
    """The K permutation and the row scale, bit for bit (test_w8_cpu.exact_case has the inputs):
    one 64-row tile, the row-tiled native kernel (200 rows) and the dequantise route (1024)."""
    code, scale, cases = exact_case(N, K)
    code, scale = code.to(DEV), scale.to(DEV)
    assert sorted(cases) == sorted(NATIVE_M + [200, 1024])
    for M, (x, want) in cases.items():
        assert (torch.ops.bfly.gemm_w8_check(M, N, K, 0) == 0) == (M != 1024)
        y = ops.linear_w8(x.to(DEV), code, scale)
        want = want.to(DEV)
        assert y.shape == (M, N) and torch.equal(y, want), \
            f"M={M}: {int((y != want).sum())}/{y.numel()} outputs differ"


@pytest.mark.parametrize("epi", ["none", "silu"])
@pytest.mark.parametrize("N,K", SHAPES)
def test_linear_w8(N, K, epi, poisoned):
    w = _weight(N, K, seed=N + K)
    code, scale = ops.quantize_fp8(w)
    for M in NATIVE_M + ROUTED_M:
        x = _bf(M, K, seed=M)
        native = torch.ops.bfly.gemm_w8_check(M, N, K, EPI[epi]) == 0
        assert native == (M <= 256)
        y = ops.linear_w8(x, code, scale, epilogue=epi)
        assert y.dtype == torch.bfloat16 and y.shape == (M, N // 2 if epi == "silu" else N)
        _close(y, ref.linear_w8(x, code, scale, epi), 2e-2, 2e-2)
        if M in (5, 200):
            out = torch.full_like(y, float("nan"))
            assert ops.linear_w8(x, code.view(torch.uint8), scale, epilogue=epi, out=out) is out
            assert torch.equal(out, y)                 # uint8-viewed codes, caller's buffer


@pytest.mark.parametrize("M,N,K,epi", [(64, 57344, 8192, "silu"), (1, 8192, 28672, "none")])
def test_linear_w8_production(M, N, K, epi, poisoned):
    """Llama-3-70B gate/up and down at real size: index width and the full split-K grid."""
    g = torch.Generator(device=DEV).manual_seed(N)
    w = torch.randn(N, K, generator=g, device=DEV, dtype=torch.bfloat16)
    w *= (torch.logspace(-6, 6, N, base=2.0, device=DEV)[torch.randperm(N, generator=g, device=DEV)]
          / math.sqrt(K)).to(torch.bfloat16)[:, None]
    code, scale = ops.quantize_fp8(w)
    del w
    x = _bf(M, K, seed=5)
    assert torch.ops.bfly.gemm_w8_check(M, N, K, EPI[epi]) == 0
    y = ops.linear_w8(x, code, scale, epilogue=epi)
    _close(y, ref.linear_w8(x, code, scale, epi), 2e-2, 2e-2)


def test_deterministic_and_graph_capture():
    N, K, M = 2048, 1024, 16
    code, scale = ops.quantize_fp8(_weight(N, K, seed=9))
    assert torch.ops.bfly.gemm_w8_splitk(M, N, K, 0) > 1       # the captured call uses the slabs
    x = _bf(M, K, seed=1)
    for epi in ("none", "silu"):
        assert torch.equal(ops.linear_w8(x, code, scale, epi), ops.linear_w8(x, code, scale, epi))
    ops.reserve_w8_workspace(DEV, M, [(N, K)])
    out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.linear_w8(x, code, scale, out=out)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    frozen = ops._arena.frozen
    ops._arena.frozen = True                                   # any workspace growth raises
    try:
        with torch.cuda.graph(g):
            ops.linear_w8(x, code, scale, out=out)
    finally:
        ops._arena.frozen = frozen
    for seed in (2, 3):
        x.copy_(_bf(M, K, seed=seed))
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ops.linear_w8(x, code, scale))


def test_model_logits_match_dequantised_reference():
    cfg = ModelConfig.from_preset("llama-small")
    g = build_model(cfg, device="cuda", dtype=torch.bfloat16)
    g.init_random(seed=7)
    bf16_bytes = g.local_bytes()
    g.quantize_weights("fp8")
    assert g.local_bytes() < bf16_bytes and not g.defer_qkv and not g.defer_reduce and g.rowscale_rows == 0
    c = build_model(cfg, device="cpu", dtype=torch.float32)
    for k, v in g.p.items():
        if k in g.wscale:
            c.p[k].copy_(ref.dequantize_fp8(v.cpu(), g.wscale[k].cpu(), torch.float32))
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
                            graph_batch_sizes=[4, 8], seed=11, weight_dtype="fp8")
        eng = LLMEngine(cfg, engine_cfg=ecfg, device="cuda")
        assert eng.weight_dtype == "fp8" and eng.model.wscale and not eng.model.packed
        outs.append(eng.generate(prompts, SamplingParams(max_tokens=12, ignore_eos=True)))
        fp8_bytes = eng.model.local_bytes()
    assert outs[0] == outs[1] and all(len(t) == 12 for t in outs[0])
    plain = LLMEngine(cfg, engine_cfg=EngineConfig(max_batch=8, max_seq_len=256, kv_cache_tokens=4096,
                                                   use_graphs=False, seed=11, weight_dtype="bf16"), device="cuda")
    assert plain.weight_dtype == "bf16" and fp8_bytes < plain.model.local_bytes()
    sized = LLMEngine(cfg, engine_cfg=EngineConfig(max_batch=4, max_seq_len=128, kv_cache_tokens=None,
                                                   use_graphs=False, seed=11, weight_dtype="fp8"), device="cuda")
    assert sized.kv.num_blocks >= 4 * (128 // 32)
    assert len(sized.generate(prompts[:2], SamplingParams(max_tokens=4, ignore_eos=True))) == 2
