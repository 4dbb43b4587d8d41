"""Qwen3 on one MI355X: the QK-norm variant of the RoPE + KV-append kernel (csrc/kernels/rope.hip,
QKNORM) against float64 from the same bf16 inputs, its bitwise facts, the split-K slab form, the
binding's refusals, graph capture, and the qwen3-tiny / cut qwen3-32b models end to end.

The kernel bound is derived, not measured. With x^_j = x_j * rsqrt(mean(x^2) + eps) * w_j in exact
arithmetic and the output o_j = x^_j c - x^_(j+D/2) s (or the other half's formula),

    |got - ref| <= 2^-8 |ref| + 2^-18 (|x^_j| + |x^_(j+-D/2)|)

The first term is the one rounding to bf16: half an ulp of an 8-bit significand, at most 2^-8 of
the value (reached just above a power of two). The second is the f32 evaluation in front of it,
which also pays for a value that it moves across a rounding boundary: v_rsq_f32 (1 ulp), the
16 + 3 additions of the sum of squares (it enters through the square root, so half its relative
error) and the two products come to fewer than 32 ulps of 2^-24 on each of the two terms of the
rotation, which may cancel: hence their magnitudes and not |ref|. The cos / sin tables are the
kernel's own f32 inputs. Zero mismatches are allowed."""
import dataclasses
import functools
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

from .test_ops_refusals_gpu import F32, I32, A

pytestmark = pytest.mark.gpu

DEV = "cuda"
BS, NBLK, MAX_POS, EPS = 32, 4, 4096, 1e-6
FP8 = torch.float8_e4m3fn
HEADS = [(5, 1, 128),      # 48 rotation + 16 V items: one wave holds both kinds of lane
         (4, 2, 128),
         (64, 8, 128),     # 576 + 128 items: three workgroups, a head group never straddles one
         (4, 2, 64)]       # 4 lanes per head


@pytest.fixture(autouse=True, scope="module")
def _kernels_loaded():
    assert ops.load_library(), "butterfly_amd/_C.so not built or failed to load"


def _bits(t):
    return t.view(torch.uint8) if t.element_size() == 1 else t.view(torch.int16)


def _poisoned(Hkv, D, fp8):
    """K and V caches filled with a byte pattern no result has in every element."""
    kc = torch.full((NBLK, Hkv, BS, D), 0x5A, dtype=torch.uint8, device=DEV)
    vc = torch.full((NBLK, Hkv, D, BS), 0x5A, dtype=torch.uint8, device=DEV)
    if fp8:
        return kc.view(FP8), vc.view(FP8)
    return (torch.full((NBLK, Hkv, BS, D), -7.0, dtype=torch.bfloat16, device=DEV),
            torch.full((NBLK, Hkv, D, BS), -7.0, dtype=torch.bfloat16, device=DEV))


@functools.lru_cache(maxsize=None)
def _inputs(T, Hq, Hkv, D):
    g = torch.Generator().manual_seed(1000 * T + Hq + D)
    qkv = (torch.randn(T, (Hq + 2 * Hkv) * D, generator=g) * 3.0).to(torch.bfloat16)
    qkv[0, :D] = 0                                    # a zero Q head and a zero K head
    qkv[T - 1, Hq * D:(Hq + 1) * D] = 0
    qw = (0.25 + 1.75 * torch.rand(D, generator=g)).to(torch.bfloat16)
    kw = (0.25 + 1.75 * torch.rand(D, generator=g)).to(torch.bfloat16)
    pos = torch.randint(0, MAX_POS, (T,), generator=g, dtype=torch.int32)
    pos[T - 1] = MAX_POS - 1
    slots = torch.randperm(NBLK * BS, generator=g)[:T].to(torch.int32)
    if T > 1:
        slots[1] = -1
    if T > 40:
        slots[40] = -5
    return qkv, qw, kw, pos, slots


@functools.lru_cache(maxsize=None)
def _tables(D):
    return ref.rope_tables(D, MAX_POS, 1e6, device=DEV)


@functools.lru_cache(maxsize=None)
def _run(T, Hq, Hkv, D, fp8):
    """One launch of the op and of the unchanged rope_kv on the same inputs; everything the tests compare."""
    qkv, qw, kw, pos, slots = (t.to(DEV) for t in _inputs(T, Hq, Hkv, D))
    cos, sin = _tables(D)
    out, (kc, vc) = qkv.clone(), _poisoned(Hkv, D, fp8)
    ops.rope_kv(out, pos, cos, sin, Hq, Hkv, slots, kc, vc, q_norm=qw, k_norm=kw, eps=EPS)
    again, (kc2, vc2) = qkv.clone(), _poisoned(Hkv, D, fp8)
    ops.rope_kv(again, pos, cos, sin, Hq, Hkv, slots, kc2, vc2, q_norm=qw, k_norm=kw, eps=EPS)
    plain, (kcp, vcp) = qkv.clone(), _poisoned(Hkv, D, fp8)
    ops.rope_kv(plain, pos, cos, sin, Hq, Hkv, slots, kcp, vcp)
    torch.cuda.synchronize()
    return dict(out=out.cpu(), kc=kc.cpu(), vc=vc.cpu(), again=again.cpu(), kc2=kc2.cpu(), vc2=vc2.cpu(),
                plain=plain.cpu(), vcp=vcp.cpu())


@functools.lru_cache(maxsize=None)
def _float64(T, Hq, Hkv, D):
    """(ref, slack): the rotated normalised heads in float64 and |x^_j| + |x^_(j+-D/2)|, [T, Hq + Hkv, D]."""
    qkv, qw, kw, pos, _ = _inputs(T, Hq, Hkv, D)
    cos, sin = (t.cpu().double() for t in _tables(D))
    x = qkv.double().view(T, Hq + 2 * Hkv, D)[:, : Hq + Hkv]
    w = torch.cat([qw.double().expand(Hq, D), kw.double().expand(Hkv, D)], 0)
    xh = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + EPS) * w
    c, s = cos[pos.long()].unsqueeze(1), sin[pos.long()].unsqueeze(1)
    a, b = xh[..., : D // 2], xh[..., D // 2:]
    want = torch.cat([a * c - b * s, b * c + a * s], -1)
    slack = (a.abs() + b.abs()).repeat(1, 1, 2)
    return want, slack


CASES = [pytest.param(T, *h, fp8, id=f"T{T}-{h[0]}x{h[1]}x{h[2]}-{'fp8' if fp8 else 'bf16'}")
         for T in (1, 3, 65) for h in HEADS for fp8 in (False, True)]


@pytest.mark.parametrize("T,Hq,Hkv,D,fp8", CASES)
def test_kernel_against_float64(T, Hq, Hkv, D, fp8):
    r = _run(T, Hq, Hkv, D, fp8)
    want, slack = _float64(T, Hq, Hkv, D)
    got = r["out"].double().view(T, Hq + 2 * Hkv, D)[:, : Hq + Hkv]
    err = (got - want).abs()
    tol = 2.0 ** -8 * want.abs() + 2.0 ** -18 * slack
    bad = int((~(err <= tol)).sum())
    print(f"max err / bound {float((err / tol.clamp_min(1e-300)).max()):.3f}, max |ref| {float(want.abs().max()):.3g}")
    assert bad == 0, f"{bad}/{err.numel()} outside the bound, worst ratio {float((err / tol.clamp_min(1e-300)).max()):.3f}"
    # the normalisation did something: the plain rotation of the same input is far from it
    assert float((r["plain"].double().view(T, -1, D)[:, : Hq + Hkv] - want).abs().max()) > 0.5
    # a zero head gives zeros
    assert bool((got[0, 0] == 0).all()) and bool((got[T - 1, Hq] == 0).all())


@pytest.mark.parametrize("T,Hq,Hkv,D,fp8", CASES)
def test_bitwise_facts(T, Hq, Hkv, D, fp8):
    r = _run(T, Hq, Hkv, D, fp8)
    qkv, _, _, _, slots = _inputs(T, Hq, Hkv, D)
    out = r["out"]
    vcols = slice((Hq + Hkv) * D, None)
    assert torch.equal(_bits(out[:, vcols]), _bits(qkv[:, vcols]))                 # V columns untouched
    assert torch.equal(_bits(r["vc"]), _bits(r["vcp"]))                            # V cache: what rope_kv writes
    for name in ("out", "kc", "vc"):                                               # two launches, equal bits
        other = {"out": "again", "kc": "kc2", "vc": "vc2"}[name]
        assert torch.equal(_bits(r[name]), _bits(r[other])), name
    k_out = out[:, Hq * D:(Hq + Hkv) * D].view(T, Hkv, D)
    want_kc, want_vc = (_bits(t.cpu()).clone() for t in _poisoned(Hkv, D, fp8))
    cached = (lambda x: _bits(x.contiguous().to(FP8))) if fp8 else (lambda x: _bits(x.contiguous()))
    rotated_uncached = 0
    for t in range(T):
        sl = int(slots[t])
        if sl < 0:                                                                 # rotated, not cached
            rotated_uncached += int(not torch.equal(_bits(out[t, : (Hq + Hkv) * D]), _bits(qkv[t, : (Hq + Hkv) * D])))
            continue
        want_kc[sl // BS, :, sl % BS, :] = cached(k_out[t])                        # the op's own K output
        want_vc[sl // BS, :, :, sl % BS] = cached(out[t, vcols].view(Hkv, D))
    assert rotated_uncached == int((slots < 0).sum())
    assert torch.equal(_bits(r["kc"]), want_kc)               # named slots hold K; every other slot its poison
    assert torch.equal(_bits(r["vc"]), want_vc)


@pytest.mark.parametrize("sk", [1, 3, 16])
@pytest.mark.parametrize("T,Hq,Hkv,D,fp8", [(3, 5, 1, 128, False), (2, 64, 8, 128, True), (65, 4, 2, 64, False),
                                           (1, 4, 2, 128, True)])
def test_splitk_slabs_equal_reduce_then_plain_variant(sk, T, Hq, Hkv, D, fp8):
    _, qw, kw, pos, slots = (t.to(DEV) for t in _inputs(T, Hq, Hkv, D))
    cos, sin = _tables(D)
    g = torch.Generator().manual_seed(sk)
    row = (Hq + 2 * Hkv) * D
    slabs = (torch.randn(sk, T, row, generator=g) * 2.0).to(DEV)
    fused = torch.full((T, row), float("nan"), dtype=torch.bfloat16, device=DEV)
    kc, vc = _poisoned(Hkv, D, fp8)
    got = ops.rope_kv(ops.Partial(slabs, fused), pos, cos, sin, Hq, Hkv, slots, kc, vc, q_norm=qw, k_norm=kw, eps=EPS)
    assert got is fused
    two = ops.Partial(slabs, torch.empty_like(fused)).materialize()
    kc2, vc2 = _poisoned(Hkv, D, fp8)
    ops.rope_kv(two, pos, cos, sin, Hq, Hkv, slots, kc2, vc2, q_norm=qw, k_norm=kw, eps=EPS)
    torch.cuda.synchronize()
    assert torch.equal(_bits(fused), _bits(two))
    assert torch.equal(_bits(kc), _bits(kc2)) and torch.equal(_bits(vc), _bits(vc2))


def test_graph_replay_equals_eager():
    T, Hq, Hkv, D = 65, 64, 8, 128
    qkv, qw, kw, pos, slots = (t.to(DEV) for t in _inputs(T, Hq, Hkv, D))
    cos, sin = _tables(D)
    eager = _run(T, Hq, Hkv, D, False)
    buf, (kc, vc) = qkv.clone(), _poisoned(Hkv, D, False)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.rope_kv(buf, pos, cos, sin, Hq, Hkv, slots, kc, vc, q_norm=qw, k_norm=kw, eps=EPS)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.rope_kv(buf, pos, cos, sin, Hq, Hkv, slots, kc, vc, q_norm=qw, k_norm=kw, eps=EPS)
    for _ in range(2):
        buf.copy_(qkv)
        pk, pv = _poisoned(Hkv, D, False)
        kc.copy_(pk)
        vc.copy_(pv)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(buf.cpu()), _bits(eager["out"]))
        assert torch.equal(_bits(kc.cpu()), _bits(eager["kc"])) and torch.equal(_bits(vc.cpu()), _bits(eager["vc"]))


# ---- refusals of the binding, in the manner of test_w4_gpu.py -------------------------------------
# (a catch-all registration outside the CUDA block that test_ops_refusals_gpu.py holds to its table;
# a valid call at zero rows returns in the launcher before any launch)
RD = 64
QK_TABLE = {
    "rope_qknorm_kv": [A(0, 4 * RD, grow=None), A(0, dtype=I32), A(16, RD // 2, dtype=F32, grow=None),
                       A(16, RD // 2, dtype=F32), 2, 1, A(0, dtype=I32), A(2, 1, 32, RD, grow=None), A(2, 1, RD, 32),
                       A(RD), A(RD), 1e-6, A(1, 0, 4 * RD, dtype=F32, grow=1)],
}
QK_SCALARS = [
    ("rope_qknorm_kv", "negative eps", {"eps": -1.0}),
    ("rope_qknorm_kv", "nan eps", {"eps": float("nan")}),
    ("rope_qknorm_kv", "heads do not divide the row", {"num_q_heads": 3}),
    ("rope_qknorm_kv", "head_dim 32", {"num_q_heads": 6}),
    ("rope_qknorm_kv", "negative heads", {"num_q_heads": -2, "num_kv_heads": 3}),
]


def _names(op):
    return [a.name for a in getattr(torch.ops.bfly, op).default._schema.arguments]


def _call(op, values):
    return getattr(torch.ops.bfly, op)(*[v.make() if isinstance(v, A) else v for v in values])


def _refusal_cases():
    out = []
    for op, specs in QK_TABLE.items():
        for i in [i for i, v in enumerate(specs) if isinstance(v, A)]:
            for m in specs[i].mutations(only_tensor=False):
                out.append(pytest.param(op, i, m, id=f"{op}-arg{i}-{m}"))
    return out


def test_refusal_table_covers_every_tensor_argument():
    schema = torch.ops.bfly.rope_qknorm_kv.default._schema
    tensors = [i for i, a in enumerate(schema.arguments) if "Tensor" in str(a.type)]
    assert tensors == [i for i, v in enumerate(QK_TABLE["rope_qknorm_kv"]) if isinstance(v, A)] and len(tensors) == 10
    plain = [a.name for a in torch.ops.bfly.rope_kv.default._schema.arguments]
    assert [n for n in _names("rope_qknorm_kv") if n not in ("q_norm_w", "k_norm_w", "eps")] == plain


def test_zero_row_call_is_accepted():
    _call("rope_qknorm_kv", QK_TABLE["rope_qknorm_kv"])
    torch.cuda.synchronize()


@pytest.mark.parametrize("op,index,mutation", _refusal_cases())
def test_mutated_argument_is_refused(op, index, mutation):
    values = list(QK_TABLE[op])
    arg = _names(op)[index]
    values[index] = values[index].make(mutation)
    with pytest.raises(RuntimeError, match=re.escape(f"{op}: {arg} ")):
        _call(op, values)


@pytest.mark.parametrize("op,what,override", [pytest.param(*s, id=s[1].replace(" ", "_")) for s in QK_SCALARS])
def test_refused_scalar(op, what, override):
    values, names = list(QK_TABLE[op]), _names(op)
    for name, v in override.items():
        values[names.index(name)] = v
    with pytest.raises(RuntimeError, match=re.escape(f"{op}: ")):
        _call(op, values)


# ---- models ---------------------------------------------------------------------------------------
def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm()).item()


def _set_qk(model, make, seed=1):
    g = torch.Generator().manual_seed(seed)
    for i in model.layer_ids:
        for which in ("q", "k"):
            model.p[f"l{i}.{which}_norm_w"].copy_(make(model.cfg.head_dim, g))


def _tiny_gpu():
    cfg = ModelConfig.from_preset("qwen3-tiny")
    g = build_model(cfg, device="cuda", dtype=torch.bfloat16)
    g.init_random(seed=7)
    _set_qk(g, lambda D, gen: 1 + 0.5 * torch.randn(D, generator=gen))
    return cfg, g


def test_tiny_prefill_and_decode_logits_match_cpu_reference():
    """The bounds of tests/test_engine_gpu.py::test_prefill_and_decode_logits_match_reference."""
    cfg, g = _tiny_gpu()
    assert g.defer_qkv
    c = build_model(cfg, device="cpu", dtype=torch.float32)
    for k, v in g.p.items():
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


def test_tiny_engine_graphs_match_eager():
    prompts = [[i + 1, 2 * i + 3, 5] * 7 for i in range(6)]
    outs = []
    for graphs in (False, True):
        cfg, g = _tiny_gpu()
        ecfg = EngineConfig(max_batch=8, max_seq_len=256, kv_cache_tokens=4096, use_graphs=graphs,
                            graph_batch_sizes=[4, 8], seed=11)
        eng = LLMEngine(cfg, engine_cfg=ecfg, device="cuda", model=g)
        outs.append(eng.generate(prompts, SamplingParams(max_tokens=12, ignore_eos=True)))
    assert outs[0] == outs[1] and all(len(o) == 12 for o in outs[0])


def test_qwen3_32b_width_prefill_decode_and_graph():
    """qwen3-32b cut to 2 layers (K = 5120 projections, the 151936-row LM head), in the manner of
    tests/test_fullsize_gpu.py and at its bounds for the dense presets."""
    cfg = dataclasses.replace(ModelConfig.from_preset("qwen3-32b"), num_layers=2)
    g = build_model(cfg, device="cuda", dtype=torch.bfloat16)
    g.init_random(seed=5)
    _set_qk(g, lambda D, gen: 0.25 + 1.75 * torch.rand(D, generator=gen))
    with ops.reference_mode():
        r = build_model(cfg, device="cuda", dtype=torch.float32)
    for k, v in g.p.items():
        r.p[k].copy_(v.float())
    V, B, P, bs = cfg.vocab_size, 4, 64, 32
    gen = torch.Generator().manual_seed(3)
    prompts = [torch.randint(0, V, (P,), generator=gen).tolist() for _ in range(B)]
    nb = (P + 1 + bs - 1) // bs + 1
    tables = [list(range(i * nb, (i + 1) * nb)) for i in range(B)]
    slots = [[tables[i][j // bs] * bs + j % bs for j in range(P)] for i in range(B)]
    kg = g.allocate_kv_cache(B * nb + 1, bs)
    with ops.reference_mode():
        kr = r.allocate_kv_cache(B * nb + 1, bs)
    fb = make_prefill_batch(prompts, slots).to("cuda")
    assert fb.num_tokens == 256
    lg = g.forward(fb, kg)
    with ops.reference_mode():
        lr = r.forward(fb, kr)
    e = _rel(lg[:, :V], lr[:, :V])
    print(f"prefill logits rel err {e:.4g}")
    assert e < 2e-2

    Bd = 3
    toks = [int(t) for t in lr[:Bd, :V].argmax(-1)]
    sl = [tables[i][P // bs] * bs + P % bs for i in range(Bd)]
    db = make_decode_batch(toks, [P] * Bd, sl, tables[:Bd], nb, nb * bs).to("cuda")
    snapshot = [(k.clone(), v.clone()) for k, v in kg]
    dg = g.forward(db, kg)
    kv_eager = [(k.clone(), v.clone()) for k, v in kg]
    with ops.reference_mode():
        dr = r.forward(db, kr)
    e = _rel(dg[:, :V], dr[:, :V])
    print(f"decode logits rel err {e:.4g}")
    assert e < 3e-2

    def restore():
        for (k, v), (k0, v0) in zip(kg, snapshot):
            k.copy_(k0)
            v.copy_(v0)

    restore()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            g.forward(db, kg)
    torch.cuda.current_stream().wait_stream(s)
    restore()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = g.forward(db, kg)
    for _ in range(2):
        restore()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, dg), "graph replay differs from eager"
        for (k, v), (k1, v1) in zip(kg, kv_eager):
            assert torch.equal(k, k1) and torch.equal(v, v1)
