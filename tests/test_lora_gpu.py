"""Multi-LoRA on the GPU: the shrink / expand kernels (csrc/kernels/lora.hip) against float64,
their refusals, and a bf16 model with adapters against the f32 CPU model.

Kernel checks
  exact      small-integer operands and power-of-two scales: every f32 sum is exact, so the result
             must EQUAL the float64 one (fragment layouts, seg indexing, slot stride, K-split
             reduce). Operands are random integers, hence asymmetric.
  tolerance  random bf16 operands, poisoned arena: |got - ref64| <= one bf16 ulp of ref64 +
             K * 2^-24 * sum|terms| (one final rounding plus worst-case f32 accumulation); rows
             without an adapter keep their bits.
Shapes are the smallest that cross every edge: T around the 16-row tile and more than one tile
with a ragged end, K = 256 and 224 (a multiple of 32 but not of the 64-element unrolled step),
N of 96 / 384 / 512 with all three seg layouts (3 x 128 for q | k | v, 2 x 256 interleaved for
gate | up), R = 8 (half an MFMA chunk of `a` rows) / 16 / 64, S = 3 and 17 (a tile of 16 distinct
adapters, dealt over the four workgroups of the tile).
"""
import re

import pytest
import torch

from butterfly_amd import ops

from .test_ops_refusals_gpu import F32, I32, U8, A, R as ROWS

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


@pytest.fixture(autouse=True, scope="module")
def _kernels_loaded():
    assert ops.load_library(), "butterfly_amd/_C.so not built or failed to load"


# ---- cases ---------------------------------------------------------------------------------------
TS = (1, 15, 16, 17, 65)
KS_ = (256, 224)
# (N, nseg, layout)
NS = ((96, 1, "one"), (384, 1, "one"), (384, 3, "qkv"), (512, 2, "gu"))
RS = (8, 16, 64)
SS = (3, 17)
PATTERNS = ("equal", "different", "alternating", "minus", "beyond", "tile_none")


def make_seg(N, nseg, layout):
    n = torch.arange(N)
    if layout == "one":
        return torch.zeros(N, dtype=torch.uint8)
    if layout == "qkv":
        return (n // (N // 3)).to(torch.uint8)
    assert layout == "gu" and nseg == 2
    return ((n // 16) % 2).to(torch.uint8)


def make_idx(pattern, T, S):
    i = torch.arange(T)
    if pattern == "equal":
        return torch.full((T,), S - 2, dtype=torch.int32)
    if pattern == "different":
        return (i * 7 % S).to(torch.int32)            # 7 is coprime to 3 and 17
    if pattern == "alternating":
        return ((i % 2) * (S - 1)).to(torch.int32)
    idx = (i * 7 % S).to(torch.int32)
    if pattern == "minus":
        idx[::3] = -1
    elif pattern == "beyond":
        idx[::4] = S
        idx[1::4] = 2 ** 30
        idx[2::8] = -(2 ** 31)
    else:
        idx[:16] = -1                                  # a whole tile without adapter (T > 16)
        idx[-1] = -1
    return idx


def ref64(y, x, a, b, seg, scale, idx):
    """(float64 result, sum of the absolute terms, valid rows) on the CPU."""
    y, x, a, b, scale = (t.detach().cpu().double() for t in (y, x, a, b, scale))
    seg, idx = seg.cpu().long(), idx.cpu().long()
    S, N, R = b.shape
    valid = (idx >= 0) & (idx < S)
    ic = idx.clamp(0, S - 1)
    cols = seg.view(N, 1) * R + torch.arange(R).view(1, R)
    out, mag, ts = y.clone(), y.abs(), torch.zeros(y.shape[0], a.shape[1], dtype=torch.float64)
    for m in range(y.shape[0]):
        if not valid[m]:
            continue
        s = ic[m]
        t, ta = a[s] @ x[m], a[s].abs() @ x[m].abs()                     # [J]
        ts[m] = t
        out[m] += scale[s] * (t[cols] * b[s]).sum(-1)
        mag[m] += scale[s].abs() * (ta[cols] * b[s].abs()).sum(-1)
    return out, mag, valid, ts


def operands(T, K, N, nseg, layout, R, S, exact, seed):
    g = torch.Generator().manual_seed(seed)
    J = nseg * R
    if exact:
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).to(BF)   # noqa: E731
        x, a, b, y = ri(-2, 2, T, K), ri(-2, 2, S, J, K), ri(-1, 1, S, N, R), ri(-8, 8, T, N)
        scale = torch.tensor([0.5, 1.0, 2.0, 0.25])[torch.arange(S) % 4]
    else:
        rn = lambda *s: torch.randn(*s, generator=g)                                # noqa: E731
        x, a, b, y = rn(T, K).to(BF), (rn(S, J, K) * 0.1).to(BF), (rn(S, N, R) * 0.3).to(BF), rn(T, N).to(BF)
        scale = torch.rand(S, generator=g) * 2 + 0.25
    return x, a, b, y, make_seg(N, nseg, layout), scale.float()


def all_cases(T):
    for K in KS_:
        for N, nseg, layout in NS:
            for R in RS:
                for S in SS:
                    for p in PATTERNS:
                        if p == "tile_none" and T <= 16:
                            continue
                        yield K, N, nseg, layout, R, S, p


def bf16_ulp(v):
    """One bf16 unit in the last place of |v| (float64 tensor), the smallest normal's for 0."""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126)))
    return torch.pow(2.0, e - 7)


@pytest.mark.parametrize("T", TS)
def test_exact(T):
    n = 0
    for K, N, nseg, layout, R, S, p in all_cases(T):
        x, a, b, y, seg, scale = operands(T, K, N, nseg, layout, R, S, True, seed=n)
        idx = make_idx(p, T, S)
        want, _, valid, tw = ref64(y, x, a, b, seg, scale, idx)
        # every sum is an exact f32 (integers and quarters below 2^24): float64 rounds to the same bf16
        want = want.to(BF)
        dx, da, db, dseg, dscale, didx = (t.to(DEV) for t in (x, a, b, seg, scale, idx))
        tag = f"T={T} K={K} N={N} {layout} R={R} S={S} {p}"
        for splitk in (0, 1, 3):
            got = ops.lora_add_(y.to(DEV), dx, da, db, dseg, dscale, didx, splitk=splitk)
            assert torch.equal(got.cpu(), want), f"{tag} splitk={splitk}"
        # the two ops on their own: t itself (no rounding at all), zero for rows without adapter
        t = ops.lora_shrink(dx, da, didx, splitk=2)
        assert torch.equal(t.cpu().double(), tw), tag
        got = ops.lora_expand_(y.to(DEV), t, db, dseg, dscale, didx)
        assert torch.equal(got.cpu(), want), tag
        n += 1
    assert n > 100


@pytest.mark.parametrize("T", TS)
def test_tolerance_and_untouched_rows(T):
    ops.set_poison(True)
    try:
        n = 0
        for K, N, nseg, layout, R, S, p in all_cases(T):
            x, a, b, y, seg, scale = operands(T, K, N, nseg, layout, R, S, False, seed=1000 + n)
            idx = make_idx(p, T, S)
            want, mag, valid, _ = ref64(y, x, a, b, seg, scale, idx)
            got = ops.lora_add_(y.to(DEV), *(t.to(DEV) for t in (x, a, b, seg, scale, idx))).cpu()
            bound = bf16_ulp(want) + K * 2.0 ** -24 * mag
            err = (got.double() - want).abs()
            tag = f"T={T} K={K} N={N} {layout} R={R} S={S} {p}"
            assert bool((err <= bound).all()), f"{tag}: max err / bound {(err / bound).max().item():.3g}"
            assert torch.equal(got[~valid].view(torch.int16), y[~valid].view(torch.int16)), tag
            if valid.any():
                assert not torch.equal(got[valid], y[valid]), tag
            n += 1
    finally:
        ops.set_poison(False)


def test_strided_output_rows_and_neighbouring_columns():
    T, K, N, R, S = 17, 256, 96, 16, 3
    x, a, b, y, seg, scale = operands(T, K, N, 1, "one", R, S, True, seed=5)
    idx = make_idx("minus", T, S)
    want = ref64(y, x, a, b, seg, scale, idx)[0].to(BF)
    wide = torch.full((T, N + 32), 7.0, dtype=BF, device=DEV)
    wide[:, 16:16 + N] = y.to(DEV)
    view = wide[:, 16:16 + N]
    ops.lora_add_(view, *(t.to(DEV) for t in (x, a, b, seg, scale, idx)))
    assert torch.equal(view.cpu(), want)
    assert bool((wide[:, :16] == 7).all()) and bool((wide[:, 16 + N:] == 7).all())


def test_launches_agree_bit_for_bit_and_graph_replay_equals_eager():
    T, K, N, R, S = 65, 256, 384, 16, 17
    x, a, b, y, seg, scale = operands(T, K, N, 3, "qkv", R, S, False, seed=77)
    idx = make_idx("minus", T, S)
    dev = [t.to(DEV) for t in (x, a, b, seg, scale, idx)]
    y0 = y.to(DEV)
    first = ops.lora_add_(y0.clone(), *dev)
    for _ in range(3):
        assert torch.equal(ops.lora_add_(y0.clone(), *dev), first)
    ybuf = y0.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.lora_add_(ybuf, *dev)
    for _ in range(2):
        ybuf.copy_(y0)
        graph.replay()
        assert torch.equal(ybuf, first)
    # the captured launches read idx when they run: another batch composition, same graph
    dev[5].copy_(make_idx("alternating", T, S))
    ybuf.copy_(y0)
    graph.replay()
    assert torch.equal(ybuf, ops.lora_add_(y0.clone(), *dev))
    assert not torch.equal(ybuf, first)


# ---- refusals of the two bindings, in the manner of tests/test_w4_gpu.py ---------------------------
LORA_TABLE = {
    "lora_shrink": [ROWS(0, 64), A(2, 16, 64, grow=2), A(0, dtype=I32), A(1, 0, 16, dtype=F32, grow=1)],
    "lora_expand": [ROWS(0, 64), A(1, 0, 16, dtype=F32, grow=1), A(2, 64, 8, grow=1), A(64, dtype=U8),
                    A(2, dtype=F32), A(0, dtype=I32)],
}
LORA_SCALARS = [
    ("lora_shrink", "K % 32", {"x": ROWS(0, 48), "a": A(2, 16, 48)}),
    ("lora_shrink", "J % 8", {"a": A(2, 12, 64), "part": A(1, 0, 12, dtype=F32)}),
    ("lora_shrink", "17 K splits", {"part": A(17, 0, 16, dtype=F32)}),
    ("lora_shrink", "no slot", {"a": A(0, 16, 64)}),
    ("lora_expand", "N % 16", {"y": ROWS(0, 40), "b": A(2, 40, 8), "seg": A(40, dtype=U8)}),
    ("lora_expand", "rank 12", {"b": A(2, 64, 12), "part": A(1, 0, 24, dtype=F32)}),
    ("lora_expand", "four rank slices", {"part": A(1, 0, 32, dtype=F32)}),
    ("lora_expand", "J % R", {"part": A(1, 0, 12, dtype=F32)}),
]


def _names(op):
    return [a.name for a in getattr(torch.ops.bfly, op).default._schema.arguments]


def _call(op, values):
    return getattr(torch.ops.bfly, op)(*[v.make() if isinstance(v, A) else v for v in values])


def _cases():
    out = []
    for op, specs in LORA_TABLE.items():
        for i in [i for i, v in enumerate(specs) if isinstance(v, A)]:
            for m in specs[i].mutations(only_tensor=False):
                out.append(pytest.param(op, i, m, id=f"{op}-arg{i}-{m}"))
    return out


@pytest.mark.parametrize("op", sorted(LORA_TABLE))
def test_zero_row_call_is_accepted(op):
    _call(op, LORA_TABLE[op])
    torch.cuda.synchronize()


@pytest.mark.parametrize("op,index,mutation", _cases())
def test_mutated_argument_is_refused(op, index, mutation):
    values = list(LORA_TABLE[op])
    arg = _names(op)[index]
    values[index] = values[index].make(mutation)
    with pytest.raises(RuntimeError, match=re.escape(f"{op}: {arg} ")):
        _call(op, values)


@pytest.mark.parametrize("op,what,override", [pytest.param(*s, id=f"{s[0]}-{s[1].replace(' ', '_')}") for s in LORA_SCALARS])
def test_refused_scalar(op, what, override):
    values, names = list(LORA_TABLE[op]), _names(op)
    for name, v in override.items():
        values[names.index(name)] = v
    with pytest.raises(RuntimeError, match=re.escape(f"{op}: ")):
        _call(op, values)


# ---- model and engine ----------------------------------------------------------------------------
def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm()).item()


def _forward_pair(model, prompts, lora, toks=None, dev="cpu", bs=32):
    """Prefill logits, then decode logits of `toks` (default: the prefill's greedy tokens)."""
    from butterfly_amd.engine.batch import make_decode_batch, make_prefill_batch

    from .test_lora_cpu import layout

    tables, slots, nb = layout(prompts)
    kv = model.allocate_kv_cache(nb, bs)
    fb = make_prefill_batch(prompts, slots)
    if lora is not None:
        fb.lora_idx = torch.tensor([s for p, s in zip(prompts, lora) for _ in p], dtype=torch.int32)
    V = model.cfg.vocab_size
    lp = model.forward(fb.to(dev), kv)[:, :V]
    toks = [int(t) for t in lp.argmax(-1)] if toks is None else toks
    pos = [len(p) for p in prompts]
    sl = [tables[i][pos[i] // bs] * bs + pos[i] % bs for i in range(len(prompts))]
    mb = max(len(t) for t in tables)
    db = make_decode_batch(toks, pos, sl, tables, mb, mb * bs)
    if lora is not None:
        db.lora_idx = torch.tensor(lora, dtype=torch.int32)
    return lp, model.forward(db.to(dev), kv)[:, :V], toks


def test_model_logits_match_the_f32_cpu_model():
    """llama-small bf16 with two adapters (ranks 16 and 8) on the kernels against the f32 CPU model
    holding the same weights and adapters: 2e-2 prefill / 3e-2 decode relative error, the bounds
    of test_w8_gpu.py::test_model_logits_match_dequantised_reference; the adapters move the
    logits by ten times those bounds at least."""
    from butterfly_amd.config import ModelConfig
    from butterfly_amd.models import build_model

    from .test_lora_cpu import make_adapter

    cfg = ModelConfig.from_preset("llama-small")
    g = build_model(cfg, device=DEV, dtype=BF)
    g.init_random(seed=7)
    c = build_model(cfg, device="cpu", dtype=torch.float32)
    for k, v in g.p.items():
        c.p[k].copy_(v.float().cpu())
    ads = [(make_adapter(cfg, 16, seed=1, amp=0.03), 2.0), (make_adapter(cfg, 8, seed=2, amp=0.03), 1.0)]
    ads = [({k: v.to(BF) for k, v in t.items()}, s) for t, s in ads]       # the values both models hold
    for m in (g, c):
        m.enable_lora(3, 16)
        for slot, (t, s) in zip((2, 0), ads):
            m.load_lora(slot, t, s)
    prompts = [[3, 1, 4, 1, 5, 9, 2, 6] * 9, list(range(1, 40)), [7], [11, 12, 13]]
    lora = [2, 0, -1, 2]
    want_p, want_d, toks = _forward_pair(c, prompts, lora)
    base_p, base_d, _ = _forward_pair(c, prompts, None, toks)
    got_p, got_d, _ = _forward_pair(g, prompts, lora, toks, dev=DEV)
    ep, ed = _rel(got_p, want_p), _rel(got_d, want_d)
    rows = [0, 1, 3]
    mp, md = _rel(want_p[rows], base_p[rows]), _rel(want_d[rows], base_d[rows])
    print(f"prefill rel err {ep:.4g} (adapters move the logits by {mp:.4g}); decode {ed:.4g} ({md:.4g})")
    assert ep < 2e-2 and ed < 3e-2
    assert mp >= 10 * 2e-2 and md >= 10 * 3e-2


def _engine(cfg, tmp_path, graphs, loras=2, **kw):
    from butterfly_amd.config import EngineConfig
    from butterfly_amd.engine.engine import LLMEngine

    ecfg = EngineConfig(max_batch=8, max_seq_len=256, kv_cache_tokens=4096, use_graphs=graphs, graph_batch_sizes=[4, 8],
                        seed=11, max_loras=loras, max_lora_rank=16, **kw)
    eng = LLMEngine(cfg, engine_cfg=ecfg, device=DEV)
    if loras:
        eng.load_lora("a", tmp_path / "a")
        eng.load_lora("b", tmp_path / "b")
    return eng


def test_engine_graphs_match_eager_on_a_mixed_batch_and_plain_steps_are_untouched(tmp_path):
    from butterfly_amd.ckpt import lora as lora_ckpt
    from butterfly_amd.config import ModelConfig
    from butterfly_amd.engine.sampler import SamplingParams

    from .test_lora_cpu import make_adapter

    cfg = ModelConfig.from_preset("llama-small")
    lora_ckpt.save_lora(tmp_path / "a", make_adapter(cfg, 16, seed=1, amp=0.03), rank=16, alpha=32.0)
    lora_ckpt.save_lora(tmp_path / "b", make_adapter(cfg, 8, seed=2, amp=0.03), rank=8, alpha=8.0)
    prompts = [[i + 1, 2 * i + 3, 5] * 7 for i in range(6)]
    names = ["a", None, "b", "a", None, "b"]

    def run(eng, names):
        rids = [eng.add_request(p, SamplingParams(max_tokens=12, ignore_eos=True, lora=nm, logprobs=0))
                for p, nm in zip(prompts, names)]
        while eng.has_unfinished():
            eng.step()
        return [(eng.requests[r].output, eng.requests[r].logprobs) for r in rids]

    eager = _engine(cfg, tmp_path, False)
    mixed_eager = run(eager, names)
    graphed = _engine(cfg, tmp_path, True)
    mixed_graph = run(graphed, names)
    assert [o for o, _ in mixed_graph] == [o for o, _ in mixed_eager] and all(len(o) == 12 for o, _ in mixed_graph)
    assert graphed.runner.lora_graphs and all(g.graph is not None for g in graphed.runner.lora_graphs.values())
    assert not graphed.runner.captured_buckets          # no plain decode step has run yet
    # a run without adapter requests on the LoRA-enabled engines is bitwise the max_loras = 0 run,
    # tokens and logprobs, and replays plain graphs only
    plain = run(_engine(cfg, tmp_path, True, loras=0), [None] * 6)
    n_lora_graphs = len(graphed.runner.lora_graphs)
    assert run(graphed, [None] * 6) == plain
    assert graphed.runner.captured_buckets and len(graphed.runner.lora_graphs) == n_lora_graphs
    # and the adapters change what is generated
    assert [o for o, _ in mixed_graph] != [o for o, _ in plain]
