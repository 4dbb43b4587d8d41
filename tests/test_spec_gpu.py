"""Speculative decoding on one MI355X: the multi-query verify attention kernel
(csrc/kernels/attention_verify.hip) on inputs whose correct output names the keys that were read
(tests/attn_cases.py through tests/spec_cases.py; tests/test_spec_cpu.py proves the cases sharp),
its binding's refusals, a verify batch through the model against the fp32 CPU model, and the
speculative engine against the non-speculative one.

Each kernel test prints its worst error as a fraction of the tolerance ("SPEC-FIGURE ...",
pytest -s / -rP) before it asserts."""
import re

import pytest
import torch

from butterfly_amd import ops
from butterfly_amd.config import EngineConfig, ModelConfig
from butterfly_amd.engine.batch import ForwardBatch, make_prefill_batch
from butterfly_amd.engine.engine import LLMEngine
from butterfly_amd.engine.sampler import SamplingParams

from . import attn_cases as ac
from . import spec_cases as sc
from .test_engine_gpu import _pair, _rel
from .test_ops_refusals_gpu import F32, I32, KC, VC, WS, A, R

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True, scope="module")
def _kernels_loaded():
    assert ops.load_library(), "butterfly_amd/_C.so not built or failed to load"


def _run_verify(c, QN, part_tokens=sc.PART, out=None):
    v = sc.verify_inputs(c, QN)
    got = ops.attn_verify(v["q"].to(DEV), c.kc.to(DEV), c.vc.to(DEV), c.tables.to(DEV), v["ctx_lens"].to(DEV),
                          v["q_lens"].to(DEV), ac.SCALE, v["max_ctx"], part_tokens, out=out)
    return v, got


def _check(label, mis, got, want):
    bad, worst = mis(got, want)
    print(f"SPEC-FIGURE {label}: worst err/tol {worst:.4f}, {bad} mismatches of {want.numel()}")
    assert bad == 0, f"{label}: {bad}/{want.numel()} mismatches, worst err/tol {worst:.3g}"


@pytest.mark.parametrize("kind,Hq,Hkv,QN,fp8", list(sc.sweep()))
def test_attn_verify_position_sweep(kind, Hq, Hkv, QN, fp8):
    """QN = 2 / 3 / 5 / 8 rows per sequence with G = 2 / 4 / 8 / 1: 1 .. 4 column tiles, the last
    one partly filled; ragged q_len (padding rows must give the last valid row's output), prefixes
    on both sides of page and split edges, a short sequence beside a long one, forced 64-token
    splits, bf16 and FP8 caches, a poisoned output buffer and poison in every slot that must not
    be read."""
    c = sc.case(kind, Hq, Hkv, QN, fp8)
    want = ac.reference_paged(c, emulate=True)[0]
    B = len(c.chunks)
    out = torch.full((B, QN, Hq, ac.D), float("nan"), dtype=torch.bfloat16, device=DEV)
    v, got = _run_verify(c, QN, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert sc.tiles(Hq, Hkv, QN) == torch.ops.bfly.attn_verify_tiles(QN, Hq // Hkv)
    _check(f"verify {kind} Hq={Hq} Hkv={Hkv} QN={QN} tiles={sc.tiles(Hq, Hkv, QN)} {'fp8' if fp8 else 'bf16'}",
           ac.mismatches_for(kind), got.cpu(), want[v["src"]])


@pytest.mark.parametrize("fp8", [False, True])
def test_attn_verify_default_split_and_single_split(fp8):
    """The split size the launcher picks itself (one split at these lengths: the kernel writes
    the output directly) and one split forced over everything agree with the reference too."""
    c = sc.case("needle", 8, 1, 5, fp8)
    want = ac.reference_paged(c, emulate=True)[0]
    for part in (0, 4096):
        v, got = _run_verify(c, 5, part_tokens=part)
        _check(f"verify needle part={part} {'fp8' if fp8 else 'bf16'}", ac.needle_mismatches, got.cpu(), want[v["src"]])


def test_attn_verify_is_deterministic_and_captures_into_a_graph():
    c = sc.case("needle", 8, 2, 5, False)
    v, first = _run_verify(c, 5)
    _, second = _run_verify(c, 5)
    assert torch.equal(first, second)
    args = [t.to(DEV) for t in (v["q"], c.kc, c.vc, c.tables, v["ctx_lens"], v["q_lens"])]
    out = torch.empty_like(first)
    frozen, ops._arena.frozen = ops._arena.frozen, True       # the warm calls above sized the partials
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ops.attn_verify(*args, ac.SCALE, v["max_ctx"], sc.PART, out=out)
    finally:
        ops._arena.frozen = frozen
    out.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, first)


@pytest.mark.parametrize("fp8", [False, True])
def test_attn_verify_single_rows_agree_with_attn_decode(fp8):
    """Sequences with q_len = 1 inside a QN = 3 call against ops.attn_decode on the same query
    and context, by the needle criterion."""
    c = sc.case("needle", 8, 2, 3, fp8)
    v, got = _run_verify(c, 3)
    ones = [b for b, (_, ql) in enumerate(c.chunks) if ql == 1]
    assert ones
    ix = torch.tensor(ones)
    dec = ops.attn_decode(v["q"][ix, 0].to(DEV), c.kc.to(DEV), c.vc.to(DEV), c.tables[ix].to(DEV),
                          v["ctx_lens"][ix].to(DEV), ac.SCALE, v["max_ctx"], sc.PART)
    for t in range(3):      # the padding rows of such a sequence repeat row 0
        _check(f"verify q_len=1 row {t} vs decode {'fp8' if fp8 else 'bf16'}", ac.needle_mismatches,
               got[ix, t].cpu(), dec.cpu().double())


# ---- binding refusals, in the manner of the W4_TABLE block of tests/test_w4_gpu.py --------------------
# (registered outside the CUDA block tests/test_ops_refusals_gpu.py holds to its table; a valid call
# at zero sequences returns in the launcher before any launch)
VERIFY_TABLE = {
    "attn_verify": [R(0, 2, 2, 128), KC(), VC(), R(1, 4, dtype=I32), A(2, dtype=I32, grow=None),
                    A(2, dtype=I32, grow=None), 0.1, 64, 32, A(0, 2, 2, 128), WS(), WS()],
}
VERIFY_SCALARS = [
    ("block table too narrow", {"max_ctx": 128}),
    ("part_tokens % 32", {"part_tokens": 48}),
    ("QN * G > 64", {"q": R(0, 5, 16, 128), "out": A(0, 5, 16, 128)}),
    ("head_dim 64", {"q": R(0, 2, 2, 64), "k_cache": A(2, 1, 32, 64), "v_cache": A(2, 1, 64, 32), "out": A(0, 2, 2, 64)}),
    ("no partials", {"part_o": None, "part_ml": None}),
]


def _names(op):
    return [a.name for a in getattr(torch.ops.bfly, op).default._schema.arguments]


def _call(op, values):
    return getattr(torch.ops.bfly, op)(*[v.make() if isinstance(v, A) else v for v in values])


def _cases():
    out = []
    for op, specs in VERIFY_TABLE.items():
        for i in [i for i, v in enumerate(specs) if isinstance(v, A)]:
            for m in specs[i].mutations(only_tensor=False):
                out.append(pytest.param(op, i, m, id=f"{op}-arg{i}-{m}"))
    return out


def test_zero_row_call_is_accepted():
    assert WS().dtype == F32
    _call("attn_verify", VERIFY_TABLE["attn_verify"])
    torch.cuda.synchronize()


@pytest.mark.parametrize("op,index,mutation", _cases())
def test_mutated_argument_is_refused(op, index, mutation):
    values = list(VERIFY_TABLE[op])
    arg = _names(op)[index]
    values[index] = values[index].make(mutation)
    with pytest.raises(RuntimeError, match=re.escape(f"{op}: {arg} ")):
        _call(op, values)


@pytest.mark.parametrize("what,override", [pytest.param(*s, id=s[0].replace(" ", "_")) for s in VERIFY_SCALARS])
def test_refused_scalar(what, override):
    values, names = list(VERIFY_TABLE["attn_verify"]), _names("attn_verify")
    for name, v in override.items():
        values[names.index(name)] = v
    with pytest.raises(RuntimeError, match=re.escape("attn_verify: ")):
        _call("attn_verify", values)


# ---- model level ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kv_dtype", [torch.bfloat16, torch.float8_e4m3fn])
def test_verify_batch_through_the_model_matches_reference(kv_dtype):
    """Three sequences prefilled, then ONE verify batch of QN = 4 rows each (drafts of 3, 0 and
    2 tokens: ragged, one sequence at q_len = 1) through model.forward on the HIP kernels, bf16
    and FP8 KV cache, against the fp32 CPU model on the same batch and the same cache element
    type (with FP8 also the same cached codes; measured 0.021 with bf16, and for FP8 0.108
    against an unrounded reference cache and 0.066 against e4m3 codes rounded from the fp32
    model's own K/V: the format's error, not the kernels'): _rel < 5e-2 over the valid
    rows, the bound of test_mixed_chunked_step_matches_reference (one bf16 model pass vs fp32)."""
    cfg, g, c = _pair("llama-small")
    bs, V, QN = 32, cfg.vocab_size, 4
    prompts = [[(7 * j) % 3000 + 1 for j in range(61)], [(11 * j) % 3000 + 2 for j in range(20)], [5, 9, 2] * 11]
    drafts = [[17, 23, 4], [], [8, 1]]
    tables, slots, nxt = [], [], 0
    for p in prompts:
        nb = (len(p) + QN + bs - 1) // bs + 1
        tables.append(list(range(nxt, nxt + nb)))
        nxt += nb
        slots.append([tables[-1][j // bs] * bs + j % bs for j in range(len(p) + QN)])
    # FP8: the CPU model's cache holds e4m3 too and, after the prefill, the very codes the GPU
    # model wrote, so both sides of the verify step read the same cached K/V and the figure
    # measures the kernels, not the format (a code that differs is a 6-12 % element error; e4m3
    # against unrounded K/V alone moves decode logits by up to 0.1,
    # test_fp8_kv_decode_logits_close_to_bf16)
    fp8 = kv_dtype == torch.float8_e4m3fn
    kg = g.allocate_kv_cache(nxt + 1, bs, kv_dtype)
    kc = c.allocate_kv_cache(nxt + 1, bs, kv_dtype if fp8 else None)
    fb = make_prefill_batch(prompts, [s[:len(p)] for s, p in zip(slots, prompts)])
    lc = c.forward(fb, kc)
    g.forward(fb.to(DEV), kg)
    if fp8:
        for (kk, vv), (gk, gv) in zip(kc, kg):
            kk.copy_(gk.cpu())
            vv.copy_(gv.cpu())
    first = [int(t) for t in lc[:, :V].argmax(-1)]
    ids, pos, sl, valid = [], [], [], []
    for i, (p, d) in enumerate(zip(prompts, drafts)):
        row = [first[i]] + d
        for t in range(QN):
            u = min(t, len(d))
            ids.append(row[u])
            pos.append(len(p) + u)
            sl.append(slots[i][len(p) + t] if t <= len(d) else -1)
            valid.append(t <= len(d))
    i32 = lambda a: torch.tensor(a, dtype=torch.int32)  # noqa: E731
    mb = max(len(t) for t in tables)
    bt = torch.zeros(len(prompts), mb, dtype=torch.int32)
    for i, t in enumerate(tables):
        bt[i, :len(t)] = i32(t)
    vb = ForwardBatch(input_ids=i32(ids), positions=i32(pos), slots=i32(sl), is_prefill=False, block_tables=bt,
                      ctx_lens=i32([len(p) + 1 for p in prompts]), max_ctx=mb * bs - (QN - 1), logits_idx=None,
                      q_rows=QN, q_lens=i32([1 + len(d) for d in drafts]))
    lg, lr = g.forward(vb.to(DEV), kg), c.forward(vb, kc)
    keep = torch.tensor(valid)
    e = _rel(lg[:, :V][keep.to(DEV)], lr[:, :V][keep])
    print(f"SPEC-FIGURE verify batch logits rel err {e:.4g} ({kv_dtype})")
    assert e < 5e-2
    # padding rows repeat the last valid row: same inputs, same keys, same logits
    rows = lg.view(len(prompts), QN, -1)
    assert _rel(rows[1, 1], rows[1, 0]) < 2e-3 and _rel(rows[2, 3], rows[2, 2]) < 2e-3


# ---- engine level -----------------------------------------------------------------------------------
class _Oracle:
    """Proposes what the non-speculative run generated."""

    def __init__(self, prompts, outs):
        self.full = [list(p) + list(o) for p, o in zip(prompts, outs)]
        self.plen = [len(p) for p in prompts]

    def propose(self, tokens, k):
        for full, n in zip(self.full, self.plen):
            if len(tokens) >= n and tokens == full[:len(tokens)]:
                return full[len(tokens):len(tokens) + k]
        return []


def _slack(model, kv_blocks, prompts, outs, V):
    """Teacher-force prompt + output through one plain prefill: max over generated positions of
    (largest logit - the logit of the token that was generated)."""
    bs = 32
    seqs = [list(p) + list(o) for p, o in zip(prompts, outs)]
    slots, nxt = [], 0
    for s in seqs:
        nb = (len(s) + bs - 1) // bs
        slots.append([nxt * bs + j for j in range(len(s))])
        nxt += nb
    assert nxt <= kv_blocks
    kv = model.allocate_kv_cache(kv_blocks, bs)
    fb = make_prefill_batch(seqs, slots)
    fb.logits_idx = None
    lg = model.forward(fb.to(DEV), kv)[:, :V].float()
    worst, at, top = 0.0, 0, 0.0
    for s, p, o in zip(seqs, prompts, outs):
        rows = lg[at + len(p) - 1: at + len(s) - 1]
        tok = torch.tensor(o, device=DEV)
        worst = max(worst, float((rows.max(-1).values - rows.gather(1, tok[:, None])[:, 0]).max()))
        top = max(top, float(rows.abs().max()))
        at += len(s)
    return worst, top


def test_speculative_engine_against_the_plain_engine():
    """llama-small, greedy, 6 requests to max_tokens: the spec_tokens = 0 engine (hipGraph decode
    steps), then the speculative engine with the oracle proposer (every draft right as long as
    the two runs agree) and with the default prompt-lookup proposer. Token equality across kernel
    paths is not required on bf16 logits; instead every run is teacher-forced through one plain
    prefill and its slack = max_i (max logit_i - logit_i[token_i]) is taken: 0 when every token
    is the prefill path's argmax, positive where the path that generated it (graph decode, or
    verify) rounded a near-tie the other way. The speculative runs' slack may exceed the plain
    run's by at most MARGIN = 8 bf16 steps at the largest logit magnitude seen (8 * 2^-8 * max
    |logit|): the decode and the verify path differ from the prefill path by rounding of the
    same kind (bf16 activations between kernels, bf16 P in attention, split order), a few steps
    of the bf16 logits each, so neither may pick a token that the prefill path ranks further
    below its best than that. Also: all requests finish at max_tokens, the counters are
    consistent, and every KV block is free again."""
    cfg = ModelConfig.from_preset("llama-small")
    V, N = cfg.vocab_size, 24
    prompts = [[(3 * i + 5 * j) % 50 + 1 for j in range(12 + 9 * i)] + [7, 8, 9, 7, 8] for i in range(6)]
    base = dict(max_batch=8, max_seq_len=256, kv_cache_tokens=4096, graph_batch_sizes=[8], seed=11)
    plain = LLMEngine(cfg, engine_cfg=EngineConfig(**base), device=DEV)
    ref_out = plain.generate(prompts, SamplingParams(max_tokens=N, ignore_eos=True))
    assert all(len(o) == N for o in ref_out)
    s0, top = _slack(plain.model, 64, prompts, ref_out, V)
    margin = 8 * 2.0 ** -8 * top
    print(f"SPEC-FIGURE engine slack plain {s0:.4g}, max |logit| {top:.4g}, margin {margin:.4g}")
    for name in ("oracle", "ngram"):
        eng = LLMEngine(cfg, engine_cfg=EngineConfig(spec_tokens=3, **base), device=DEV)     # same seed, same weights
        if name == "oracle":
            eng.proposer = _Oracle(prompts, ref_out)
        kinds = []
        rids = [eng.add_request(p, SamplingParams(max_tokens=N, ignore_eos=True)) for p in prompts]
        while eng.has_unfinished():
            kinds.append(eng.step().kind)
        outs = [eng.requests[r].output for r in rids]
        cnt = eng.metrics.counters
        s1, _ = _slack(plain.model, 64, prompts, outs, V)
        same = sum(a == b for a, b in zip(outs, ref_out))
        print(f"SPEC-FIGURE engine {name}: slack {s1:.4g} (plain {s0:.4g}), {same}/6 outputs equal, "
              f"{int(cnt['spec_verify_steps'])} verify steps, {int(cnt['spec_draft_tokens'])} drafted, "
              f"{int(cnt['spec_accepted_tokens'])} accepted, {len(kinds)} steps")
        assert all(len(o) == N and eng.requests[r].finish_reason == "length" for o, r in zip(outs, rids))
        # (prompt lookup on a random-init model: its output rarely repeats the context, so the
        # default proposer may find no draft at all and every step is then a plain decode step)
        assert name != "oracle" or (cnt["spec_verify_steps"] >= 1 and "verify" in kinds)
        assert 0 <= cnt["spec_accepted_tokens"] <= cnt["spec_draft_tokens"]
        assert cnt["tokens_verify"] == cnt["spec_verify_sequences"] + cnt["spec_accepted_tokens"]
        assert eng.kv.manager.num_free == eng.kv.manager.num_blocks and eng.kv.manager.num_seqs == 0
        assert s1 <= s0 + margin
        if name == "oracle":
            assert cnt["spec_accepted_tokens"] > 0
