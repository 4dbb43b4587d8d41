"""Speculative decoding on the CPU reference path: the engine with n-gram (or any) drafts emits
exactly what the spec_tokens = 0 engine emits, for greedy and seeded sampling alike, with the
bookkeeping (KV slots, lengths, counters, finish rules) right; the proposer, the reference
verify attention, KVBlockManager.truncate, the refusals and the command-line / HTTP surface;
and the attn_verify cases the GPU file runs are sharp (tests/spec_cases.py)."""
import json
import os
import shutil
import subprocess
import threading

import pytest
import torch

from butterfly_amd import _native_loader
from butterfly_amd.config import EngineConfig, ModelConfig
from butterfly_amd.engine.engine import LLMEngine
from butterfly_amd.engine.sampler import SamplingParams
from butterfly_amd.engine.spec import NgramProposer, accepted_prefix
from butterfly_amd.ops import reference as ref
from butterfly_amd.parallel.mesh import Mesh

from . import attn_cases as ac
from . import spec_cases as sc
from .spec_cases import OracleProposer, RandomProposer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 3
MARGIN = 1e-4
# repetitive prompts (the n-gram lookup finds matches) of ragged lengths
PROMPTS = [[(5 * i + 3 * (j % (4 + i))) % 200 + 1 for j in range(n)] for i, n in enumerate((45, 7, 20, 33, 5, 12))]


def _ecfg(**kw):
    base = dict(max_batch=4, max_seq_len=128, kv_cache_tokens=1024, use_graphs=False, seed=5)
    base.update(kw)
    return EngineConfig(**base)


def _params(sampling, i, n, **kw):
    if sampling == "greedy":
        return SamplingParams(max_tokens=n, ignore_eos=True, logprobs=2, **kw)
    # seeded temperature rows, some with a top-k, some with a top-p filter
    return SamplingParams(max_tokens=n, ignore_eos=True, logprobs=2, temperature=0.9, seed=17 + i,
                          top_k=(0, 6, 0)[i % 3], top_p=(1.0, 1.0, 0.85)[i % 3], **kw)


def _drive(eng, prompts, params, late=None, check=None):
    """Run the requests to the end -> (request objects, step outputs). `late`: (step index,
    prompts, params) added once that many steps ran; `check(eng)` runs after every step."""
    rids = [eng.add_request(p, q) for p, q in zip(prompts, params)]
    steps = []
    while eng.has_unfinished():
        if late is not None and len(steps) == late[0]:
            rids += [eng.add_request(p, q) for p, q in zip(late[1], late[2])]
            late = None
        steps.append(eng.step())
        if check is not None:
            check(eng)
    assert late is None
    return [eng.requests[r] for r in rids], steps


def _assert_margins(reqs):
    """The precondition of every equality below, from the non-speculative run alone: at every
    generated position the two most likely tokens are at least MARGIN apart in log-probability,
    so an fp32 reordering (one more row in a GEMM, per-row attention) cannot swap them."""
    for q in reqs:
        assert len(q.logprobs) == len(q.output)
        for _, top in q.logprobs:
            assert len(top) == 2 and top[0][1] - top[1][1] >= MARGIN, top


def _assert_same(reqs, want, what):
    for a, b in zip(reqs, want):
        assert a.output == b.output, f"{what}: request {a.rid}"
        assert a.finish_reason == b.finish_reason
        assert len(a.logprobs) == len(b.logprobs) == len(a.output)
        for (la, ta), (lb, tb) in zip(a.logprobs, b.logprobs):
            assert abs(la - lb) <= 1e-5 and [t for t, _ in ta] == [t for t, _ in tb]
            assert all(abs(x - y) <= 1e-5 for (_, x), (_, y) in zip(ta, tb))


def _all_free(eng):
    m = eng.kv.manager
    return m.num_free == m.num_blocks and m.num_seqs == 0


def _proposer(name, cfg, prompts, outs):
    if name == "ngram":
        return None                      # the engine's default
    oracle = OracleProposer(prompts, outs)
    if name == "oracle":
        return oracle
    if name == "wrong":
        return OracleProposer(prompts, outs, wrong=True, vocab=cfg.vocab_size)
    return RandomProposer(oracle, cfg.vocab_size, seed=3)


# ---- losslessness ---------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", ["greedy", "seeded"])
@pytest.mark.parametrize("preset", ["llama-tiny", "qwen3-tiny", "mixtral-tiny", "gpt2-tiny"])
def test_speculative_outputs_equal_the_plain_engine(preset, sampling):
    cfg = ModelConfig.from_preset(preset)
    n = 14
    params = [_params(sampling, i, n) for i in range(len(PROMPTS))]
    plain = LLMEngine(cfg, engine_cfg=_ecfg(), device="cpu")
    assert plain.spec_k == 0 and plain.proposer is None
    want, steps = _drive(plain, PROMPTS, params)
    assert "verify" not in {s.kind for s in steps}
    _assert_margins(want)
    outs = [q.output for q in want]
    for name in ("ngram", "oracle", "wrong", "random"):
        eng = LLMEngine(cfg, engine_cfg=_ecfg(spec_tokens=K), device="cpu")
        assert eng.spec_k == K and not eng.async_pp and isinstance(eng.proposer, NgramProposer)
        prop = _proposer(name, cfg, PROMPTS, outs)
        if prop is not None:
            eng.proposer = prop
        got, steps = _drive(eng, PROMPTS, params)
        _assert_same(got, want, f"{preset} {sampling} {name}")
        c = eng.metrics.counters
        assert _all_free(eng) and c["spec_accepted_tokens"] <= c["spec_draft_tokens"]
        if name != "ngram":
            assert c["spec_verify_steps"] >= 1 and "verify" in {s.kind for s in steps}
        if name == "oracle":
            assert c["spec_accepted_tokens"] == c["spec_draft_tokens"] > 0
        if name == "wrong":
            assert c["spec_accepted_tokens"] == 0 < c["spec_draft_tokens"]


# ---- bookkeeping ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["oracle", "wrong"])
def test_bookkeeping_tokens_per_step_lengths_and_counters(name):
    cfg = ModelConfig.from_preset("llama-tiny")
    n = 1 + 3 * (K + 1)          # the prefill's token, then whole verify steps: no draft is clamped
    params = [SamplingParams(max_tokens=n, ignore_eos=True) for _ in PROMPTS]
    want, _ = _drive(LLMEngine(cfg, engine_cfg=_ecfg(), device="cpu"), PROMPTS, params)
    eng = LLMEngine(cfg, engine_cfg=_ecfg(spec_tokens=K), device="cpu")
    eng.proposer = _proposer(name, cfg, PROMPTS, [q.output for q in want])

    def check(e):
        for r in e.scheduler.running():
            q = e.requests[r]
            if q.n_gen >= 1:
                assert e.kv.manager.length(r) == len(q.prompt) + q.n_gen - 1

    got, steps = _drive(eng, PROMPTS, params, check=check)
    assert [q.output for q in got] == [q.output for q in want]
    per = K + 1 if name == "oracle" else 1
    verify = [s for s in steps if s.kind == "verify"]
    assert verify
    for s in verify:
        assert len(s.rids) == len(s.new_tokens)
        assert all(s.rids.count(r) == per for r in set(s.rids))       # a request once per emitted token
        assert s.rids == sorted(s.rids, key=s.rids.index)              # and its tokens in one run, in order
    c = eng.metrics.counters
    emitted = sum(len(s.new_tokens) for s in verify)
    assert c["spec_verify_steps"] == len(verify)
    assert c["spec_accepted_tokens"] <= c["spec_draft_tokens"]
    assert emitted == c["tokens_verify"] == c["spec_verify_sequences"] + c["spec_accepted_tokens"]
    assert c["spec_accepted_tokens"] == (c["spec_draft_tokens"] if name == "oracle" else 0)
    assert _all_free(eng)


# ---- stops ----------------------------------------------------------------------------------------
def _stop_case(want):
    """(request index, output index j, token): a token first seen at output index j that lies
    inside a verify step's accepted run (indices 1 .. K + 1 are the first step's: j = 2 or 3)."""
    for i, q in enumerate(want):
        for j in (2, 3):
            if q.output[j] not in q.output[:j]:
                return i, j, q.output[j]
    raise AssertionError("no request has a fresh token at output index 2 or 3")


@pytest.mark.parametrize("how", ["stop_token", "eos"])
def test_stop_inside_an_accepted_run_cuts_there(how):
    cfg = ModelConfig.from_preset("llama-tiny")
    free = [SamplingParams(max_tokens=12, ignore_eos=True) for _ in PROMPTS]
    full, _ = _drive(LLMEngine(cfg, engine_cfg=_ecfg(), device="cpu"), PROMPTS, free)
    i, j, tok = _stop_case(full)
    if how == "stop_token":
        params = [SamplingParams(max_tokens=12, stop_token_ids=[tok]) for _ in PROMPTS]
        kw = {}
    else:
        params = [SamplingParams(max_tokens=12) for _ in PROMPTS]
        kw = dict(eos_token_id=tok)
    want, _ = _drive(LLMEngine(cfg, engine_cfg=_ecfg(), device="cpu", **kw), PROMPTS, params)
    assert want[i].output == full[i].output[:j + 1] and want[i].finish_reason == "stop"
    eng = LLMEngine(cfg, engine_cfg=_ecfg(spec_tokens=K), device="cpu", **kw)
    eng.proposer = OracleProposer(PROMPTS, [q.output for q in full])      # drafts run past the stop
    got, steps = _drive(eng, PROMPTS, params)
    assert [q.output for q in got] == [q.output for q in want]
    assert [q.finish_reason for q in got] == [q.finish_reason for q in want]
    assert got[i].finish_reason == "stop" and len(got[i].output) == j + 1
    hit = [s for s in steps if s.kind == "verify" and got[i].rid in s.finished]
    assert hit and hit[0].rids.count(got[i].rid) == j             # tokens 1 .. j of the run, nothing after
    assert _all_free(eng)


def test_max_tokens_is_reached_exactly_and_drafts_respect_the_clamps():
    cfg = ModelConfig.from_preset("llama-tiny")
    lens = (7, 2, 9, 5, 1, 6)
    params = [SamplingParams(max_tokens=n, ignore_eos=True) for n in lens]
    # the longest request ends exactly at max_seq_len
    msl = max(len(p) + n for p, n in zip(PROMPTS, lens))
    want, _ = _drive(LLMEngine(cfg, engine_cfg=_ecfg(max_seq_len=msl), device="cpu"), PROMPTS, params)
    eng = LLMEngine(cfg, engine_cfg=_ecfg(spec_tokens=K, max_seq_len=msl), device="cpu")
    prop = eng.proposer = OracleProposer(PROMPTS, [q.output for q in want], extra=5)   # offers more than asked
    got, steps = _drive(eng, PROMPTS, params)
    assert [q.output for q in got] == [q.output for q in want]
    assert all(len(q.output) == n and q.finish_reason == "length" for q, n in zip(got, lens))
    assert prop.calls and all(1 <= k <= K for _, k in prop.calls)
    by_len = {len(p): n for p, n in zip(PROMPTS, lens)}
    for ntok, k in prop.calls:        # k <= max_tokens - n_gen - 1 and <= max_seq_len - len(tokens) - 1
        plen = max(pl for pl in by_len if pl <= ntok and ntok - pl < by_len[pl])
        assert k <= by_len[plen] - (ntok - plen) - 1 and k <= msl - ntok - 1
    c = eng.metrics.counters
    assert c["spec_draft_tokens"] <= K * c["spec_verify_sequences"]
    assert _all_free(eng)


def test_row_budget_falls_back_to_the_decode_step():
    cfg = ModelConfig.from_preset("llama-tiny")
    params = [SamplingParams(max_tokens=8, ignore_eos=True) for _ in PROMPTS]
    want, _ = _drive(LLMEngine(cfg, engine_cfg=_ecfg(), device="cpu"), PROMPTS, params)
    eng = LLMEngine(cfg, engine_cfg=_ecfg(spec_tokens=K, spec_max_rows=4 * (K + 1) - 1), device="cpu")
    eng.proposer = OracleProposer(PROMPTS, [q.output for q in want])
    got, steps = _drive(eng, PROMPTS, params)
    assert [q.output for q in got] == [q.output for q in want]
    # four sequences with full drafts need 4 (K + 1) rows: those steps are plain decode steps
    # (the oracle's drafts are all accepted, so a request's tokens in a step are its rows)
    verify = [s for s in steps if s.kind == "verify"]
    assert verify and all(len(set(s.rids)) * max(s.rids.count(r) for r in s.rids) <= 4 * (K + 1) - 1 for s in verify)
    assert "decode" in {s.kind for s in steps}


# ---- coexistence ----------------------------------------------------------------------------------
def test_preemption_under_a_tight_cache():
    cfg = ModelConfig.from_preset("llama-tiny")
    prompts = [[(i + 1) * 7 % 90 + 1, 3, 4] * 10 for i in range(3)]
    params = [SamplingParams(max_tokens=20, ignore_eos=True, logprobs=2) for _ in prompts]
    # 4 pages of 32 tokens for 3 sequences of 50: forces preemption and recompute
    tight = dict(max_batch=3, kv_cache_tokens=128)
    plain = LLMEngine(cfg, engine_cfg=_ecfg(**tight), device="cpu")
    want, _ = _drive(plain, prompts, params)
    assert plain.metrics.counters["preempted_sequences"] > 0
    _assert_margins(want)
    for name in ("ngram", "oracle"):
        eng = LLMEngine(cfg, engine_cfg=_ecfg(spec_tokens=K, **tight), device="cpu")
        if name == "oracle":
            eng.proposer = OracleProposer(prompts, [q.output for q in want])
        got, steps = _drive(eng, prompts, params)
        _assert_same(got, want, f"preemption {name}")
        assert eng.metrics.counters["preempted_sequences"] > 0 and _all_free(eng)
        assert "verify" in {s.kind for s in steps}


def test_late_arrival_mixed_steps_and_prefix_cache_hits():
    cfg = ModelConfig.from_preset("llama-tiny")
    shared = [(13 * j) % 150 + 1 for j in range(70)]
    first, second = PROMPTS[:3], [shared + [5, 6], shared + [9], PROMPTS[3]]
    mk = lambda ps: [SamplingParams(max_tokens=10, ignore_eos=True, logprobs=2) for _ in ps]  # noqa: E731
    cfgs = dict(max_batch=6, max_seq_len=160, max_prefill_tokens=48, kv_cache_tokens=2048)
    runs = {}
    for spec in (0, K):
        eng = LLMEngine(cfg, engine_cfg=_ecfg(spec_tokens=spec, **cfgs), device="cpu")
        warm, _ = _drive(eng, [shared + [1]], mk([0]))           # registers the shared prefix pages
        if spec:
            eng.proposer = OracleProposer([shared + [1]] + first + second, runs[0][0])
        reqs, steps = _drive(eng, first, mk(first), late=(3, second, mk(second)))
        kinds = {s.kind for s in steps}
        assert "mixed" in kinds and eng.scheduler.prefix_hit_tokens >= 64 and _all_free(eng)
        if spec:
            assert "verify" in kinds
        runs[spec] = ([q.output for q in warm + reqs], warm + reqs)
    _assert_margins(runs[0][1])
    _assert_same(runs[K][1], runs[0][1], "late arrival")


def test_penalised_and_lora_requests_share_the_batch(tmp_path):
    from butterfly_amd.ckpt import lora as lora_ckpt

    from .test_lora_cpu import make_adapter

    cfg = ModelConfig.from_preset("llama-tiny")
    lora_ckpt.save_lora(tmp_path / "a", make_adapter(cfg, 8, seed=11), rank=8, alpha=16.0)
    extra = [dict(), dict(lora="a"), dict(presence_penalty=0.5, repetition_penalty=1.3), dict(lora="a"),
             dict(frequency_penalty=0.7), dict()]
    params = [SamplingParams(max_tokens=12, ignore_eos=True, logprobs=2, **kw) for kw in extra]
    runs = {}
    for spec in (0, K):
        eng = LLMEngine(cfg, engine_cfg=_ecfg(spec_tokens=spec, max_batch=6, max_loras=1, max_lora_rank=8), device="cpu")
        eng.load_lora("a", tmp_path / "a")
        if spec:
            oracle, asked = OracleProposer(PROMPTS, [q.output for q in runs[0]]), []

            class Recording:
                def propose(self, tokens, k):
                    asked.append(list(tokens))
                    return oracle.propose(tokens, k)

            eng.proposer = Recording()
        runs[spec], steps = _drive(eng, PROMPTS, params)
        assert _all_free(eng)
    _assert_margins(runs[0])
    _assert_same(runs[K], runs[0], "penalties + LoRA")
    assert "verify" in {s.kind for s in steps}
    # penalised requests carry no draft: the proposer is never asked about them
    penalised = [p for p, kw in zip(PROMPTS, extra) if kw and "lora" not in kw]
    assert asked and not any(t[:len(p)] == p for t in asked for p in penalised)
    assert runs[K][1].output != [q.output for q in runs[0]][0]        # the adapter rows ran their adapter


def _dp_gen(mesh, comm, prompts, params, spec, outs=None):
    cfg = ModelConfig.from_preset("llama-tiny")
    eng = LLMEngine(cfg, mesh, _ecfg(spec_tokens=spec), comm=comm, device="cpu")
    if outs is not None:
        eng.proposer = OracleProposer(prompts, outs)
    reqs, steps = _drive(eng, prompts, params)
    return [q.output for q in reqs], {s.kind for s in steps}, _all_free(eng)


def test_dp2_loopback_run():
    from butterfly_amd.parallel.fake import FakeWorld

    torch.set_num_threads(1)
    mesh = Mesh(dp=2)
    halves = [PROMPTS[:3], PROMPTS[3:]]
    params = [SamplingParams(max_tokens=10, ignore_eos=True) for _ in range(3)]
    want = [_dp_gen(Mesh(), None, h, params, 0)[0] for h in halves]
    world = FakeWorld(mesh, timeout_s=60)
    outs = world.run(lambda r, c: _dp_gen(mesh, c, halves[mesh.coord(r).dp], params, K, want[mesh.coord(r).dp]))
    for r, (got, kinds, free) in enumerate(outs):
        assert got == want[mesh.coord(r).dp] and "verify" in kinds and free


# ---- the proposer, the reference attention, truncate, refusals ------------------------------------------
def test_ngram_proposer_definition():
    p = NgramProposer(4, 2)
    #              0  1  2  3  4  5  6  7  8  9 10 11
    t = [1, 2, 3, 9, 1, 2, 3, 8, 7, 1, 2, 3]
    assert p.propose(t, 3) == [8, 7, 1]                   # latest earlier "1 2 3" (at 4), not the first (at 0)
    assert p.propose(t, 1) == [8] and p.propose(t, 0) == []
    assert p.propose(t, 20) == [8, 7, 1, 2, 3]            # up to k: what follows it, to the end
    # longest n first: "5 1 2 3" occurs once earlier, followed by 6; the 3-gram's latest match gives 8
    u = [5, 1, 2, 3, 6, 0, 1, 2, 3, 8, 5, 1, 2, 3]
    assert p.propose(u, 2) == [6, 0]
    assert NgramProposer(3, 2).propose(u, 2) == [8, 5]
    assert NgramProposer(1, 1).propose([4, 5, 4], 2) == [5, 4]
    assert p.propose([1, 2, 3, 4, 5, 6], 3) == []         # no match, no draft
    assert p.propose([7, 7], 3) == [] and p.propose([7, 7, 7], 3) == [7]   # the match must have a token after it
    assert NgramProposer(4, 3).propose([1, 2, 9, 1, 2], 3) == []           # only a 2-gram matches: below ngram_min
    for bad in ((2, 3), (4, 0)):
        with pytest.raises(ValueError, match="spec_ngram_min"):
            NgramProposer(*bad)
    assert accepted_prefix([4, 5, 6], [4, 5, 7, 9]) == 2 and accepted_prefix([], [3]) == 0
    assert accepted_prefix([4], [4, 1]) == 1 and accepted_prefix([4, 5], [3, 5, 6]) == 0


@pytest.mark.parametrize("fp8", [False, True])
def test_reference_attn_verify_equals_per_row_decode(fp8):
    c = sc.case("needle", 8, 2, 5, fp8)
    v = sc.verify_inputs(c, 5)
    got = ref.attn_verify(v["q"], c.kc, c.vc, c.tables, v["ctx_lens"], v["q_lens"], ac.SCALE, v["max_ctx"])
    assert got.shape == v["q"].shape
    for b, (pre, ql) in enumerate(c.chunks):
        for t in range(5):
            lim = torch.tensor([pre + 1 + min(t, ql - 1)])
            row = ref.attn_decode(v["q"][b:b + 1, t], c.kc, c.vc, c.tables[b:b + 1], lim, ac.SCALE)
            assert torch.equal(got[b, t], row[0])
    out = torch.empty_like(got)
    assert ref.attn_verify(v["q"], c.kc, c.vc, c.tables, v["ctx_lens"], v["q_lens"], ac.SCALE, out=out) is out
    assert torch.equal(out, got)


def test_truncate_through_the_binding():
    kv = _native_loader.native().KVBlockManager(8, 4)
    kv.allocate(1, 6)
    kv.extend(1, 7)
    assert kv.length(1) == 13 and kv.num_free == 4
    table = kv.block_table(1)
    kv.truncate(1, 9)
    assert kv.length(1) == 9 and kv.num_free == 5 and kv.block_table(1) == table[:3]
    kv.truncate(sid=1, new_len=8)
    assert kv.num_free == 6 and kv.block_table(1) == table[:2]
    for bad in (9, -1):
        with pytest.raises(ValueError):
            kv.truncate(1, bad)
    assert kv.length(1) == 8
    with pytest.raises(IndexError):
        kv.truncate(7, 0)
    kv.fork(1, 2)
    kv.truncate(2, 3)                       # shared pages only lose the child's reference
    assert kv.num_free == 6 and kv.block_table(1) == table[:2] and kv.block_table(2) == table[:1]
    kv.free(1)
    assert kv.num_free == 7
    kv.free(2)
    assert kv.num_free == 8
    # registered prompt pages stay registered through a truncate above the prompt
    toks = list(range(1, 10))
    hs = kv.block_hashes(toks)
    kv.allocate(3, 9)
    kv.register_blocks(3, hs)
    kv.append_slot(3)
    kv.extend(3, 6)
    kv.truncate(3, 10)
    assert kv.num_cached_blocks == 2 and kv.match_prefix(hs, 2) == 2 and kv.num_free == 5
    kv.free(3)
    assert kv.num_free == 8 and kv.match_prefix(hs, 2) == 2


def test_kv_cache_truncate_wrapper():
    eng = LLMEngine(ModelConfig.from_preset("llama-tiny"), engine_cfg=_ecfg(), device="cpu")
    eng.kv.manager.allocate(5, 40)
    eng.kv.truncate(5, 33)
    assert eng.kv.manager.length(5) == 33 and len(eng.kv.manager.block_table(5)) == 2
    eng.kv.truncate(5, 32)
    assert len(eng.kv.manager.block_table(5)) == 1


@pytest.mark.parametrize("mesh_kw,ecfg_kw,match", [
    (dict(tp=2), dict(), "tp = pp = ep = 1"),
    (dict(pp=2), dict(), "tp = pp = ep = 1"),
    (dict(dp=2, ep=2), dict(), "tp = pp = ep = 1"),
    (dict(dp=2), dict(cp_prefill_min_tokens=32), "context-parallel"),
    (dict(), dict(spec_ngram_min=0), "spec_ngram_min"),
    (dict(), dict(spec_ngram_min=5, spec_ngram_max=4), "spec_ngram_min"),
    (dict(), dict(spec_tokens=-1), "spec_tokens"),
    (dict(), dict(spec_max_rows=-2), "spec_max_rows"),
    (dict(), dict(spec_ngram_max=-1), "spec_ngram_max"),
    (dict(), dict(spec_tokens=32), r"\(spec_tokens \+ 1\) \* \(heads / kv heads\)"),
])
def test_refusals_at_engine_construction(mesh_kw, ecfg_kw, match):
    cfg = ModelConfig.from_preset("mixtral-tiny" if "ep" in mesh_kw else "llama-tiny")
    kw = dict(spec_tokens=K)
    kw.update(ecfg_kw)
    with pytest.raises(ValueError, match=match):
        LLMEngine._check_spec(cfg, Mesh(**mesh_kw), _ecfg(**kw), "cpu")
    if not mesh_kw:
        with pytest.raises(ValueError, match=match):
            LLMEngine(cfg, engine_cfg=_ecfg(**kw), device="cpu")


def test_head_dim_refusal_is_for_the_gpu_kernel_only():
    cfg = ModelConfig.from_preset("gpt2-tiny")
    assert cfg.head_dim != 128
    assert LLMEngine._check_spec(cfg, Mesh(), _ecfg(spec_tokens=K), "cpu") == K
    with pytest.raises(ValueError, match="head_dim 128"):
        LLMEngine._check_spec(cfg, Mesh(), _ecfg(spec_tokens=K), "cuda")
    assert LLMEngine._check_spec(cfg, Mesh(tp=2), _ecfg(), "cuda") == 0        # off: nothing is refused
    assert LLMEngine._check_spec(cfg, Mesh(dp=4), _ecfg(spec_tokens=K), "cpu") == K   # any dp


# ---- command line and server ------------------------------------------------------------------------
def test_cli_generate_and_info(capsys):
    from butterfly_amd import cli

    prompt = "abcabcabcabcabcabc"
    common = ["generate", "--model", "llama-tiny", "--max-tokens", "12", "--no-graphs", "--prompt", prompt]

    def run(extra):
        assert cli.main(common + extra) == 0
        return json.loads(capsys.readouterr().out.splitlines()[0])["token_ids"]

    plain = run([])
    assert run(["--spec-tokens", "4", "--spec-ngram-max", "3", "--spec-ngram-min", "1", "--spec-max-rows", "32"]) == plain
    with pytest.raises(ValueError, match="spec_ngram_min"):
        cli.main(common + ["--spec-tokens", "2", "--spec-ngram-min", "0"])
    assert cli.main(["info"]) == 0
    info = json.loads(capsys.readouterr().out)
    assert info["spec"]["spec_tokens"] == 0 and info["spec"]["spec_max_rows"] == 64
    assert "spec_accepted_tokens" in info["spec"]["metrics"]


def test_llm_engine_cfg_and_http_metrics():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient

    from butterfly_amd.api import LLM
    from butterfly_amd.server import ServingLoop, create_app

    ids = [1, 2, 3, 4] * 6
    base = dict(max_batch=4, max_seq_len=128, kv_cache_tokens=1024, use_graphs=False)
    want = LLM("llama-tiny", engine_config=EngineConfig(**base)).generate(
        [ids], SamplingParams(max_tokens=10, ignore_eos=True))[0].token_ids
    llm = LLM("llama-tiny", engine_cfg=EngineConfig(spec_tokens=K, spec_ngram_min=1, **base))
    assert llm.engine.spec_k == K
    with pytest.raises(ValueError, match="not both"):
        LLM("llama-tiny", engine_config=EngineConfig(**base), engine_cfg=EngineConfig(**base))
    loop = ServingLoop(llm)
    th = threading.Thread(target=loop.run, daemon=True)
    th.start()
    try:
        c = TestClient(create_app(loop))
        text = c.get("/metrics").text
        assert "bfly_spec_verify_steps 0" in text and "bfly_spec_accepted_tokens 0" in text
        r = c.post("/v1/completions", json={"prompt": ids, "max_tokens": 10, "ignore_eos": True}).json()
        got = r["choices"][0]["token_ids"]
        assert got == want[:len(got)] and len(got) >= 1
        with c.stream("POST", "/v1/completions", json={"prompt": ids, "max_tokens": 10, "stream": True}) as resp:
            events = [ln[len("data: "):] for ln in resp.iter_lines() if ln.startswith("data: ")]
        assert events[-1] == "[DONE]"
        chunks = [json.loads(e)["choices"][0] for e in events[:-1]]
        assert [t for ch in chunks for t in ch["token_ids"]] == got     # several tokens of one step, in order
        text = c.get("/metrics").text
        for name in ("spec_verify_steps", "spec_draft_tokens", "spec_accepted_tokens"):
            assert f"bfly_{name} " in text
    finally:
        loop.stop = True
        th.join(timeout=30)


# ---- the sanitizer self-test of truncate ----------------------------------------------------------------
@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_runtime_spec_selftest_asan_ubsan(tmp_path):
    exe = tmp_path / "rt_selftest_spec"
    src = os.path.join(ROOT, "csrc", "runtime", "tests", "selftest_spec.cpp")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", src, "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "runtime spec selftest: PASS" in r.stdout


# ---- sharpness of the GPU file's attn_verify cases ------------------------------------------------------
@pytest.mark.parametrize("kind,Hq,Hkv,QN,fp8", list(sc.sweep()))
def test_verify_cases_are_sharp(kind, Hq, Hkv, QN, fp8):
    """The criterion of tests/test_spec_gpu.py (zero mismatches against the bf16-P emulation, in
    attn_verify's layout) accepts the plain-torch ops.reference.attn_verify and rejects every
    mutant reference: limits shifted by one key either way, the last page taken from a
    neighbouring table entry."""
    c = sc.case(kind, Hq, Hkv, QN, fp8)
    v = sc.verify_inputs(c, QN)
    mis = ac.mismatches_for(kind)
    want = ac.reference_paged(c, emulate=True)[0][v["src"]]
    assert sorted({ql for _, ql in c.chunks})[0] == 1 and max(ql for _, ql in c.chunks) == QN
    got = ref.attn_verify(v["q"], c.kc, c.vc, c.tables, v["ctx_lens"], v["q_lens"], ac.SCALE, v["max_ctx"])
    bad, worst = mis(got, want)
    assert bad == 0, f"ops.reference.attn_verify: {bad} mismatches, worst {worst:.3g}"
    for name, out in ac.mutants_paged(c):
        bad, _ = mis(out[v["src"]], want)
        assert bad > 0, f"verify {kind} Hq={Hq} Hkv={Hkv} QN={QN} fp8={fp8}: the criterion does not notice {name}"
