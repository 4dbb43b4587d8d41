"""Presence / frequency / repetition penalties on the CPU path: the reference op against a naive
per-token loop, the engine (synchronous and asynchronous, mixed chunked prefill, preemption, TP2
on the loopback backend, snapshots), the HTTP server and the CLI.

Semantics (ops.reference.apply_penalties): for the logit x of token t, with P the prompt, O the
tokens generated so far and c the occurrences of t in O, in f32:
  if t in P or c > 0: x = x / rep if x > 0 else x * rep;  x -= freq * c;  x -= pres * (c > 0)
with 1 / rep taken once in f32 on the host, then one rounding to the logits' dtype."""
import json
import threading

import numpy as np
import pytest
import torch

from butterfly_amd import SamplingParams, ops
from butterfly_amd.config import EngineConfig, ModelConfig
from butterfly_amd.engine import state
from butterfly_amd.engine.batch import make_prefill_batch
from butterfly_amd.engine.engine import LLMEngine
from butterfly_amd.ops import reference as ref
from butterfly_amd.parallel.fake import FakeWorld
from butterfly_amd.parallel.mesh import Mesh

PROMPTS = [[3, 1, 4, 1, 5], [9, 2, 6], [5, 3, 5, 8, 9, 7, 9]]
LONG = [(7 * i + 3) % 97 + 1 for i in range(40)]
PEN = dict(repetition_penalty=1.3, frequency_penalty=0.7, presence_penalty=0.4)


# ---- reference op ---------------------------------------------------------------------------
def _naive(logits, hist, slots, lens, plens, last, params, vstart):
    """The semantics, one history token at a time, numpy f32 scalars."""
    out = logits.clone()
    V = logits.shape[1]
    for r in range(logits.shape[0]):
        slot, n = int(slots[r]), int(lens[r])
        if slot < 0 or n <= 0:
            continue
        toks = hist[slot, :n - 1].tolist() + [int(last[r])]
        in_prompt, count = set(), {}
        for p, t in enumerate(toks):
            if p < int(plens[r]):
                in_prompt.add(t)
            else:
                count[t] = count.get(t, 0) + 1
        rep, inv_rep, freq, pres = (np.float32(v) for v in params[r].tolist())
        for t in in_prompt | set(count):
            col = t - vstart
            if not 0 <= col < V:
                continue
            c = count.get(t, 0)
            x = np.float32(float(logits[r, col]))
            with np.errstate(all="ignore"):
                x = x * inv_rep if x > 0 else x * rep
                x = np.float32(x - np.float32(freq * np.float32(c)))
                x = np.float32(x - np.float32(pres * np.float32(1 if c else 0)))
            out[r, col] = torch.tensor(float(x), dtype=torch.float32).to(logits.dtype)
    return out


def _case(R, V, vstart, seed, width=128):
    """bf16 logits [R, V] and histories of 90 tokens (12 of them prompt): tokens only in the
    prompt, only in the output, in both, one 40 times in the output, ids of other shards, a
    negative id, -inf logits under history tokens. Row 1 (R = 3) has no slot but non-default
    parameters; row 2 has a history and default parameters."""
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(R, V, generator=g) * 4).to(torch.bfloat16)
    hist = torch.full((4, width), -5, dtype=torch.int32)
    n, plen = 90, 12
    cols = [0, V - 1, V // 2, V // 3, min(4095, V - 1), min(4096, V - 1), 1 % V, 2 % V]
    slots, lens, plens, last = [], [], [], []
    for r in range(R):
        both, p_only, o_only, many = (vstart + cols[(r + k) % len(cols)] for k in range(4))
        row = [int(t) for t in torch.randint(0, V, (n,), generator=g) + vstart]
        row[0:4] = [both, p_only, p_only, vstart - 1 if vstart else -1]
        row[4:6] = [vstart + V, 5]                     # the column after the shard; shard 0's token
        row[12:16] = [both, both, o_only, -1]
        row[20:60] = [many] * 40
        logits[r, both - vstart] = float("-inf")
        hist[3 - r, :n - 1] = torch.tensor(row[:n - 1], dtype=torch.int32)
        slots.append(3 - r)
        lens.append(n)
        plens.append(plen)
        last.append(row[n - 1] if r else many)
    params = [(1.3, 0.7, 0.4)] * R
    if R == 3:
        slots[1] = -1
        params[2] = (1.0, 0.0, 0.0)
    i32 = lambda a: torch.tensor(a, dtype=torch.int32)      # noqa: E731
    return logits, hist, i32(slots), i32(lens), i32(plens), i32(last), ops.penalty_params(params)


@pytest.mark.parametrize("V", [7, 1000, 8200])
@pytest.mark.parametrize("R", [1, 3])
def test_reference_matches_naive_loop(R, V):
    for vstart in (0, 96192):
        logits, hist, slots, lens, plens, last, params = _case(R, V, vstart, seed=R * 31 + V)
        want = _naive(logits, hist, slots, lens, plens, last, params, vstart)
        before = hist.clone()
        got = ops.apply_penalties(logits, hist, slots, lens, plens, last, params, vstart=vstart)
        assert got.dtype == logits.dtype and got.data_ptr() != logits.data_ptr()
        assert torch.equal(got.view(torch.int16), want.view(torch.int16))
        assert not torch.equal(got[0].view(torch.int16), logits[0].view(torch.int16))
        for r in range(R):
            s = int(slots[r])
            if s >= 0:
                assert int(hist[s, int(lens[r]) - 1]) == int(last[r])
                before[s, int(lens[r]) - 1] = last[r]
        assert torch.equal(hist, before)                    # nothing else was written
        if R == 3:
            assert torch.equal(got[1].view(torch.int16), logits[1].view(torch.int16))   # no slot
            assert torch.equal(got[2].view(torch.int16), logits[2].view(torch.int16))   # defaults
        # -inf stays -inf
        assert torch.equal(torch.isinf(got), torch.isinf(logits))


def test_reference_edges():
    """len <= 0: no history, no write; len 1: `last` alone; the host's f32 reciprocal."""
    logits = torch.tensor([[2.0, -2.0, 1.0]], dtype=torch.bfloat16)
    hist = torch.full((1, 8), 1, dtype=torch.int32)
    i32 = lambda a: torch.tensor(a, dtype=torch.int32)      # noqa: E731
    params = ops.penalty_params([(2.0, 0.5, 0.25)])
    assert params.dtype == torch.float32 and params.tolist() == [[2.0, 0.5, 0.5, 0.25]]
    assert ops.penalty_params([(1.3, 0, 0)])[0, 1].item() == float(np.float32(1) / np.float32(1.3))
    out = ops.apply_penalties(logits, hist, i32([0]), i32([0]), i32([0]), i32([0]), params)
    assert torch.equal(out, logits) and hist.tolist() == [[1] * 8]
    out = ops.apply_penalties(logits, hist, i32([0]), i32([1]), i32([0]), i32([0]), params)
    assert out.tolist() == [[2.0 * 0.5 - 0.5 - 0.25, -2.0, 1.0]] and hist[0].tolist() == [0] + [1] * 7
    out = ops.apply_penalties(logits, hist, i32([0]), i32([3]), i32([3]), i32([1]), params)   # prompt only
    assert out.tolist() == [[1.0, -4.0, 1.0]]


# ---- engine ---------------------------------------------------------------------------------
def _engine(async_decode=False, comm=None, mesh=Mesh(), **kw):
    cfg = ModelConfig.from_preset("llama-tiny")
    e = dict(max_batch=4, max_seq_len=128, kv_cache_tokens=2048, use_graphs=False, seed=5,
             async_decode=async_decode)
    e.update(kw)
    return LLMEngine(cfg, mesh, EngineConfig(**e), comm=comm, device="cpu")


def _run(eng, prompts, params):
    params = params if isinstance(params, list) else [params] * len(prompts)
    rids = [eng.add_request(p, q) for p, q in zip(prompts, params)]
    while eng.has_unfinished_global():
        eng.step()
    return [eng.requests[r] for r in rids]


def _free_list_full(eng):
    return eng._pen is not None and not eng._pen.slot and sorted(eng._pen.free) == list(range(eng.ecfg.max_batch))


@pytest.fixture(scope="module")
def runs():
    """llama-tiny, greedy, 12 tokens, mixed chunked prefill with a prompt (40 tokens) longer than
    one chunk (16): no penalties, explicit defaults, penalties (synchronous and asynchronous),
    and a batch in which every other request is penalised."""
    torch.set_num_threads(1)
    prompts = PROMPTS + [LONG]
    kw = dict(max_prefill_tokens=16, mixed_prefill=True)
    sp = dict(max_tokens=12, ignore_eos=True)
    out, engines = {}, {}
    for name, ad, params in (
            ("plain", False, SamplingParams(**sp)),
            ("defaults", True, SamplingParams(presence_penalty=0.0, frequency_penalty=0.0,
                                              repetition_penalty=1.0, **sp)),
            ("sync", False, SamplingParams(**sp, **PEN)),
            ("async", True, SamplingParams(**sp, **PEN)),
            ("mixed", True, [SamplingParams(**sp, **(PEN if i % 2 == 0 else {})) for i in range(4)])):
        eng = engines[name] = _engine(ad, **kw)
        assert bool(eng.async_pp) == ad and eng.mixed
        out[name] = [r.output for r in _run(eng, prompts, params)]
    out["engines"] = engines
    out["prompts"] = prompts
    return out


def test_engine_teacher_forced_oracle(runs):
    """The model's reference-mode logits over prompt + output, penalised with the history
    prompt + output[:i] by the reference op: the argmax is output[i]."""
    eng = runs["engines"]["sync"]
    V, bs = eng.cfg.vocab_size, 16
    p = SamplingParams(**PEN)
    params = ops.penalty_params([(p.repetition_penalty, p.frequency_penalty, p.presence_penalty)])
    i32 = lambda a: torch.tensor(a, dtype=torch.int32)      # noqa: E731
    for prompt, output in zip(runs["prompts"], runs["sync"]):
        assert len(output) == 12
        toks = prompt + output[:-1]
        with ops.reference_mode():
            kv = eng.model.allocate_kv_cache(len(toks) // bs + 2, bs)
            fb = make_prefill_batch([toks], [list(range(len(toks)))])
            fb.logits_idx = torch.arange(len(prompt) - 1, len(toks), dtype=torch.int64)
            logits = eng.model.forward(fb, kv)[:, :V].float()
        for i, t in enumerate(output):
            n = len(prompt) + i
            hist = i32(toks[:n] + [0] * (-n % 4)).view(1, -1)
            pen = ref.apply_penalties(logits[i:i + 1], hist, i32([0]), i32([n]), i32([len(prompt)]),
                                      i32([toks[n - 1]]), params)
            assert int(pen[0].argmax()) == t, (prompt, i)


def test_engine_async_matches_sync(runs):
    """A history that misses the token still in flight would diverge here."""
    assert runs["async"] == runs["sync"]
    assert runs["sync"] != runs["plain"], "the penalties must change some token"
    for name in ("sync", "async"):
        assert _free_list_full(runs["engines"][name])


def test_engine_defaults_are_the_unchanged_path(runs):
    assert runs["defaults"] == runs["plain"]
    assert runs["engines"]["defaults"]._pen is None and runs["engines"]["plain"]._pen is None
    assert not SamplingParams().needs_penalty and SamplingParams(presence_penalty=0.1).needs_penalty


def test_engine_mixed_batch(runs):
    for i, out in enumerate(runs["mixed"]):
        assert out == (runs["sync"][i] if i % 2 == 0 else runs["plain"][i])
    assert _free_list_full(runs["engines"]["mixed"])


def test_engine_seeded_sampling_sync_async():
    torch.set_num_threads(1)
    sp = SamplingParams(max_tokens=12, temperature=0.8, top_k=10, seed=3, ignore_eos=True, **PEN)
    kw = dict(max_prefill_tokens=16, mixed_prefill=True)
    a = [r.output for r in _run(_engine(False, **kw), PROMPTS + [LONG], sp)]
    b = [r.output for r in _run(_engine(True, **kw), PROMPTS + [LONG], sp)]
    assert a == b


def test_engine_preemption():
    """A KV cache too small for the running sequences (tests/test_distributed_cpu.py
    test_async_mixed_preemption_recompute_matches_sync): preempted sequences give their history
    row back and are rewritten on recompute, the token still in flight included."""
    torch.set_num_threads(1)
    prompts = [[(3 * i + j) % 90 + 1 for i in range(30)] for j in range(4)]
    params = [SamplingParams(max_tokens=12 + i, ignore_eos=True, **PEN) for i in range(4)]

    def run(async_decode, kv_tokens):
        eng = _engine(async_decode, max_seq_len=160, kv_cache_tokens=kv_tokens, max_prefill_tokens=24,
                      mixed_prefill=True, prefix_caching=True)
        out = [r.output for r in _run(eng, prompts, params)]
        assert _free_list_full(eng)
        return out, eng.metrics.counters.get("preempted_sequences", 0)

    ample, pre = run(False, 2048)
    assert pre == 0
    for async_decode in (False, True):
        got, pre = run(async_decode, 160)
        assert pre > 0, "the configuration must preempt"
        assert got == ample


def test_tensor_parallel(runs):
    """TP2 on the loopback backend: each rank penalises its own vocab shard from its own
    history; both ranks identical and equal to TP1."""
    mesh = Mesh(tp=2)
    sp = SamplingParams(max_tokens=12, ignore_eos=True, **PEN)

    def rank(r, c):
        eng = _engine(comm=c, mesh=mesh, max_prefill_tokens=16, mixed_prefill=True)
        return [q.output for q in _run(eng, PROMPTS + [LONG], sp)]

    got = FakeWorld(mesh, timeout_s=120).run(rank)
    assert got[0] == got[1] == runs["sync"]


def test_refusals():
    eng = _engine()
    bad = [dict(presence_penalty=2.5), dict(presence_penalty=-2.01), dict(frequency_penalty=3),
           dict(frequency_penalty=float("nan")), dict(presence_penalty=float("inf")), dict(repetition_penalty=0),
           dict(repetition_penalty=-1.0), dict(repetition_penalty=float("inf")), dict(repetition_penalty=float("nan")),
           dict(presence_penalty=True), dict(frequency_penalty=False), dict(repetition_penalty=True),
           dict(presence_penalty="1"), dict(repetition_penalty=None)]
    for kw in bad:
        with pytest.raises(ValueError, match="penalty"):
            eng.add_request([1, 2, 3], SamplingParams(max_tokens=2, **kw))
    assert not eng.requests and eng._pen is None
    for kw in (dict(presence_penalty=2, frequency_penalty=-2.0), dict(repetition_penalty=1e-3)):
        eng.add_request([1, 2, 3], SamplingParams(max_tokens=2, **kw))
    mesh = Mesh(pp=2)

    def rank(r, c):
        e = _engine(comm=c, mesh=mesh)
        with pytest.raises(ValueError, match="pipeline"):
            e.add_request([1, 2, 3], SamplingParams(max_tokens=2, frequency_penalty=0.5))
        e.add_request([1, 2, 3], SamplingParams(max_tokens=2))
        return True

    assert FakeWorld(mesh, timeout_s=120).run(rank) == [True, True]


def test_snapshot_round_trip(runs):
    """The fields travel; a run resumed mid-generation (prompt + output re-prefilled, P still the
    request's prompt) ends with the uninterrupted run's tokens."""
    torch.set_num_threads(1)
    kw = dict(max_prefill_tokens=16, mixed_prefill=True)
    sp = SamplingParams(max_tokens=12, ignore_eos=True, **PEN)
    eng = _engine(**kw)
    rids = [eng.add_request(p, sp) for p in PROMPTS + [LONG]]
    for _ in range(6):
        eng.step()
    done = [len(eng.requests[r].output) for r in rids]
    assert any(0 < d < 12 for d in done)
    snap = json.loads(json.dumps(state.snapshot(eng)))
    assert all(snap["requests"][0]["params"][k] == v for k, v in PEN.items())
    fresh = _engine(**kw)
    state.restore(fresh, snap)
    assert all(getattr(fresh.requests[r].params, k) == v for r in rids for k, v in PEN.items())
    while fresh.has_unfinished_global():
        fresh.step()
    assert [fresh.requests[r].output for r in rids] == runs["sync"]
    assert _free_list_full(fresh)
    for r in snap["requests"]:              # a snapshot written before the fields existed
        for k in PEN:
            del r["params"][k]
    old = _engine(**kw)
    state.restore(old, snap)
    assert not any(q.params.needs_penalty for q in old.requests.values()) and old._pen is None


# ---- public interfaces ----------------------------------------------------------------------
def _llm():
    from butterfly_amd.api import LLM

    return LLM("llama-tiny", engine_config=EngineConfig(max_batch=4, max_seq_len=128, kv_cache_tokens=1024,
                                                        use_graphs=False))


def test_llm_generate():
    llm = _llm()
    prompt = [[5, 6, 7, 5, 6, 7]]
    plain = llm.generate(prompt, SamplingParams(max_tokens=12, ignore_eos=True))[0]
    pen = llm.generate(prompt, SamplingParams(max_tokens=12, ignore_eos=True, repetition_penalty=1.8,
                                              frequency_penalty=2.0, presence_penalty=2.0))[0]
    assert len(pen.token_ids) == 12 and pen.token_ids != plain.token_ids
    again = llm.generate(prompt, SamplingParams(max_tokens=12, ignore_eos=True))[0]
    assert again.token_ids == plain.token_ids


def test_http_penalties():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient

    from butterfly_amd.server import ServingLoop, create_app

    llm = _llm()
    loop = ServingLoop(llm)
    seen = []
    add = llm.engine.add_request
    llm.engine.add_request = lambda ids, params=None, rid=None: (seen.append(params), add(ids, params, rid=rid))[1]
    th = threading.Thread(target=loop.run, daemon=True)
    th.start()
    try:
        c = TestClient(create_app(loop))
        body = {"prompt": [5, 6, 7, 5, 6, 7], "max_tokens": 12}
        plain = c.post("/v1/completions", json=body)
        assert plain.status_code == 200 and not seen[-1].needs_penalty
        r = c.post("/v1/completions", json=dict(body, presence_penalty=2.0, frequency_penalty=2, repetition_penalty=1.8))
        assert r.status_code == 200
        p = seen[-1]
        assert (p.presence_penalty, p.frequency_penalty, p.repetition_penalty) == (2.0, 2, 1.8)
        assert r.json()["choices"][0]["token_ids"] != plain.json()["choices"][0]["token_ids"]
        assert set(r.json()["choices"][0]) == set(plain.json()["choices"][0])
        with c.stream("POST", "/v1/completions", json=dict(body, stream=True, presence_penalty=2.0,
                                                           frequency_penalty=2, repetition_penalty=1.8)) as resp:
            events = [ln[len("data: "):] for ln in resp.iter_lines() if ln.startswith("data: ")]
        toks = [t for e in events[:-1] for t in json.loads(e)["choices"][0]["token_ids"]]
        assert events[-1] == "[DONE]" and toks == r.json()["choices"][0]["token_ids"]
        n = len(seen)
        for bad in (dict(presence_penalty=2.5), dict(frequency_penalty=-3), dict(repetition_penalty=0),
                    dict(repetition_penalty=-1), dict(presence_penalty=True), dict(frequency_penalty="x")):
            assert c.post("/v1/completions", json=dict(body, **bad)).status_code == 400, bad
        assert len(seen) == n
    finally:
        loop.stop = True
        th.join(timeout=30)


def test_cli_flags(capsys):
    from butterfly_amd import cli

    base = ["generate", "--model", "llama-tiny", "--max-tokens", "12", "--no-graphs", "--prompt", "abcabc"]
    assert cli.main(base) == 0
    plain = json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][0])
    assert cli.main(base + ["--presence-penalty", "2", "--frequency-penalty", "2.0", "--repetition-penalty", "1.8"]) == 0
    pen = json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][0])
    assert len(pen["token_ids"]) == 12 and pen["token_ids"] != plain["token_ids"]
