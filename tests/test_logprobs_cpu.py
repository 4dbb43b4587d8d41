"""Per-token logprobs on the CPU path: the plain-torch reference ops, the engine (synchronous and
asynchronous, mixed chunked prefill, stop tokens, sampling with filters, TP2 on the loopback
backend), snapshots, the HTTP server and the CLI.

Tolerance: log-probabilities are compared with a float64 log_softmax of the same logits at 1e-4
absolute on finite entries (an f32 evaluation is within 6e-6 of float64 at these sizes; torch's
own f32 log_softmax is off by 2.5e-5 at V = 128256, hence float64). Ids are compared exactly:
logit descending, global token id ascending on equal logits (a stable descending sort)."""
import json
import math
import threading

import pytest
import torch

from butterfly_amd import SamplingParams, ops
from butterfly_amd.api import TokenLogprob, token_logprobs
from butterfly_amd.config import EngineConfig, ModelConfig
from butterfly_amd.engine import state
from butterfly_amd.engine.batch import make_prefill_batch
from butterfly_amd.engine.engine import LLMEngine
from butterfly_amd.ops import reference as ref
from butterfly_amd.parallel.fake import FakeWorld
from butterfly_amd.parallel.mesh import Mesh

TOL = 1e-4
PROMPTS = [[3, 1, 4, 1, 5], [9, 2, 6], [5, 3, 5, 8, 9, 7, 9]]


def _reference(x, ids, n, vstart=0):
    """float64 log_softmax + stable descending sort of logits x [R, V]."""
    R, V = x.shape
    xd = x.double()
    lsm = torch.log_softmax(xd, 1)
    chosen = lsm[torch.arange(R), ids.long() - vstart]
    k = min(n, V)
    order = torch.sort(xd, dim=1, descending=True, stable=True).indices[:, :k]
    top_ids = torch.full((R, n), -1, dtype=torch.int64)
    top_lp = torch.full((R, n), float("-inf"), dtype=torch.float64)
    top_ids[:, :k] = order + vstart
    top_lp[:, :k] = lsm.gather(1, order)
    return chosen, top_ids, top_lp


def _close(got, want):
    got, want = got.double(), want.double()
    fin = torch.isfinite(want)
    assert torch.equal(torch.isfinite(got), fin)
    assert torch.equal(got[~fin], want[~fin])
    err = (got[fin] - want[fin]).abs().max().item() if fin.any() else 0.0
    assert err <= TOL, err


def _rows(V, seed):
    """R = 3 rows of bf16-valued f32 logits (ties present): row 0 random, row 1 with every other
    logit -inf, row 2 all equal."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(3, V, generator=g) * 4).to(torch.bfloat16).float()
    x[1, 0::2] = float("-inf")
    x[2] = 1.5
    return x


@pytest.mark.parametrize("V", [7, 1000, 4104])
def test_reference_ops(V):
    x = _rows(V, V)
    for vstart in (0, 96192):
        ids = torch.tensor([V // 2, 1, V - 1], dtype=torch.int32) + vstart
        for n in (0, 1, 5, 20):
            rec = ops.logprobs_partial(x, ids, n, vstart=vstart)
            assert rec.shape == (3, 3 + 2 * n) and rec.dtype == torch.float32
            assert torch.equal(rec, ref.logprobs_partial(x, ids, n, vstart))
            chosen, top_ids, top_lp = ops.logprobs_merge(rec.view(1, 3, -1))
            wc, wi, wl = _reference(x, ids, n, vstart)
            assert top_ids.dtype == torch.int32 and torch.equal(top_ids.long(), wi)
            _close(chosen, wc)
            _close(top_lp, wl)
            if n > V:      # fewer valid tokens than n: id -1, logprob -inf
                assert (top_ids[:, V:] == -1).all() and torch.isinf(top_lp[:, V:]).all()
    # an id outside the shard: a -inf partial
    rec = ops.logprobs_partial(x, torch.tensor([-1, V, V + 5], dtype=torch.int32), 1)
    assert torch.isinf(rec[:, 2]).all()
    with pytest.raises(ValueError):
        ops.logprobs_partial(x, ids, 21)


def test_shard_merge():
    """V = 1000 in 4 unequal shards, each a column slice of a padded buffer whose padded columns
    (beyond the valid count) hold large values that must not enter."""
    V, n = 1000, 20
    x = _rows(V, 77)
    ids = torch.tensor([999, 1, 500], dtype=torch.int32)
    bounds = [0, 130, 512, 519, 1000]
    recs = []
    for a, b in zip(bounds, bounds[1:]):
        padded = torch.full((3, b - a + 24), 1e4)
        padded[:, : b - a] = x[:, a:b]
        recs.append(ops.logprobs_partial(padded[:, : b - a], ids, n, vstart=a))
    chosen, top_ids, top_lp = ops.logprobs_merge(torch.stack(recs))
    one = ops.logprobs_merge(ops.logprobs_partial(x, ids, n).view(1, 3, -1))
    assert torch.equal(top_ids, one[1])
    wc, wi, wl = _reference(x, ids, n)
    assert torch.equal(top_ids.long(), wi)
    _close(chosen, wc)
    _close(top_lp, wl)


# ---- engine --------------------------------------------------------------------------------
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


def _check_greedy(req, n):
    assert len(req.logprobs) == len(req.output)
    for t, (lp, top) in zip(req.output, req.logprobs):
        assert len(top) == n and top[0] == (t, lp)
        assert lp <= 0 and all(v <= 0 for _, v in top)
        assert sum(math.exp(v) for _, v in top) <= 1 + 1e-5
        assert [v for _, v in top] == sorted((v for _, v in top), reverse=True)


def _same(a, b):
    """Two runs' logprob entries: ids equal, values within tolerance."""
    assert len(a) == len(b)
    for (la, ta), (lb, tb) in zip(a, b):
        assert abs(la - lb) <= TOL and [i for i, _ in ta] == [i for i, _ in tb]
        assert all(abs(x - y) <= TOL for (_, x), (_, y) in zip(ta, tb))


@pytest.fixture(scope="module")
def greedy_runs():
    """llama-tiny, greedy: without logprobs and with logprobs=5, synchronous and asynchronous;
    mixed chunked prefill with a prompt (40 tokens) longer than one chunk (16)."""
    torch.set_num_threads(1)
    long_prompt = [(7 * i + 3) % 97 + 1 for i in range(40)]
    prompts = PROMPTS + [long_prompt]
    kw = dict(max_prefill_tokens=16, mixed_prefill=True)
    out = {}
    for name, ad, n in (("plain", False, None), ("sync", False, 5), ("async", True, 5)):
        eng = _engine(ad, **kw)
        assert bool(eng.async_pp) == ad and eng.mixed
        out[name] = _run(eng, prompts, SamplingParams(max_tokens=8, ignore_eos=True, logprobs=n))
    return out


def test_engine_greedy(greedy_runs):
    plain, sync, asyn = greedy_runs["plain"], greedy_runs["sync"], greedy_runs["async"]
    assert [r.output for r in plain] == [r.output for r in sync] == [r.output for r in asyn]
    assert all(r.logprobs == [] and token_logprobs(r) == (None, None) for r in plain)
    for a, b in zip(sync, asyn):
        assert a.finish_reason == b.finish_reason == "length" and len(a.output) == 8
        _check_greedy(a, 5)
        _check_greedy(b, 5)
        _same(a.logprobs, b.logprobs)
    lps, cum = token_logprobs(sync[0])
    assert all(isinstance(e, TokenLogprob) for e in lps) and [e.token_id for e in lps] == sync[0].output
    assert cum == pytest.approx(sum(e.logprob for e in lps))


@pytest.mark.parametrize("async_decode", [False, True])
def test_engine_stop_token(greedy_runs, async_decode):
    """A request that ends on a stop token has one entry per token it keeps (the asynchronous
    engine discards the token sampled after the stop token, and its entry)."""
    plain = greedy_runs["plain"]
    stop = plain[0].output[2]
    want = plain[0].output[: plain[0].output.index(stop) + 1]
    params = [SamplingParams(max_tokens=8, stop_token_ids=[stop], logprobs=5)] + \
        [SamplingParams(max_tokens=8, ignore_eos=True, logprobs=0)] * 2
    reqs = _run(_engine(async_decode), PROMPTS, params)
    assert reqs[0].finish_reason == "stop" and reqs[0].output == want
    _check_greedy(reqs[0], 5)
    for r, p in zip(reqs[1:], plain[1:]):        # logprobs=0: the token's own value only
        assert r.output == p.output and len(r.logprobs) == 8
        assert all(top == [] and lp <= 0 for lp, top in r.logprobs)


def test_engine_sampling_matches_float64():
    """temperature 0.8, top-k 10, seeded: the same tokens as without logprobs, and the reported
    values are log_softmax of the RAW logits (no temperature, no filter): recomputed in float64
    from the model's logits over prompt + output in reference mode."""
    torch.set_num_threads(1)
    sp = dict(max_tokens=8, temperature=0.8, top_k=10, seed=3, ignore_eos=True)
    plain = _run(_engine(), PROMPTS, SamplingParams(**sp))
    eng = _engine()
    reqs = _run(eng, PROMPTS, SamplingParams(logprobs=5, **sp))
    assert [r.output for r in reqs] == [r.output for r in plain]
    V, bs = eng.cfg.vocab_size, 16
    for r in reqs:
        toks = r.prompt + r.output[:-1]
        with ops.reference_mode():
            kv = eng.model.allocate_kv_cache(len(toks) // bs + 2, bs)
            fb = make_prefill_batch([toks], [list(range(len(toks)))])
            fb.logits_idx = torch.arange(len(r.prompt) - 1, len(toks), dtype=torch.int64)
            logits = eng.model.forward(fb, kv)[:, :V].float()
        ids = torch.tensor(r.output, dtype=torch.int32)
        wc, wi, wl = _reference(logits, ids, 5)
        _close(torch.tensor([lp for lp, _ in r.logprobs]), wc)
        assert [[i for i, _ in top] for _, top in r.logprobs] == wi.tolist()
        _close(torch.tensor([[v for _, v in top] for _, top in r.logprobs]), wl)


def test_tensor_parallel():
    """TP2 on the loopback backend: each rank's vocab shard gives a record, one all-gather, the
    same merge; ids equal the TP1 run, values within tolerance, both ranks identical."""
    torch.set_num_threads(1)
    sp = SamplingParams(max_tokens=8, ignore_eos=True, logprobs=5)
    one = _run(_engine(), PROMPTS, sp)
    mesh = Mesh(tp=2)

    def rank(r, c):
        reqs = _run(_engine(comm=c, mesh=mesh), PROMPTS, sp)
        return [(q.output, q.logprobs) for q in reqs]

    got = FakeWorld(mesh, timeout_s=120).run(rank)
    assert got[0] == got[1]
    for (out, lps), q in zip(got[0], one):
        assert out == q.output
        _same(lps, q.logprobs)


def test_refusals_and_snapshots():
    mesh = Mesh(pp=2)

    def rank(r, c):
        eng = _engine(comm=c, mesh=mesh)
        with pytest.raises(ValueError, match="logprobs"):
            eng.add_request([1, 2, 3], SamplingParams(max_tokens=2, logprobs=1))
        return True

    assert FakeWorld(mesh, timeout_s=120).run(rank) == [True, True]
    eng = _engine()
    for bad in (21, -1, 1.5, True):
        with pytest.raises(ValueError, match="logprobs"):
            eng.add_request([1, 2, 3], SamplingParams(max_tokens=2, logprobs=bad))
    assert not eng.requests
    # snapshot round trip: the field survives; logprobs themselves are not stored
    a = eng.add_request([1, 2, 3], SamplingParams(max_tokens=6, ignore_eos=True, logprobs=2))
    b = eng.add_request([4, 5], SamplingParams(max_tokens=6, ignore_eos=True))
    for _ in range(3):
        eng.step()
    done = len(eng.requests[a].output)
    assert 0 < done < 6
    snap = json.loads(json.dumps(state.snapshot(eng)))
    assert snap["requests"][0]["params"]["logprobs"] == 2 and "logprobs" not in snap["requests"][0]
    fresh = _engine()
    state.restore(fresh, snap)
    assert fresh.requests[a].params.logprobs == 2 and fresh.requests[b].params.logprobs is None
    while fresh.has_unfinished_global():
        fresh.step()
    ra = fresh.requests[a]
    assert len(ra.output) == len(ra.logprobs) == 6
    assert ra.logprobs[:done] == [None] * done and all(e is not None for e in ra.logprobs[done:])
    lps, cum = token_logprobs(ra)
    assert lps[:done] == [None] * done and cum == pytest.approx(sum(e[0] for e in ra.logprobs[done:]))
    assert fresh.requests[b].logprobs == []
    # a snapshot written before the field existed
    for r in snap["requests"]:
        del r["params"]["logprobs"]
    old = _engine()
    state.restore(old, snap)
    assert all(q.params.logprobs is None for q in old.requests.values())


# ---- public interfaces ----------------------------------------------------------------------
def _llm():
    from butterfly_amd.api import LLM

    return LLM("llama-tiny", engine_config=EngineConfig(max_batch=4, max_seq_len=128, kv_cache_tokens=1024,
                                                        use_graphs=False))


def test_llm_generate():
    llm = _llm()
    outs = llm.generate(["hello", [5, 6, 7]], SamplingParams(max_tokens=4, ignore_eos=True, logprobs=2))
    for o in outs:
        assert [e.token_id for e in o.logprobs] == o.token_ids and len(o.logprobs) == 4
        assert all(len(e.top) == 2 and e.top[0] == (e.token_id, e.logprob) for e in o.logprobs)
        assert o.cumulative_logprob == pytest.approx(sum(e.logprob for e in o.logprobs))
    plain = llm.generate([[5, 6, 7]], SamplingParams(max_tokens=4, ignore_eos=True))[0]
    assert plain.token_ids == outs[1].token_ids and plain.logprobs is None and plain.cumulative_logprob is None


def test_http_logprobs():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient

    from butterfly_amd.server import ServingLoop, create_app

    llm = _llm()
    loop = ServingLoop(llm)
    th = threading.Thread(target=loop.run, daemon=True)
    th.start()
    try:
        c = TestClient(create_app(loop))
        plain = c.post("/v1/completions", json={"prompt": [1, 2, 3], "max_tokens": 4}).json()
        assert set(plain["choices"][0]) == {"index", "text", "token_ids", "finish_reason"}
        r = c.post("/v1/completions", json={"prompt": [1, 2, 3], "max_tokens": 4, "logprobs": 2}).json()
        ch = r["choices"][0]
        assert ch["token_ids"] == plain["choices"][0]["token_ids"]
        lp = ch["logprobs"]
        assert set(lp) == {"token_ids", "token_logprobs", "top_logprobs"}
        assert lp["token_ids"] == ch["token_ids"] and len(lp["token_logprobs"]) == len(lp["top_logprobs"]) == 4
        for t, v, top in zip(lp["token_ids"], lp["token_logprobs"], lp["top_logprobs"]):
            assert len(top) == 2 and set(top[0]) == {"token_id", "logprob", "token"}
            assert top[0]["token_id"] == t and top[0]["logprob"] == v and v <= 0 and top[0]["token"] is None
        text = c.post("/v1/completions", json={"prompt": "hi there", "max_tokens": 3, "logprobs": 1}).json()
        assert all(isinstance(e[0]["token"], str) for e in text["choices"][0]["logprobs"]["top_logprobs"])
        zero = c.post("/v1/completions", json={"prompt": [1, 2, 3], "max_tokens": 4, "logprobs": 0}).json()
        assert zero["choices"][0]["logprobs"]["top_logprobs"] == [[]] * 4
        assert zero["choices"][0]["logprobs"]["token_logprobs"] == pytest.approx(lp["token_logprobs"], abs=TOL)
        with c.stream("POST", "/v1/completions",
                      json={"prompt": [1, 2, 3], "max_tokens": 4, "stream": True, "logprobs": 2}) as resp:
            events = [ln[len("data: "):] for ln in resp.iter_lines() if ln.startswith("data: ")]
        assert events[-1] == "[DONE]"
        chunks = [json.loads(e)["choices"][0] for e in events[:-1]]
        toks = [ch for ch in chunks if ch["token_ids"]]
        assert [ch["token_ids"][0] for ch in toks] == lp["token_ids"]
        for ch, v, top in zip(toks, lp["token_logprobs"], lp["top_logprobs"]):
            assert ch["logprobs"]["token_ids"] == ch["token_ids"]
            assert ch["logprobs"]["token_logprobs"] == pytest.approx([v], abs=TOL)
            assert [e["token_id"] for e in ch["logprobs"]["top_logprobs"][0]] == [e["token_id"] for e in top]
        assert "logprobs" not in chunks[-1] and chunks[-1]["finish_reason"] == "length"
        assert c.post("/v1/completions", json={"prompt": [1, 2, 3], "max_tokens": 4, "logprobs": 99}).status_code == 400
    finally:
        loop.stop = True
        th.join(timeout=30)


def test_cli_logprobs(capsys):
    from butterfly_amd import cli

    assert cli.main(["generate", "--model", "llama-tiny", "--max-tokens", "4", "--no-graphs", "--prompt", "abc",
                     "--logprobs", "2"]) == 0
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    head, entries = lines[0], lines[1:]
    assert len(head["token_ids"]) == 4 and len(entries) == 4
    for pos, (t, e) in enumerate(zip(head["token_ids"], entries)):
        assert e["request"] == 0 and e["position"] == pos and e["token_id"] == t and e["logprob"] <= 0
        assert len(e["top"]) == 2 and e["top"][0] == {"token_id": t, "logprob": e["logprob"]}
