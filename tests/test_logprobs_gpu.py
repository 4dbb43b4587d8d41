"""Per-token logprobs on the GPU: the fused log-softmax / top-N kernels (csrc/kernels/logprobs.hip)
against a float64 log_softmax of the same bf16 logits, and the engine's graph-sampling path.

Tolerance: 1e-4 absolute on finite log-probabilities (an f32 chunked evaluation differs from
float64 by at most 6e-6 on these sizes; the rest is room for the GPU's exp and log). Ids are
compared exactly: the order is logit descending, global token id ascending on equal logits
(bf16 logits tie often), which is what a stable descending sort gives."""
import math

import pytest
import torch

from butterfly_amd import SamplingParams, ops
from butterfly_amd.api import token_logprobs
from butterfly_amd.config import EngineConfig, ModelConfig
from butterfly_amd.engine.engine import LLMEngine

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-4
NS = (0, 1, 5, 20)


@pytest.fixture(autouse=True, scope="module")
def _kernels_loaded():
    assert ops.load_library(), "butterfly_amd/_C.so not built or failed to load"


@pytest.fixture
def poisoned():
    prev = ops._POISON
    ops.set_poison(True)
    yield
    ops.set_poison(prev)


def _logits(R, V, seed=0, pad=64):
    """bf16 randn * 4 logits [R, V] as a column slice of a wider buffer (row stride > V), with
    row 0 masked to -inf on every other column (the last column stays finite)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    stride = (V + 7) // 8 * 8 + pad
    buf = (torch.randn(R, stride, generator=g) * 4).to(torch.bfloat16)
    buf[0, 0:max(V - 1, 0):2] = float("-inf")
    return buf


def _ids(R, V, vstart, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    ids = torch.randint(0, V, (R,), generator=g, dtype=torch.int32) + vstart
    ids[R - 1] = vstart + V - 1          # the last valid column
    return ids


def _reference(x, ids, n, vstart):
    """float64 log_softmax + stable descending sort of bf16 logits x [R, V] (CPU)."""
    R, V = x.shape
    xd = x.double()
    lsm = torch.log_softmax(xd, 1)
    chosen = lsm[torch.arange(R), (ids.long() - vstart)]
    k = min(n, V)
    order = torch.sort(xd, dim=1, descending=True, stable=True).indices[:, :k]
    top_ids = torch.full((R, n), -1, dtype=torch.int64)
    top_lp = torch.full((R, n), float("-inf"), dtype=torch.float64)
    top_ids[:, :k] = order + vstart
    top_lp[:, :k] = lsm.gather(1, order)
    return chosen, top_ids, top_lp


def _close(got, want):
    got, want = got.double().cpu(), want.double()
    fin = torch.isfinite(want)
    assert torch.equal(torch.isfinite(got), fin)
    assert torch.equal(got[~fin], want[~fin])
    err = (got[fin] - want[fin]).abs().max().item() if fin.any() else 0.0
    assert err <= TOL, err


def _check(buf, V, ids, n, vstart):
    lg = buf.to(DEV)[:, :V]
    rec = ops.logprobs_partial(lg, ids.to(DEV), n, vstart=vstart)
    assert rec.shape == (buf.shape[0], 3 + 2 * n) and rec.dtype == torch.float32
    chosen, top_ids, top_lp = ops.logprobs_merge(rec.view(1, *rec.shape))
    wc, wi, wl = _reference(buf[:, :V], ids, n, vstart)
    assert torch.equal(top_ids.cpu().long(), wi)
    _close(chosen, wc)
    _close(top_lp, wl)
    return chosen, top_ids, top_lp


@pytest.mark.parametrize("V", [7, 1000, 8200, 32064])
@pytest.mark.parametrize("R", [1, 3, 65])
def test_kernel_matches_float64(R, V):
    """Sizes: below one 16-B load, the per-element tail (V % 8 != 0), a full chunk plus a ragged
    one whatever the chunk size (8200), and a TP shard of a 128256 vocabulary; 65 rows = more than
    one wave of row indices. V = 7 with n = 20 pads with id -1 / -inf."""
    buf = _logits(R, V, seed=R * 131 + V)
    assert buf.stride(0) > V
    for vstart in (0, 96192):
        ids = _ids(R, V, vstart, seed=V)
        for n in NS:
            _, top_ids, top_lp = _check(buf, V, ids, n, vstart)
            if n > V:
                assert (top_ids[:, V:] == -1).all() and torch.isinf(top_lp[:, V:]).all()


def test_chosen_outside_shard():
    """An id outside [vstart, vstart + V) (another TP rank's token, or the NaN guard's -1) gives
    a -inf partial, and the statistics are untouched."""
    V, vstart = 1000, 96192
    buf = _logits(3, V, seed=5)
    lg = buf.to(DEV)[:, :V]
    inside = ops.logprobs_partial(lg, _ids(3, V, vstart).to(DEV), 5, vstart=vstart)
    for out in ([vstart - 1, vstart + V, -1], [0, 5, 96191]):
        rec = ops.logprobs_partial(lg, torch.tensor(out, dtype=torch.int32, device=DEV), 5, vstart=vstart)
        assert torch.isinf(rec[:, 2]).all() and (rec[:, 2] < 0).all()
        assert torch.equal(rec[:, :2], inside[:, :2]) and torch.equal(rec[:, 3:], inside[:, 3:])


def test_tp_merge():
    """Four vocab shards of 32064 columns, their records stacked as the TP all-gather would,
    against the unsharded V = 128256 result: ids exact, values within tolerance."""
    R, V, tp, n = 3, 128256, 4, 20
    buf = _logits(R, V, seed=9, pad=0)
    ids = _ids(R, V, 0, seed=9)
    full = buf.to(DEV)
    vl = V // tp
    recs = torch.stack([ops.logprobs_partial(full[:, k * vl:(k + 1) * vl], ids.to(DEV), n, vstart=k * vl)
                        for k in range(tp)])
    chosen, top_ids, top_lp = ops.logprobs_merge(recs)
    wc, wi, wl = _reference(buf, ids, n, 0)
    assert torch.equal(top_ids.cpu().long(), wi)
    _close(chosen, wc)
    _close(top_lp, wl)
    one = ops.logprobs_merge(ops.logprobs_partial(full, ids.to(DEV), n).view(1, R, -1))
    assert torch.equal(one[1], top_ids)
    assert (one[0] - chosen).abs().max().item() <= TOL and (one[2] - top_lp).abs().max().item() <= TOL


def test_poisoned_arena(poisoned):
    """Outputs allocated as NaN / sentinels and a workspace full of garbage: same results."""
    R, V, n = 3, 8200, 5
    buf = _logits(R, V, seed=3)
    ids = _ids(R, V, 0)
    ops.set_poison(False)
    want = _check(buf, V, ids, n, 0)
    ops.set_poison(True)
    ops._arena.get(torch.device(DEV, torch.cuda.current_device()), "logprobs", 1, torch.int64).fill_(-1)
    got = _check(buf, V, ids, n, 0)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_graph_capture():
    """partial + merge captured as one linear chain; a replay after the logits and ids were
    overwritten in place matches an eager call bitwise."""
    R, V, n, vstart = 4, 8200, 5, 96192
    a, b = _logits(R, V, seed=1), _logits(R, V, seed=2)
    ia, ib = _ids(R, V, vstart, seed=1), _ids(R, V, vstart, seed=2)
    buf, ids = a.to(DEV), ia.to(DEV)

    def run():
        rec = ops.logprobs_partial(buf[:, :V], ids, n, vstart=vstart)
        return ops.logprobs_merge(rec.view(1, *rec.shape))

    run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = run()
    buf.copy_(b)
    ids.copy_(ib)
    g.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in out]
    want = run()
    for x, y in zip(got, want):
        assert torch.equal(x, y)
    assert torch.equal(got[1].cpu().long(), _reference(b[:, :V], ib, n, vstart)[1])


def test_engine_graph_sampling():
    """llama-tiny, decode graphs ending in the sampler, asynchronous engine; logprobs=3 on every
    other request. Tokens equal a run without logprobs; greedy tokens are top[0]; the other
    requests report nothing."""
    cfg = ModelConfig.from_preset("llama-tiny")
    prompts = [[i + 1, 2 * i + 3, 5] * 3 for i in range(6)]

    def run(n):
        eng = LLMEngine(cfg, engine_cfg=EngineConfig(max_batch=8, max_seq_len=128, kv_cache_tokens=2048,
                                                     use_graphs=True, graph_batch_sizes=[8], seed=11), device=DEV)
        assert eng.async_pp and eng.runner.sample_fn is not None
        rids = [eng.add_request(p, SamplingParams(max_tokens=8, ignore_eos=True,
                                                  logprobs=n if i % 2 == 0 else None))
                for i, p in enumerate(prompts)]
        while eng.has_unfinished_global():
            eng.step()
        reqs = [eng.requests[r] for r in rids]
        eng.close()
        return reqs

    plain, with_lp = run(None), run(3)
    assert [r.output for r in plain] == [r.output for r in with_lp]
    for i, r in enumerate(with_lp):
        if i % 2:
            assert r.logprobs == [] and token_logprobs(r) == (None, None)
            continue
        assert len(r.logprobs) == len(r.output) == 8
        for t, (lp, top) in zip(r.output, r.logprobs):
            assert len(top) == 3 and top[0][0] == t and top[0][1] == lp
            assert all(v <= 0 for _, v in top) and lp <= 0
            assert sum(math.exp(v) for _, v in top) <= 1 + 1e-5
            assert [v for _, v in top] == sorted((v for _, v in top), reverse=True)
