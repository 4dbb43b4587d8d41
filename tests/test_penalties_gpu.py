"""Presence / frequency / repetition penalties on the GPU: the fused kernel
(csrc/kernels/penalties.hip) against the CPU reference (ops.reference.apply_penalties), and the
engine's graph-sampling path.

Tolerance: a column whose token is not in the row's history, and every column of a row without a
history, must keep its bits. A penalised column may differ from the reference by one bf16 ulp:
the f32 value can differ by a few f32 ulps through FMA contraction of x - freq * c before the one
rounding to bf16. With operands whose every f32 intermediate is exact the result is bitwise."""
import pytest
import torch

from butterfly_amd import SamplingParams, ops
from butterfly_amd.config import EngineConfig, ModelConfig
from butterfly_amd.engine.batch import make_prefill_batch
from butterfly_amd.engine.engine import LLMEngine
from butterfly_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
PEN = dict(repetition_penalty=1.3, frequency_penalty=0.7, presence_penalty=0.4)
LENGTHS = ((1, 128), (5, 128), (127, 128), (128, 128), (300, 304))     # (history length, hist width)


@pytest.fixture(autouse=True, scope="module")
def _kernels_loaded():
    assert ops.load_library(), "butterfly_amd/_C.so not built or failed to load"


@pytest.fixture
def poisoned():
    prev = ops._POISON
    ops.set_poison(True)
    yield
    ops.set_poison(prev)


def _i32(a):
    return torch.tensor(a, dtype=torch.int32)


def _case(R, V, vstart, n, width, seed, exact=False):
    """Host tensors of one call. Logits: a column slice of a wider buffer (row stride > V), -inf
    under one history token of row 0. Histories of n tokens (the last one passed as `last`), a
    third of them prompt: the columns 0, 4095, 4096 and V - 1 (where the shard has them),
    duplicates (a pool of 24 tokens), ids of other shards and -1; the unused tail of every hist
    row holds an in-shard token that must not be counted. Row 1 of R >= 3 has no slot but
    non-default parameters."""
    g = torch.Generator().manual_seed(seed)
    stride = (V + 7) // 8 * 8 + 64
    if exact:
        buf = (torch.randint(-128, 129, (R, stride), generator=g).float() / 8).to(torch.bfloat16)
    else:
        buf = (torch.randn(R, stride, generator=g) * 4).to(torch.bfloat16)
    hist = torch.full((R + 1, width), vstart + min(3, V - 1), dtype=torch.int32)
    special = [vstart, vstart + min(4095, V - 1), vstart + min(4096, V - 1), vstart + V - 1, vstart,
               vstart + V + 5, vstart - 3 if vstart else 1 << 20, -1, vstart]
    slots, lens, plens, last = [], [], [], []
    for r in range(R):
        pool = (torch.randint(0, V, (24,), generator=g) + vstart).tolist()
        toks = special[r % 4:] + [pool[int(i)] for i in torch.randint(0, 24, (max(n, 32),), generator=g)]
        if exact:           # counts <= 32
            toks = [t for i, t in enumerate(toks) if toks[:i].count(t) < 32]
        toks = toks[:n]
        slot = R - r
        hist[slot, :n - 1] = _i32(toks[:n - 1])
        slots.append(slot)
        lens.append(n)
        plens.append(n // 3 if r % 2 == 0 else 0)
        last.append(toks[n - 1])
        if r == 0 and n > 1 and 0 <= toks[1] - vstart < V:
            buf[0, toks[1] - vstart] = float("-inf")
    rep = (2.0, 0.5, 0.25) if exact else (1.3, 0.7, 0.4)
    params = [rep] * R
    if R >= 3:
        slots[1] = -1
        params[2] = (4.0, 0.25, 0.5) if exact else (0.8, -0.5, -1.0)
    return buf, hist, _i32(slots), _i32(lens), _i32(plens), _i32(last), ops.penalty_params(params)


def _touched(V, vstart, hist, slots, lens, last):
    """[R, V] bool: columns whose token is in the row's history."""
    m = torch.zeros(len(slots), V, dtype=torch.bool)
    for r, (s, n) in enumerate(zip(slots.tolist(), lens.tolist())):
        if s >= 0 and n > 0:
            for t in hist[s, :n - 1].tolist() + [int(last[r])]:
                if 0 <= t - vstart < V:
                    m[r, t - vstart] = True
    return m


def _ordered(x):
    """bf16 -> integers in which neighbouring values differ by 1."""
    b = x.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(b < 0, -(b & 0x7fff), b)


def _run_gpu(case, V, vstart):
    buf, hist, slots, lens, plens, last, params = case
    hd = hist.to(DEV)
    out = ops.apply_penalties(buf.to(DEV)[:, :V], hd, slots.to(DEV), lens.to(DEV), plens.to(DEV), last.to(DEV),
                              params.to(DEV), vstart=vstart)
    assert out.shape == (buf.shape[0], V) and out.dtype == torch.bfloat16
    return out.cpu(), hd.cpu()


def _check(case, V, vstart, bitwise=False):
    buf, hist, slots, lens, plens, last, params = case
    x = buf[:, :V].contiguous()
    got, hist_after = _run_gpu(case, V, vstart)
    want_hist = hist.clone()
    want = ref.apply_penalties(x, want_hist, slots, lens, plens, last, params, vstart)
    touched = _touched(V, vstart, hist, slots, lens, last)
    gb, xb = got.view(torch.int16), x.view(torch.int16)
    assert torch.equal(gb[~touched], xb[~touched])
    for r in (slots < 0).nonzero().flatten().tolist():
        assert torch.equal(gb[r], xb[r])
    if bitwise:
        assert torch.equal(gb, want.view(torch.int16))
    else:
        fin = torch.isfinite(want.float())
        assert torch.equal(got.float()[~fin], want.float()[~fin])
        assert (_ordered(got)[fin] - _ordered(want)[fin]).abs().max().item() <= 1
    assert touched.any() and (int(lens.max()) < 5 or not torch.equal(gb, xb))
    # hist[slot, len - 1] == last, and nothing else was written
    assert torch.equal(hist_after, want_hist)
    for r, (s, n) in enumerate(zip(slots.tolist(), lens.tolist())):
        if s >= 0:
            assert int(hist_after[s, n - 1]) == int(last[r])
    return got


@pytest.mark.parametrize("V", [7, 1000, 8200, 32064])
@pytest.mark.parametrize("R", [1, 3, 65])
def test_kernel_matches_reference(R, V):
    """Sizes: below one 16-B load, a ragged tail (V % 8 != 0), a full chunk plus a ragged one, a
    TP shard of a 128256 vocabulary; 65 rows. History lengths: `last` alone, a 16-B tail, one
    short of the row, the full row, and more tokens than the workgroup has threads."""
    for vstart in (0, 96192):
        for n, width in LENGTHS:
            case = _case(R, V, vstart, n, width, seed=R * 131 + V + n)
            assert case[0].stride(0) > V
            _check(case, V, vstart)


@pytest.mark.parametrize("V", [1000, 8200])
def test_exact_arithmetic_is_bitwise(V):
    """Logits k / 8 with |x| <= 16, rep = 2 (1 / rep = 0.5), freq = 0.5, pres = 0.25, counts <= 32:
    every f32 intermediate is exact, so contraction cannot change it."""
    for vstart in (0, 96192):
        for n, width in ((128, 128), (300, 304)):
            _check(_case(3, V, vstart, n, width, seed=V + n, exact=True), V, vstart, bitwise=True)


def test_history_length_zero():
    """len <= 0: the row is copied and nothing is stored."""
    buf, hist, slots, lens, plens, last, params = _case(3, 1000, 0, 5, 128, seed=4)
    lens = _i32([0, 5, -2])
    got, hist_after = _run_gpu((buf, hist, slots, lens, plens, last, params), 1000, 0)
    assert torch.equal(got.view(torch.int16), buf[:, :1000].contiguous().view(torch.int16))
    assert torch.equal(hist_after, hist)


def test_poisoned_arena(poisoned):
    """The output buffer allocated as NaN and full of garbage before the call: same results."""
    V = 8197
    case = _case(3, V, 0, 127, 128, seed=3)
    ops.set_poison(False)
    want = _check(case, V, 0)
    ops.set_poison(True)
    ops._arena.get(torch.device(DEV, torch.cuda.current_device()), "penalties", 1, torch.bfloat16).fill_(-1)
    got = _check(case, V, 0)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


def test_graph_capture():
    """The op captured; logits, slots, lens, last and params overwritten in place; the replay is
    bitwise equal to an eager call on the same inputs."""
    R, V, vstart = 4, 8200, 96192
    a = _case(R, V, vstart, 127, 128, seed=1)
    b = _case(R, V, vstart, 5, 128, seed=2)
    b[2][0] = -1                                   # another row without a slot
    dev = [t.to(DEV) for t in a]
    hist0 = b[1].to(DEV)

    def run():
        return ops.apply_penalties(dev[0][:, :V], dev[1], dev[2], dev[3], dev[4], dev[5], dev[6], vstart=vstart)

    run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = run()
    for d, src in zip(dev, b):
        d.copy_(src)
    g.replay()
    torch.cuda.synchronize()
    got, hist_got = out.clone(), dev[1].clone()
    dev[1].copy_(hist0)
    want = run()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)) and torch.equal(hist_got, dev[1])
    x = b[0][:, :V].contiguous()
    cpu = ref.apply_penalties(x, b[1].clone(), *b[2:], vstart)
    assert (_ordered(got.cpu()) - _ordered(cpu))[torch.isfinite(cpu.float())].abs().max().item() <= 1


def test_engine_graph_sampling():
    """llama-tiny, decode graphs ending in the sampler, asynchronous engine, 6 prompts, penalties
    on every other request: a plan with a penalised row samples eagerly from the graph's logits.
    The unpenalised requests' tokens equal a run without any penalty. The penalised ones pass the
    teacher-forced check with a margin: the logits of a GPU prefill over prompt + output,
    penalised by the CPU reference with the history prompt + output[:i], put output[i] within
    delta of the maximum. delta is twice the largest difference between the logits the engine
    sampled from and that prefill's logits at the same positions, measured in the run without
    penalties (a property of the decode / prefill kernels, not of the penalties).
    Measured on an MI355X: largest difference 0.0, so delta = 0.0 (at these sizes, one K tile and
    one attention chunk, the decode and prefill kernels accumulate in the same order): the
    penalised maximum itself, ties allowed."""
    cfg = ModelConfig.from_preset("llama-tiny")
    V = cfg.vocab_size
    prompts = [[i + 1, 2 * i + 3, 5] * 3 for i in range(6)]
    sp = dict(max_tokens=12, ignore_eos=True)

    def prefill_logits(eng, prompt, output):
        toks = prompt + output[:-1]
        kv = eng.model.allocate_kv_cache(len(toks) // 16 + 2, 16)
        fb = make_prefill_batch([toks], [list(range(len(toks)))])
        fb.logits_idx = torch.arange(len(prompt) - 1, len(toks), dtype=torch.int64)
        return eng.model.forward(fb.to(DEV), kv)[:, :V].cpu()

    def run(pen, check):
        eng = LLMEngine(cfg, engine_cfg=EngineConfig(max_batch=8, max_seq_len=128, kv_cache_tokens=2048,
                                                     use_graphs=True, graph_batch_sizes=[8], seed=11), device=DEV)
        assert eng.async_pp and eng.runner.sample_fn is not None
        seen: dict = {}
        sample = eng._sample

        def recording(logits, rids, *a, **kw):      # the logits each token was sampled from
            for i, r in enumerate(rids):
                seen.setdefault(r, []).append(logits[i, :V].cpu())
            return sample(logits, rids, *a, **kw)

        eng._sample = recording
        rids = [eng.add_request(p, SamplingParams(**sp, **(PEN if pen and i % 2 == 0 else {})))
                for i, p in enumerate(prompts)]
        while eng.has_unfinished_global():
            eng.step()
        outs = [eng.requests[r].output for r in rids]
        assert (eng._pen is not None) == pen and (not pen or sorted(eng._pen.free) == list(range(8)))
        res = check(eng, outs, [torch.stack(seen[r]) for r in rids])
        eng.close()
        return outs, res

    def measure(eng, outs, sampled):
        return max((s.float() - prefill_logits(eng, p, o).float()).abs().max().item()
                   for p, o, s in zip(prompts, outs, sampled))

    plain, diff = run(False, measure)
    delta = 2 * diff
    print(f"decode-versus-prefill logit difference {diff}, delta {delta}")
    params = ops.penalty_params([(PEN["repetition_penalty"], PEN["frequency_penalty"], PEN["presence_penalty"])])

    def oracle(eng, outs, sampled):
        for k in range(0, 6, 2):
            prompt, output = prompts[k], outs[k]
            logits = prefill_logits(eng, prompt, output)
            toks = prompt + output
            for i, t in enumerate(output):
                n = len(prompt) + i
                hist = _i32(toks[:n] + [0] * (-n % 4)).view(1, -1)
                pen = ref.apply_penalties(logits[i:i + 1], hist, _i32([0]), _i32([n]), _i32([len(prompt)]),
                                          _i32([toks[n - 1]]), params).float()[0]
                assert pen[t].item() >= pen.max().item() - delta, (k, i, pen[t].item(), pen.max().item(), delta)

    got, _ = run(True, oracle)
    assert all(len(o) == 12 for o in got)
    assert [got[k] for k in (1, 3, 5)] == [plain[k] for k in (1, 3, 5)]
    assert any(got[k] != plain[k] for k in (0, 2, 4)), "the penalties must change some request"
