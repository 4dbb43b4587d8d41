"""Multi-LoRA on the CPU (reference ops, f32): the two ops against a per-element float64 loop,
a model with adapters against a model holding the merged weights W + scale B A, mixed batches,
the engine (sync / async, chunked prefill, preemption, prefix cache, snapshots), tensor
parallelism, quantised base weights, adapter files and refusals."""
import json
import math

import pytest
import torch
from safetensors.torch import save_file

from butterfly_amd.ckpt import lora as lora_ckpt
from butterfly_amd.config import EngineConfig, ModelConfig
from butterfly_amd.engine.batch import make_decode_batch, make_prefill_batch
from butterfly_amd.engine.engine import LLMEngine
from butterfly_amd.engine.sampler import SamplingParams
from butterfly_amd.models import Shard, build_model
from butterfly_amd.ops import reference as ref
from butterfly_amd.parallel.mesh import Mesh

# two f32 formulations of one model agree to this (tests/test_model_cpu.py)
ATOL = RTOL = 1e-4
TARGETS = ("attn.q_proj", "attn.k_proj", "attn.v_proj", "attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")


def target_shapes(cfg):
    """target -> (N, K) of the logical weight."""
    h, I = cfg.hidden_size, cfg.intermediate_size
    return {"attn.q_proj": (cfg.q_size, h), "attn.k_proj": (cfg.kv_size, h), "attn.v_proj": (cfg.kv_size, h),
            "attn.o_proj": (h, cfg.q_size), "mlp.gate_proj": (I, h), "mlp.up_proj": (I, h), "mlp.down_proj": (h, I)}


def make_adapter(cfg, rank, seed, amp=0.05, targets=TARGETS, layers=None):
    g = torch.Generator().manual_seed(seed)
    out = {}
    for i in (range(cfg.num_layers) if layers is None else layers):
        for t in targets:
            N, K = target_shapes(cfg)[t]
            out[f"layers.{i}.{t}.lora_A"] = torch.randn(rank, K, generator=g) * amp
            out[f"layers.{i}.{t}.lora_B"] = torch.randn(N, rank, generator=g) * amp
    return out


def merged_model(base, tensors, scale, cfg, shard=Shard(), comm=None):
    """A plain model whose weights are W + scale B A (logical tensors, sliced like the weights)."""
    m = build_model(cfg, shard, device="cpu", dtype=torch.float32, comm=comm)
    for k, v in base.p.items():
        m.p[k].copy_(v)
    for lp in m.logical_params():
        if not lp.name.endswith("_proj.weight"):
            continue
        stem = lp.name[:-len(".weight")]
        A, B = tensors.get(stem + ".lora_A"), tensors.get(stem + ".lora_B")
        if A is None:
            continue
        delta = scale * (B.double() @ A.double())
        if lp.split_dim is not None:
            delta = delta.narrow(lp.split_dim, lp.offset, lp.length)
        lp.set((lp.get().double() + delta).float())
    return m


def layout(prompts, bs=32, extra=8):
    tables, slots, nxt = [], [], 0
    for p in prompts:
        nb = (len(p) + extra + bs - 1) // bs
        tables.append(list(range(nxt, nxt + nb)))
        nxt += nb
        slots.append([tables[-1][j // bs] * bs + j % bs for j in range(len(p))])
    return tables, slots, nxt + 1


def prefill_decode(model, prompts, lora=None, bs=32):
    """(prefill logits, decode logits of the greedy next tokens) with per-sequence adapters `lora`."""
    tables, slots, nb = layout(prompts)
    kv = model.allocate_kv_cache(nb, bs)
    fb = make_prefill_batch(prompts, slots)
    if lora is not None:
        fb.lora_idx = torch.tensor([s for p, s in zip(prompts, lora) for _ in p], dtype=torch.int32)
    V = model.cfg.vocab_size
    lp = model.forward(fb, kv)[:, :V]
    toks = [int(t) for t in lp.argmax(-1)]
    pos = [len(p) for p in prompts]
    sl = [tables[i][pos[i] // bs] * bs + pos[i] % bs for i in range(len(prompts))]
    mb = max(len(t) for t in tables)
    db = make_decode_batch(toks, pos, sl, tables, mb, mb * bs)
    if lora is not None:
        db.lora_idx = torch.tensor(lora, dtype=torch.int32)
    return lp, model.forward(db, kv)[:, :V]


PROMPTS = [[3, 1, 4, 1, 5, 9, 2, 6] * 3, list(range(1, 20)), [7]]


# ---- the reference ops against a per-element float64 loop -----------------------------------------
def loop64(y, x, a, b, seg, scale, idx):
    T, N = y.shape
    S, J, K = a.shape
    R = b.shape[2]
    out = y.double().clone()
    t = torch.zeros(T, J, dtype=torch.float64)
    for m in range(T):
        s = int(idx[m])
        if not 0 <= s < S:
            continue
        for j in range(J):
            t[m, j] = sum(float(x[m, k]) * float(a[s, j, k]) for k in range(K))
        for n in range(N):
            d = sum(t[m, int(seg[n]) * R + r].item() * float(b[s, n, r]) for r in range(R))
            out[m, n] = float(y[m, n]) + float(scale[s]) * d
    return t, out


@pytest.mark.parametrize("layout_", ["one", "qkv", "gu"])
def test_reference_ops_against_float64_loop(layout_):
    g = torch.Generator().manual_seed(3)
    T, K, R, S = 7, 12, 4, 3
    n = torch.arange(48)
    seg = {"one": n * 0, "qkv": (n >= 16).long() + (n >= 32).long(), "gu": (n // 16) % 2}[layout_].to(torch.uint8)
    nseg = int(seg.max()) + 1
    x, a, b = torch.randn(T, K, generator=g), torch.randn(S, nseg * R, K, generator=g), torch.randn(S, 48, R, generator=g)
    b[1, :, 2:] = 0          # an adapter of rank 2 zero-padded to the slot rank
    a[1, 2:R] = 0
    y, scale = torch.randn(T, 48, generator=g), torch.tensor([0.5, 2.0, 1.25])
    idx = torch.tensor([0, 1, -1, 2, 3, 1, -7], dtype=torch.int32)       # -1, -7 and 3 >= S: no adapter
    tw, want = loop64(y, x, a, b, seg, scale, idx)
    t = ref.lora_shrink(x, a, idx)
    assert t.dtype == torch.float32 and torch.allclose(t.double(), tw, atol=1e-5, rtol=1e-5)
    assert bool((t[[2, 4, 6]] == 0).all())
    got = ref.lora_expand_(y.clone(), t, b, seg, scale, idx)
    assert torch.allclose(got.double(), want, atol=1e-5, rtol=1e-5)
    assert torch.equal(got[[2, 4, 6]], y[[2, 4, 6]])                    # rows without adapter: not written
    assert torch.equal(ref.lora_add_(y.clone(), x, a, b, seg, scale, idx), got)
    # rank padding changes no value: the rank-2 adapter in a table of slot rank 2
    a2, b2 = a[:, :2].clone(), b[:, :, :2].clone()
    if layout_ == "one":
        rows = idx == 1
        got2 = ref.lora_add_(y.clone(), x, a2, b2, seg, scale, idx)
        assert torch.allclose(got2[rows], got[rows], atol=1e-6, rtol=1e-6)


# ---- model -------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset", ["llama-tiny", "llama-small"])
def test_model_matches_merged_weights(preset):
    cfg = ModelConfig.from_preset(preset)
    m = build_model(cfg, device="cpu", dtype=torch.float32)
    m.init_random(7)
    m.enable_lora(2, 6)
    assert m.lora_rank == 8 and m.lora_slots == 2
    ad = make_adapter(cfg, 6, seed=1)
    m.load_lora(1, ad, scale=2.0)
    twin = merged_model(m, ad, 2.0, cfg)
    base_p, base_d = prefill_decode(m, PROMPTS)
    got_p, got_d = prefill_decode(m, PROMPTS, lora=[1, 1, 1])
    want_p, want_d = prefill_decode(twin, PROMPTS)
    for got, want, base in ((got_p, want_p, base_p), (got_d, want_d, base_d)):
        assert torch.allclose(got, want, atol=ATOL, rtol=RTOL)
        # the adapter matters: ten times the tolerance at least
        assert float((got - base).abs().max()) >= 10 * (ATOL + RTOL * float(base.abs().max()))
    # an empty slot and a cleared one are the base model
    zero_p, _ = prefill_decode(m, PROMPTS, lora=[0, 0, 0])
    assert torch.allclose(zero_p, base_p, atol=ATOL, rtol=RTOL)
    m.clear_lora(1)
    assert torch.equal(prefill_decode(m, PROMPTS, lora=[1, 1, 1])[0], zero_p)


def test_partial_targets_and_layers_stay_zero_elsewhere():
    cfg = ModelConfig.from_preset("llama-tiny")
    m = build_model(cfg, device="cpu", dtype=torch.float32)
    m.init_random(7)
    m.enable_lora(1, 8)
    ad = make_adapter(cfg, 8, seed=2, targets=("attn.k_proj", "mlp.up_proj", "mlp.down_proj"), layers=[1])
    m.load_lora(0, ad, 1.5)
    twin = merged_model(m, ad, 1.5, cfg)
    got, want = prefill_decode(m, PROMPTS, lora=[0, 0, 0]), prefill_decode(twin, PROMPTS)
    assert torch.allclose(got[0], want[0], atol=ATOL, rtol=RTOL) and torch.allclose(got[1], want[1], atol=ATOL, rtol=RTOL)
    # reloading a smaller adapter into the slot leaves nothing of the earlier one
    m.load_lora(0, make_adapter(cfg, 4, seed=3, targets=("attn.q_proj",), layers=[0]), 1.0)
    assert float(m.lora_a["l1.gu_w"].abs().max()) == 0 and float(m.lora_b["l1.down_w"].abs().max()) == 0


def test_mixed_batch_equals_single_adapter_runs():
    cfg = ModelConfig.from_preset("llama-tiny")
    m = build_model(cfg, device="cpu", dtype=torch.float32)
    m.init_random(7)
    m.enable_lora(3, 8)
    m.load_lora(0, make_adapter(cfg, 8, seed=1), 2.0)
    m.load_lora(2, make_adapter(cfg, 4, seed=2), 1.0)
    prompts = PROMPTS + [[11, 12, 13, 14]]
    mix = [0, -1, 2, 5]                                   # 5: beyond the slots = none
    got_p, got_d = prefill_decode(m, prompts, lora=mix)
    for s in (0, 2):
        one_p, one_d = prefill_decode(m, prompts, lora=[s] * 4)
        rows = [i for i, v in enumerate(mix) if v == s]
        assert torch.equal(got_p[rows], one_p[rows]) and torch.equal(got_d[rows], one_d[rows])
    base_p, base_d = prefill_decode(m, prompts)
    assert torch.equal(got_p[[1, 3]], base_p[[1, 3]]) and torch.equal(got_d[[1, 3]], base_d[[1, 3]])
    assert not torch.equal(got_p[[0, 2]], base_p[[0, 2]])


@pytest.mark.parametrize("weight_dtype", ["fp8", "mxfp4"])
def test_quantised_base_weights_with_an_adapter(weight_dtype):
    cfg = ModelConfig.from_preset("llama-tiny")
    m = build_model(cfg, device="cpu", dtype=torch.float32)
    m.init_random(7)
    plain = build_model(cfg, device="cpu", dtype=torch.float32)
    m.quantize_weights(weight_dtype)
    deq = ref.dequantize_fp8 if weight_dtype == "fp8" else ref.dequantize_mxfp4
    for k, v in m.p.items():
        plain.p[k].copy_(deq(v, m.wscale[k], torch.float32) if k in m.wscale else v)
    m.enable_lora(1, 8)
    ad = make_adapter(cfg, 8, seed=4)
    m.load_lora(0, ad, 2.0)
    twin = merged_model(plain, ad, 2.0, cfg)
    got, want = prefill_decode(m, PROMPTS, lora=[0, 0, 0]), prefill_decode(twin, PROMPTS)
    assert torch.allclose(got[0], want[0], atol=ATOL, rtol=RTOL) and torch.allclose(got[1], want[1], atol=ATOL, rtol=RTOL)


def test_model_refusals():
    for preset, word in (("mixtral-tiny", "MoE"), ("gpt2-tiny", "bias")):
        m = build_model(ModelConfig.from_preset(preset), device="cpu", dtype=torch.float32)
        with pytest.raises(ValueError, match=word):
            m.enable_lora(1, 8)
    cfg = ModelConfig.from_preset("llama-tiny")
    m = build_model(cfg, device="cpu", dtype=torch.float32)
    with pytest.raises(ValueError, match="max_rank"):
        m.enable_lora(1, 65)
    with pytest.raises(ValueError, match="enable_lora"):
        m.load_lora(0, {}, 1.0)
    m.enable_lora(2, 8)
    with pytest.raises(ValueError, match="rank 16"):
        m.load_lora(0, make_adapter(cfg, 16, seed=1), 1.0)
    bad = make_adapter(cfg, 8, seed=1)
    bad["layers.0.attn.q_proj.lora_A"] = torch.zeros(8, cfg.hidden_size + 1)
    with pytest.raises(ValueError, match="base model"):
        m.load_lora(0, bad, 1.0)
    with pytest.raises(ValueError, match="unknown adapter tensor"):
        m.load_lora(0, {"embed_tokens.lora_A": torch.zeros(8, 4)}, 1.0)
    with pytest.raises(ValueError, match="both"):
        m.load_lora(0, {"layers.0.attn.q_proj.lora_A": torch.zeros(8, cfg.hidden_size)}, 1.0)
    with pytest.raises(ValueError, match="slot"):
        m.load_lora(2, {}, 1.0)
    fb = make_prefill_batch([[1, 2]], [[-1, -1]])
    fb.lora_idx = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="enable_lora"):
        build_model(cfg, device="cpu", dtype=torch.float32).forward(fb, None)


def test_forward_batch_to_carries_lora_idx():
    fb = make_prefill_batch([[1, 2]], [[-1, -1]])
    assert fb.lora_idx is None and fb.to("cpu").lora_idx is None
    fb.lora_idx = torch.tensor([1, -1], dtype=torch.int32)
    assert torch.equal(fb.to("cpu").lora_idx, fb.lora_idx)


# ---- adapter files -----------------------------------------------------------------------------
def test_butterfly_lora_directory_round_trips(tmp_path):
    cfg = ModelConfig.from_preset("llama-tiny")
    ad = make_adapter(cfg, 4, seed=5)
    lora_ckpt.save_lora(tmp_path / "a", ad, rank=4, alpha=8.0, base_model="llama-tiny")
    got = lora_ckpt.load_lora(tmp_path / "a")
    assert got.rank == 4 and got.alpha == 8.0 and got.scale == 2.0 and got.base_model == "llama-tiny"
    assert set(got.tensors) == set(ad) and all(torch.equal(got.tensors[k], ad[k]) for k in ad)
    with pytest.raises(ValueError, match="unsupported tensor"):
        lora_ckpt.save_lora(tmp_path / "b", {"lm_head.lora_A": torch.zeros(4, 4)}, 4, 8.0)
    with pytest.raises(ValueError, match="rank"):
        lora_ckpt.save_lora(tmp_path / "c", ad, rank=8, alpha=8.0)
    with pytest.raises(FileNotFoundError):
        lora_ckpt.load_lora(tmp_path / "nothing")


def _peft_dir(path, cfg, ad, r, alpha, **extra):
    path.mkdir()
    hf = {"attn": "self_attn", "mlp": "mlp"}
    out = {}
    for k, v in ad.items():
        _, i, blk, proj, which = k.split(".")
        out[f"base_model.model.model.layers.{i}.{hf[blk]}.{proj}.{which}.weight"] = v.contiguous()
    out.update(extra.pop("tensors", {}))
    save_file(out, str(path / "adapter_model.safetensors"))
    meta = {"peft_type": "LORA", "r": r, "lora_alpha": alpha, "target_modules": ["q_proj", "v_proj"],
            "base_model_name_or_path": "some/base", **extra}
    (path / "adapter_config.json").write_text(json.dumps(meta))


def test_peft_directory_key_mapping_and_scales(tmp_path):
    cfg = ModelConfig.from_preset("llama-tiny")
    ad = make_adapter(cfg, 4, seed=6, targets=("attn.q_proj", "attn.v_proj", "mlp.down_proj"))
    _peft_dir(tmp_path / "p", cfg, ad, 4, 16)
    got = lora_ckpt.load_lora(tmp_path / "p")
    assert got.scale == 4.0 and got.rank == 4 and got.base_model == "some/base"
    assert set(got.tensors) == set(ad) and all(torch.equal(got.tensors[k], ad[k]) for k in ad)
    _peft_dir(tmp_path / "rs", cfg, ad, 4, 16, use_rslora=True)
    assert lora_ckpt.load_lora(tmp_path / "rs").scale == 16 / math.sqrt(4)
    assert lora_ckpt.peft_name("base_model.model.model.layers.3.mlp.gate_proj.lora_B.default.weight") == \
        "layers.3.mlp.gate_proj.lora_B"
    _peft_dir(tmp_path / "emb", cfg, ad, 4, 16,
              tensors={"base_model.model.model.embed_tokens.lora_embedding_A": torch.zeros(4, 8)})
    with pytest.raises(ValueError, match="unsupported tensor"):
        lora_ckpt.load_lora(tmp_path / "emb")
    _peft_dir(tmp_path / "dora", cfg, ad, 4, 16, use_dora=True)
    with pytest.raises(ValueError, match="plain LoRA"):
        lora_ckpt.load_lora(tmp_path / "dora")


# ---- engine ------------------------------------------------------------------------------------
GEN = [[(5 * i + 3 * j) % 1000 + 1 for j in range(n)] for i, n in enumerate((45, 3, 20, 33, 1, 9))]


def _ecfg(**kw):
    base = dict(max_batch=4, max_seq_len=128, kv_cache_tokens=1024, use_graphs=False, seed=5)
    base.update(kw)
    return EngineConfig(**base)


def _adapters(tmp_path, cfg):
    """Two adapter directories (one of each form) and their logical tensors / scales."""
    a, b = make_adapter(cfg, 8, seed=11), make_adapter(cfg, 4, seed=12, targets=("attn.q_proj", "attn.v_proj", "mlp.up_proj"))
    lora_ckpt.save_lora(tmp_path / "a", a, rank=8, alpha=16.0)
    _peft_dir(tmp_path / "b", cfg, b, 4, 8)
    return {"a": (a, 2.0), "b": (b, 2.0)}


def _run(eng, prompts, names, n=8):
    rids = [eng.add_request(p, SamplingParams(max_tokens=n, ignore_eos=True, lora=nm)) for p, nm in zip(prompts, names)]
    kinds = set()
    while eng.has_unfinished():
        kinds.add(eng.step().kind)
    return [eng.requests[r].output for r in rids], kinds


def _merged_outputs(cfg, ads, prompts, names, n=8, seed=5):
    """What an engine on the merged (or base) weights generates for each prompt."""
    base = build_model(cfg, device="cpu", dtype=torch.float32)
    base.init_random(seed)
    out = []
    for nm in sorted(set(names), key=str):
        model = base if nm is None else merged_model(base, ads[nm][0], ads[nm][1], cfg)
        eng = LLMEngine(cfg, engine_cfg=_ecfg(max_loras=0, prefix_caching=False), device="cpu", model=model)
        rows = [i for i, v in enumerate(names) if v == nm]
        got, _ = _run(eng, [prompts[i] for i in rows], [None] * len(rows), n)
        out.extend(zip(rows, got))
    return [o for _, o in sorted(out)]


@pytest.mark.parametrize("async_decode", [False, True])
@pytest.mark.parametrize("budget", [16, 8192])
def test_engine_mixed_adapters_match_merged_engines(tmp_path, async_decode, budget):
    cfg = ModelConfig.from_preset("llama-tiny")
    ads = _adapters(tmp_path, cfg)
    names = ["a", None, "b", "a", "b", None]
    eng = LLMEngine(cfg, engine_cfg=_ecfg(max_loras=2, max_lora_rank=8, async_decode=async_decode,
                                          max_prefill_tokens=budget), device="cpu")
    assert eng.load_lora("a", tmp_path / "a") == 0 and eng.load_lora("b", tmp_path / "b") == 1
    got, kinds = _run(eng, GEN, names)
    assert got == _merged_outputs(cfg, ads, GEN, names)
    if budget == 16:
        assert "mixed" in kinds


def test_engine_preemption_keeps_the_adapter(tmp_path):
    cfg = ModelConfig.from_preset("llama-tiny")
    ads = _adapters(tmp_path, cfg)
    prompts, names = [[i + 1] * 30 for i in range(3)], ["a", "b", None]
    # 4 blocks of 32 tokens for 3 sequences of 50: forces preemption and recompute
    eng = LLMEngine(cfg, engine_cfg=_ecfg(max_batch=3, kv_cache_tokens=128, max_loras=2, max_lora_rank=8), device="cpu")
    eng.load_lora("a", tmp_path / "a")
    eng.load_lora("b", tmp_path / "b")
    got, _ = _run(eng, prompts, names, n=20)
    assert got == _merged_outputs(cfg, ads, prompts, names, n=20)


def test_adapter_requests_bypass_the_prefix_cache(tmp_path):
    cfg = ModelConfig.from_preset("llama-tiny")
    _adapters(tmp_path, cfg)
    shared = [(13 * j) % 1000 + 1 for j in range(100)]
    eng = LLMEngine(cfg, engine_cfg=_ecfg(max_seq_len=256, max_prefill_tokens=64, kv_cache_tokens=2048, max_loras=1,
                                          max_lora_rank=8), device="cpu")
    eng.load_lora("a", tmp_path / "a")
    first, _ = _run(eng, [shared + [5, 6, 7]], ["a"], n=5)
    assert eng.scheduler.prefix_hit_tokens == 0 and eng.kv.manager.num_cached_blocks == 0    # registers no page
    plain, _ = _run(eng, [shared + [5, 6, 7]], [None], n=5)
    assert eng.scheduler.prefix_hit_tokens == 0 and eng.kv.manager.num_cached_blocks > 0
    again, _ = _run(eng, [shared + [5, 6, 7]], ["a"], n=5)                                    # takes no hit
    assert eng.scheduler.prefix_hit_tokens == 0 and again == first and first != plain
    hit, _ = _run(eng, [shared + [9]], [None], n=5)                                           # still does
    assert eng.scheduler.prefix_hit_tokens >= 64


@pytest.mark.parametrize("async_decode", [False, True])
def test_lora_enabled_engine_without_adapter_requests_is_bitwise_the_plain_engine(async_decode):
    cfg = ModelConfig.from_preset("llama-tiny")
    outs = []
    for loras in (0, 3):
        eng = LLMEngine(cfg, engine_cfg=_ecfg(max_loras=loras, async_decode=async_decode), device="cpu")
        assert bool(eng.model.lora_a) == bool(loras) and (eng.runner.lora_of is None) == (loras == 0)
        rids = [eng.add_request(p, SamplingParams(max_tokens=8, ignore_eos=True, logprobs=2, temperature=0.7, seed=i))
                for i, p in enumerate(GEN)]
        while eng.has_unfinished():
            eng.step()
        outs.append([(eng.requests[r].output, eng.requests[r].logprobs) for r in rids])
    assert outs[0] == outs[1]


def test_flag_and_config_select_the_slots(monkeypatch):
    cfg = ModelConfig.from_preset("llama-tiny")
    monkeypatch.delenv("BFLY_MAX_LORAS", raising=False)
    assert LLMEngine(cfg, engine_cfg=_ecfg(), device="cpu").max_loras == 0
    monkeypatch.setenv("BFLY_MAX_LORAS", "4")
    eng = LLMEngine(cfg, engine_cfg=_ecfg(), device="cpu")
    assert eng.max_loras == 4 and eng.model.lora_slots == 4 and eng.model.lora_rank == 16
    assert LLMEngine(cfg, engine_cfg=_ecfg(max_loras=0), device="cpu").max_loras == 0


def test_engine_refusals(tmp_path):
    cfg = ModelConfig.from_preset("llama-tiny")
    _adapters(tmp_path, cfg)
    off = LLMEngine(cfg, engine_cfg=_ecfg(max_loras=0), device="cpu")
    with pytest.raises(ValueError, match="without LoRA"):
        off.add_request([1, 2], SamplingParams(lora="a"))
    with pytest.raises(ValueError, match="without LoRA"):
        off.load_lora("a", tmp_path / "a")
    assert not off.requests
    eng = LLMEngine(cfg, engine_cfg=_ecfg(max_loras=1, max_lora_rank=4), device="cpu")
    with pytest.raises(ValueError, match="rank 8"):
        eng.load_lora("a", tmp_path / "a")
    assert not eng.loras
    eng.load_lora("b", tmp_path / "b")
    with pytest.raises(ValueError, match="already loaded"):
        eng.load_lora("b", tmp_path / "b")
    with pytest.raises(ValueError, match="slots are in use"):
        eng.load_lora("c", tmp_path / "b")
    with pytest.raises(ValueError, match="unknown LoRA adapter"):
        eng.add_request([1, 2], SamplingParams(lora="nope"))
    rid = eng.add_request([1, 2, 3], SamplingParams(max_tokens=4, ignore_eos=True, lora="b"))
    with pytest.raises(ValueError, match="in use"):
        eng.unload_lora("b")
    while eng.has_unfinished():
        eng.step()
    assert len(eng.requests[rid].output) == 4
    eng.unload_lora("b")
    assert not eng.loras and float(eng.model.lora_scale.abs().max()) == 0
    with pytest.raises(ValueError, match="unknown LoRA adapter"):
        eng.unload_lora("b")
    assert eng.load_lora("again", tmp_path / "b") == 0
    with pytest.raises(ValueError, match="pipeline"):
        LLMEngine(cfg, Mesh(pp=2), _ecfg(max_loras=1), device="cpu")
    for preset in ("mixtral-tiny", "gpt2-tiny"):
        with pytest.raises(ValueError, match="LoRA"):
            LLMEngine(ModelConfig.from_preset(preset), engine_cfg=_ecfg(max_loras=1), device="cpu")
    with pytest.raises(ValueError, match="context-parallel"):
        LLMEngine(cfg, engine_cfg=_ecfg(max_loras=1, cp_prefill_min_tokens=64), device="cpu")


def test_snapshots_carry_the_adapter_name(tmp_path):
    cfg = ModelConfig.from_preset("llama-tiny")
    ads = _adapters(tmp_path, cfg)
    names = ["a", None, "b"]
    prompts = GEN[:3]

    def engine(load=("a", "b")):
        e = LLMEngine(cfg, engine_cfg=_ecfg(max_loras=2, max_lora_rank=8, async_decode=False), device="cpu")
        for nm in load:
            e.load_lora(nm, tmp_path / nm)
        return e

    e1 = engine()
    rids = [e1.add_request(p, SamplingParams(max_tokens=10, ignore_eos=True, lora=nm)) for p, nm in zip(prompts, names)]
    for _ in range(5):
        e1.step()
    snap = json.loads(json.dumps(e1.snapshot()))
    assert [r["params"]["lora"] for r in snap["requests"]] == names
    assert any(0 < len(r["output"]) < 10 for r in snap["requests"])
    e2 = engine()
    e2.restore(snap)
    while e2.has_unfinished():
        e2.step()
    assert [e2.requests[r].output for r in rids] == _merged_outputs(cfg, ads, prompts, names, n=10)
    with pytest.raises(ValueError, match="unknown LoRA adapter 'b'"):
        engine(load=("a",)).restore(snap)
    # a snapshot written before the field existed loads as base-model requests
    for r in snap["requests"]:
        del r["params"]["lora"]
    e3 = engine(load=())
    e3.restore(snap)
    assert all(q.params.lora is None for q in e3.requests.values())


def _tp_generate(rank, world, root, tp):
    """One rank of a tp-way engine (gloo, tests/dist_utils.py) or the single-process engine."""
    from pathlib import Path

    from butterfly_amd.parallel.comm import Communicator

    cfg = ModelConfig.from_preset("llama-tiny")
    mesh = Mesh(tp=tp)
    eng = LLMEngine(cfg, mesh, _ecfg(max_loras=2, max_lora_rank=8), comm=Communicator.from_mesh(mesh) if tp > 1 else None,
                    device="cpu")
    eng.load_lora("a", Path(root) / "a")
    eng.load_lora("b", Path(root) / "b")
    if tp == 2:     # column-parallel b rows / row-parallel a columns are the local halves
        assert eng.model.lora_b["l0.qkv_w"].shape[1] == eng.model.p["l0.qkv_w"].shape[0]
        assert eng.model.lora_a["l0.down_w"].shape[2] == cfg.intermediate_size // 2
        assert eng.model.lora_a["l0.qkv_w"].shape[2] == cfg.hidden_size
    return _run(eng, GEN[:4], ["a", None, "b", "a"], n=12)[0]


def test_tensor_parallel_over_gloo_matches_single_process(tmp_path):
    from .dist_utils import run_world

    _adapters(tmp_path, ModelConfig.from_preset("llama-tiny"))
    want = _tp_generate(0, 1, str(tmp_path), 1)
    assert all(len(t) == 12 for t in want)
    for got in run_world(_tp_generate, 2, str(tmp_path), 2):
        assert got == want


# ---- Python API, HTTP server, command line --------------------------------------------------------
def _llm(tmp_path, loras=2):
    from butterfly_amd.api import LLM

    llm = LLM("llama-tiny", engine_config=EngineConfig(max_batch=4, max_seq_len=128, kv_cache_tokens=1024,
                                                       use_graphs=False, max_loras=loras, max_lora_rank=8))
    _adapters(tmp_path, llm.cfg)
    return llm


def test_llm_generate_with_an_adapter(tmp_path):
    llm = _llm(tmp_path)
    assert llm.load_lora("a", tmp_path / "a") == 0
    base = llm.generate([[5, 6, 7]], SamplingParams(max_tokens=6, ignore_eos=True))[0].token_ids
    tuned = llm.generate([[5, 6, 7]], SamplingParams(max_tokens=6, ignore_eos=True, lora="a"))[0].token_ids
    assert len(tuned) == 6 and tuned != base
    llm.unload_lora("a")
    with pytest.raises(ValueError, match="unknown LoRA adapter"):
        llm.generate([[5, 6, 7]], SamplingParams(max_tokens=6, lora="a"))


def test_http_model_field_selects_the_adapter(tmp_path):
    pytest.importorskip("fastapi")
    import threading

    from fastapi.testclient import TestClient

    from butterfly_amd.server import ServingLoop, create_app

    llm = _llm(tmp_path)
    llm.load_lora("tuned-a", tmp_path / "a")
    llm.load_lora("tuned-b", tmp_path / "b")
    loop = ServingLoop(llm)
    th = threading.Thread(target=loop.run, daemon=True)
    th.start()
    try:
        c = TestClient(create_app(loop))
        models = c.get("/v1/models").json()["data"]
        assert [m["id"] for m in models] == ["llama-tiny", "tuned-a", "tuned-b"]
        assert "parent" not in models[0] and all(m["parent"] == "llama-tiny" for m in models[1:])
        body = {"prompt": [1, 2, 3], "max_tokens": 6}
        base = c.post("/v1/completions", json=body).json()
        other = c.post("/v1/completions", json={**body, "model": "something-else"}).json()     # exactly as before
        named = c.post("/v1/completions", json={**body, "model": "llama-tiny"}).json()
        a = c.post("/v1/completions", json={**body, "model": "tuned-a"}).json()
        b = c.post("/v1/completions", json={**body, "model": "tuned-b"}).json()
        assert base["model"] == other["model"] == named["model"] == "llama-tiny"
        assert base["choices"][0]["token_ids"] == other["choices"][0]["token_ids"] == named["choices"][0]["token_ids"]
        assert a["model"] == "tuned-a" and b["model"] == "tuned-b"
        toks = [r["choices"][0]["token_ids"] for r in (base, a, b)]
        assert all(len(t) == 6 for t in toks) and toks[0] != toks[1] and toks[1] != toks[2]
        with c.stream("POST", "/v1/completions", json={**body, "model": "tuned-a", "stream": True}) as resp:
            events = [json.loads(ln[len("data: "):]) for ln in resp.iter_lines()
                      if ln.startswith("data: ") and not ln.endswith("[DONE]")]
        assert all(e["model"] == "tuned-a" for e in events)
        assert [t for e in events for t in e["choices"][0]["token_ids"]] == toks[1]
    finally:
        loop.stop = True
        th.join(timeout=30)


def test_cli_generate_with_adapters(tmp_path, capsys):
    from butterfly_amd import cli

    cfg = ModelConfig.from_preset("llama-tiny")
    _adapters(tmp_path, cfg)
    common = ["generate", "--model", "llama-tiny", "--prompt", "hello", "--max-tokens", "5", "--no-graphs",
              "--max-seq-len", "128"]

    def tokens(extra):
        assert cli.main(common + extra) == 0
        return json.loads(capsys.readouterr().out.splitlines()[0])["token_ids"]

    base = tokens([])
    lora = ["--lora", f"a={tmp_path / 'a'}", "--lora", f"b={tmp_path / 'b'}", "--max-lora-rank", "8"]
    assert tokens(lora) == base                              # loaded, not used
    tuned = tokens(lora + ["--use-lora", "a"])
    assert len(tuned) == 5 and tuned != base
    with pytest.raises(SystemExit):
        cli.main(common + ["--use-lora", "a"])
    with pytest.raises(SystemExit):
        cli.main(common + ["--lora", "no-directory"])
    assert cli.main(["info"]) == 0
    info = json.loads(capsys.readouterr().out)
    assert info["lora"]["max_rank"] == 16 and info["lora"]["slot_ranks"] == [8, 16, 32, 64]
