"""Qwen3 dense models on the CPU: the Llama layer plus a per-head RMSNorm of Q and K in front of
RoPE (ModelConfig.qk_norm). HuggingFace import against transformers' own forward, the reference
op against a per-element float64 loop, the config mapping and its refusals, the presets, and the
wiring through checkpoints, the engine, tensor parallelism, MXFP4 weights, LoRA and the CLI.

The QK-norm weights are set to 1 + 0.5 randn wherever logits or tokens are compared: with the
ones of init_random a dropped weight would go unnoticed."""
import json
import math

import pytest
import torch

from butterfly_amd import cli, ops
from butterfly_amd.ckpt import format as ck
from butterfly_amd.ckpt.hf import convert_hf
from butterfly_amd.config import EngineConfig, ModelConfig
from butterfly_amd.engine.batch import make_prefill_batch
from butterfly_amd.engine.engine import LLMEngine
from butterfly_amd.engine.sampler import SamplingParams
from butterfly_amd.models import Shard, build_model
from butterfly_amd.models.ir import build_ir
from butterfly_amd.models.shard import local_dims
from butterfly_amd.ops import reference as ref
from butterfly_amd.parallel.mesh import Mesh
from butterfly_amd.partition import partition

from .dist_utils import run_world
from .test_lora_cpu import ATOL, RTOL, make_adapter, merged_model, prefill_decode

PROMPTS = [[3, 14, 15, 92, 65], [35, 89, 79, 32, 38, 46, 26], [43], [38, 32, 79, 50, 28, 84]]


def set_qk_norm(model, seed=1):
    """QK-norm weights 1 + 0.5 randn, the same on every rank of a layout."""
    g = torch.Generator().manual_seed(seed)
    for i in range(model.cfg.num_layers):
        for which in ("q", "k"):
            w = 1 + 0.5 * torch.randn(model.cfg.head_dim, generator=g)
            if i in model.layer_ids:
                model.p[f"l{i}.{which}_norm_w"].copy_(w)


def tiny(seed=7, **kw):
    m = build_model(ModelConfig.from_preset("qwen3-tiny"), device="cpu", dtype=torch.float32, **kw)
    m.init_random(seed)
    set_qk_norm(m)
    return m


# ---- HuggingFace parity ---------------------------------------------------------------------------
def _hf_qwen3(tie):
    transformers = pytest.importorskip("transformers")
    c = transformers.Qwen3Config(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=2,
                                 num_attention_heads=4, num_key_value_heads=2, head_dim=128,
                                 max_position_embeddings=256, rms_norm_eps=1e-6, tie_word_embeddings=tie)
    torch.manual_seed(0)
    m = transformers.Qwen3ForCausalLM(c).eval()
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for layer in m.model.layers:
            for norm in (layer.self_attn.q_norm, layer.self_attn.k_norm):
                norm.weight.copy_(1 + 0.5 * torch.randn(128, generator=g))
    return m


@pytest.mark.parametrize("tie", [False, True], ids=["untied", "tied"])
def test_hf_qwen3_parity(tmp_path, tie):
    m = _hf_qwen3(tie)
    ids = [1, 5, 9, 33, 100, 7, 250]
    m.save_pretrained(tmp_path / "hf", safe_serialization=True)
    cfg = convert_hf(tmp_path / "hf", tmp_path / "ck", dtype=torch.float32)
    ours = build_model(cfg, dtype=torch.float32)
    ck.load_into(ours, tmp_path / "ck")
    with torch.no_grad():
        want = m(torch.tensor([ids])).logits[0].float()
    fb = make_prefill_batch([ids], [[-1] * len(ids)])
    fb.logits_idx = torch.arange(len(ids))
    got = ours.forward(fb, None)[:, : cfg.vocab_size]
    print(f"max |ours - hf| {float((got - want).abs().max()):.3g}, max |hf| {float(want.abs().max()):.3g}")
    assert torch.allclose(got, want, atol=2e-4, rtol=1e-3), (got - want).abs().max()
    assert cfg.arch == "llama" and cfg.qk_norm and cfg.head_dim == 128 and cfg.tie_embeddings == tie
    assert cfg.norm_eps == 1e-6
    assert torch.equal(ours.p["l1.k_norm_w"], m.model.layers[1].self_attn.k_norm.weight.detach())


def test_ckpt_convert_cli_then_llm(tmp_path):
    """`ckpt convert-hf` of a Qwen3 directory, then what LLM(<directory>) does with it, on the CPU."""
    from butterfly_amd.ckpt import model_config

    m = _hf_qwen3(False)
    m.save_pretrained(tmp_path / "hf", safe_serialization=True)
    assert cli.main(["ckpt", "convert-hf", str(tmp_path / "hf"), str(tmp_path / "ck")]) == 0
    man = ck.read_manifest(tmp_path / "ck")
    assert man["model"]["qk_norm"] is True and "layers.0.attn.q_norm.weight" in man["tensors"]
    cfg = model_config(str(tmp_path / "ck"))
    assert cfg.qk_norm
    model = build_model(cfg, device="cpu", dtype=torch.float32)
    ck.load_into(model, tmp_path / "ck")
    want = m.model.layers[0].self_attn.q_norm.weight.detach().to(torch.bfloat16).float()       # stored as bf16
    assert torch.equal(model.p["l0.q_norm_w"], want)
    eng = LLMEngine(cfg, Mesh(), EngineConfig(max_batch=2, max_seq_len=64, kv_cache_tokens=256, use_graphs=False),
                    device="cpu", model=model)
    out = eng.generate([[1, 5, 9]], SamplingParams(max_tokens=3, ignore_eos=True))
    assert out == _greedy_by_forward(model, [[1, 5, 9]], 3)


# ---- the reference op ----------------------------------------------------------------------------
@pytest.mark.parametrize("Hq,Hkv,D", [(3, 1, 16), (4, 2, 8)])
def test_reference_op_against_float64_loop(Hq, Hkv, D):
    g = torch.Generator().manual_seed(5)
    T, BS, NB, eps = 5, 4, 3, 1e-3
    qkv = torch.randn(T, (Hq + 2 * Hkv) * D, generator=g)
    qw, kw = 1 + 0.5 * torch.randn(D, generator=g), 1 + 0.5 * torch.randn(D, generator=g)
    pos = torch.tensor([0, 3, 7, 2, 5], dtype=torch.int32)
    slots = torch.tensor([4, -1, 9, 0, -3], dtype=torch.int32)
    cos, sin = ops.rope_tables(D, 8, 10000.0, None, device="cpu")
    kc = torch.full((NB, Hkv, BS, D), 77.0)
    vc = torch.full((NB, Hkv, D, BS), 77.0)
    x = qkv.clone()
    out = ref.rope_kv(x, pos, cos, sin, Hq, Hkv, slots, kc, vc, qw, kw, eps)
    assert out is x
    want = qkv.double().clone()
    h2 = D // 2
    for t in range(T):
        for h in range(Hq + Hkv):
            w = qw if h < Hq else kw
            v = [float(qkv[t, h * D + j]) for j in range(D)]
            inv = 1.0 / math.sqrt(sum(a * a for a in v) / D + eps)
            n = [v[j] * inv * float(w[j]) for j in range(D)]
            for j in range(h2):
                c, s = float(cos[int(pos[t]), j]), float(sin[int(pos[t]), j])
                want[t, h * D + j] = n[j] * c - n[j + h2] * s
                want[t, h * D + j + h2] = n[j + h2] * c + n[j] * s
    assert torch.allclose(x.double(), want, atol=1e-5, rtol=1e-5)
    vcols = slice((Hq + Hkv) * D, None)
    assert torch.equal(x[:, vcols], qkv[:, vcols])                       # V: bitwise untouched
    assert not torch.allclose(x[:, : Hq * D], ref.rope_kv(qkv.clone(), pos, cos, sin, Hq, Hkv)[:, : Hq * D], atol=1e-2)
    written = set()
    for t in range(T):
        sl = int(slots[t])
        if sl < 0:
            continue
        b, o = sl // BS, sl % BS
        written.add((b, o))
        assert torch.equal(kc[b, :, o, :], x[t, Hq * D:(Hq + Hkv) * D].view(Hkv, D))
        assert torch.equal(vc[b, :, :, o], x[t, vcols].view(Hkv, D))
    for b in range(NB):
        for o in range(BS):
            if (b, o) not in written:                                    # slots < 0: nothing cached
                assert bool((kc[b, :, o, :] == 77).all()) and bool((vc[b, :, :, o] == 77).all())
    with pytest.raises(ValueError):
        ops.rope_kv(qkv.clone(), pos, cos, sin, Hq, Hkv, q_norm=qw)


# ---- from_hf -------------------------------------------------------------------------------------
QWEN3_8B_HF = dict(model_type="qwen3", vocab_size=151936, hidden_size=4096, intermediate_size=12288,
                   num_hidden_layers=36, num_attention_heads=32, num_key_value_heads=8, head_dim=128,
                   max_position_embeddings=40960, rms_norm_eps=1e-6, rope_theta=1000000.0,
                   tie_word_embeddings=False, attention_bias=False, use_sliding_window=False, sliding_window=None)


def test_from_hf_fields():
    c = ModelConfig.from_hf(QWEN3_8B_HF, name="qwen3-8b")
    assert c == ModelConfig.from_preset("qwen3-8b")
    new = dict(QWEN3_8B_HF, rope_parameters={"rope_theta": 5e6, "rope_type": "default"}, tie_word_embeddings=True)
    del new["rope_theta"]
    c = ModelConfig.from_hf(new)
    assert c.rope_theta == 5e6 and c.rope_scaling is None and c.tie_embeddings and c.qk_norm and c.arch == "llama"
    # head_dim is read, not derived: Qwen3-0.6B has 16 heads of 128 on a hidden size of 1024
    assert ModelConfig.from_hf(dict(QWEN3_8B_HF, hidden_size=1024, num_attention_heads=16)).head_dim == 128
    assert ModelConfig.from_dict(c.to_dict()) == c


def test_from_hf_refusals():
    with pytest.raises(ValueError, match="attention_bias"):
        ModelConfig.from_hf(dict(QWEN3_8B_HF, attention_bias=True))
    with pytest.raises(ValueError, match="attention_bias"):
        ModelConfig.from_hf(dict(QWEN3_8B_HF, model_type="llama", attention_bias=True))
    with pytest.raises(ValueError, match="mlp_bias"):
        ModelConfig.from_hf(dict(QWEN3_8B_HF, model_type="llama", mlp_bias=True))
    with pytest.raises(ValueError, match="use_sliding_window"):
        ModelConfig.from_hf(dict(QWEN3_8B_HF, use_sliding_window=True, sliding_window=4096))


def test_llama_config_imports_as_before():
    hf = dict(model_type="llama", vocab_size=128256, hidden_size=4096, intermediate_size=14336, num_hidden_layers=32,
              num_attention_heads=32, num_key_value_heads=8, max_position_embeddings=8192, rms_norm_eps=1e-5,
              rope_theta=500000.0, attention_bias=False, mlp_bias=False)
    assert ModelConfig.from_hf(hf, name="llama3-8b") == ModelConfig.from_preset("llama3-8b")
    assert not ModelConfig.from_hf(dict(hf, model_type="mistral")).qk_norm
    gpt2 = ModelConfig.from_hf(dict(model_type="gpt2", vocab_size=50257, n_embd=768, n_layer=12, n_head=12, n_positions=1024))
    assert gpt2.bias and not gpt2.qk_norm


def test_convert_refuses_an_unmapped_tensor(tmp_path):
    from safetensors.torch import save_file

    cfg = ModelConfig.from_preset("qwen3-tiny")
    hf = dict(model_type="qwen3", vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size,
              intermediate_size=cfg.intermediate_size, num_hidden_layers=cfg.num_layers,
              num_attention_heads=cfg.num_heads, num_key_value_heads=cfg.num_kv_heads, head_dim=cfg.head_dim)
    for sub, model_type in (("q", "qwen3"), ("l", "llama")):
        d = tmp_path / sub
        d.mkdir()
        (d / "config.json").write_text(json.dumps(dict(hf, model_type=model_type)))
        save_file({"model.norm.weight": torch.ones(cfg.hidden_size),
                   "model.layers.0.self_attn.q_norm.weight": torch.ones(cfg.head_dim),
                   "model.layers.0.self_attn.q_proj.bias": torch.ones(cfg.q_size)}, str(d / "model.safetensors"))
    with pytest.raises(ValueError, match="q_proj.bias"):
        convert_hf(tmp_path / "q", tmp_path / "q_out")
    convert_hf(tmp_path / "l", tmp_path / "l_out")          # other model types drop it, as before


# ---- presets --------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset,published", [("qwen3-8b", 6.95e9), ("qwen3-32b", 31.2e9)])
def test_preset_parameter_counts(preset, published):
    c = ModelConfig.from_preset(preset)
    non_embedding = c.param_count() - 2 * c.vocab_size * c.hidden_size
    assert abs(non_embedding - published) / published < 5e-3, non_embedding
    assert c.qk_norm and not c.tie_embeddings and c.head_dim == 128 and c.max_position == 40960
    plain = ModelConfig.from_preset(preset, qk_norm=False)
    assert c.layer_params() - plain.layer_params() == 2 * c.head_dim
    for tp in (1, 2, 4, 8):
        d = local_dims(c, Shard(tp_rank=tp - 1, tp_size=tp, layer_start=0, layer_end=c.num_layers))
        assert d.hq == c.num_heads // tp and d.hkv == c.num_kv_heads // tp and d.ffn == c.intermediate_size // tp
        ir = build_ir(c, tp=tp)
        assert ir.layers[0].op("rope_kv").param_elems == 2 * c.head_dim
    pad = 2 * (build_ir(c).head[-1].n - c.vocab_size) * c.hidden_size
    assert build_ir(c).param_elems == c.param_count() + pad


@pytest.mark.skipif(not ops.load_library(), reason="kernel library not built")
@pytest.mark.parametrize("preset", ["qwen3-8b", "qwen3-32b"])
@pytest.mark.parametrize("tp", [1, 2, 4, 8])
def test_every_gemm_plan_is_instantiated(preset, tp):
    from .test_gemm_plans import model_shapes

    Ms = list(range(1, 130)) + [160, 192, 255, 256, 300, 512, 1000, 1024, 2048, 4096, 8192, 16384]
    shapes = model_shapes(preset, tp)
    assert len(shapes) == 5
    for N, K, epi in shapes:
        assert N % 128 == 0 and K % 64 == 0, (N, K)
        for M in Ms:
            assert torch.ops.bfly.gemm_check(M, N, K, epi) == 0, (preset, tp, M, N, K, epi)


# ---- wiring ---------------------------------------------------------------------------------------
def _globals(m):
    return {lp.name: lp.get().clone() for lp in m.logical_params() if lp.owner}


def test_init_random_sets_ones_and_tp_ranks_hold_whole_weights():
    cfg = ModelConfig.from_preset("qwen3-tiny")
    m = build_model(cfg, Shard(tp_rank=1, tp_size=2), dtype=torch.float32)
    m.init_random(3)
    for i in range(cfg.num_layers):
        for which in ("q", "k"):
            assert torch.equal(m.p[f"l{i}.{which}_norm_w"], torch.ones(cfg.head_dim))
    names = {lp.name: lp for lp in m.logical_params()}
    lp = names["layers.1.attn.k_norm.weight"]
    assert lp.split_dim is None and lp.global_shape == (cfg.head_dim,) and not lp.owner       # rank 0 writes it
    stage = build_model(cfg, Shard(layer_start=1, layer_end=2), dtype=torch.float32)
    assert "l1.q_norm_w" in stage.p and "l0.q_norm_w" not in stage.p
    assert "l0.q_norm_w" not in build_model(ModelConfig.from_preset("llama-tiny"), dtype=torch.float32).p


def test_checkpoint_roundtrip_and_reshard(tmp_path):
    cfg = ModelConfig.from_preset("qwen3-tiny")
    m = build_model(cfg, dtype=torch.bfloat16)
    m.init_random(seed=2)
    set_qk_norm(m)
    want = _globals(m)
    assert "layers.0.attn.q_norm.weight" in want and "layers.1.attn.k_norm.weight" in want
    ck.save(m, tmp_path / "a", dtype=torch.bfloat16)
    ck.reshard(tmp_path / "a", tmp_path / "b", partition(cfg, 2, {"tp": 2}, batch_per_gpu=4, ctx=64))     # tp1 -> tp2
    assert ck.read_manifest(tmp_path / "b")["plan"]["tp"] == 2
    for r in range(2):
        part = build_model(cfg, Shard(tp_rank=r, tp_size=2), dtype=torch.bfloat16)
        ck.load_into(part, tmp_path / "b")
        for i in range(cfg.num_layers):
            for which in ("q", "k"):
                assert torch.equal(part.p[f"l{i}.{which}_norm_w"], m.p[f"l{i}.{which}_norm_w"])
    ck.reshard(tmp_path / "b", tmp_path / "c", partition(cfg, 1, {"tp": 1}, batch_per_gpu=4, ctx=64))     # tp2 -> tp1
    back = build_model(cfg, dtype=torch.bfloat16)
    ck.load_into(back, tmp_path / "c")
    got = _globals(back)
    assert got.keys() == want.keys()
    for k, v in want.items():
        assert torch.equal(v, got[k]), k


def _greedy_by_forward(model, prompts, n):
    """Greedy continuation with the bare model: every step a prefill of the whole sequence, no cache."""
    outs = []
    for p in prompts:
        seq = list(p)
        for _ in range(n):
            fb = make_prefill_batch([seq], [[-1] * len(seq)])
            seq.append(int(model.forward(fb, None)[0, : model.cfg.vocab_size].argmax()))
        outs.append(seq[len(p):])
    return outs


@pytest.mark.parametrize("async_decode", [False, True], ids=["sync", "async"])
def test_engine_reproduces_greedy_forward(async_decode):
    m = tiny()
    want = _greedy_by_forward(m, PROMPTS, 6)
    plain = build_model(ModelConfig.from_preset("llama-tiny"), device="cpu", dtype=torch.float32)
    plain.init_random(7)
    assert _greedy_by_forward(plain, PROMPTS, 6) != want               # the norm weights matter
    ecfg = EngineConfig(max_batch=8, max_seq_len=128, kv_cache_tokens=2048, use_graphs=False, seed=7,
                        async_decode=async_decode)
    eng = LLMEngine(m.cfg, Mesh(), ecfg, device="cpu", model=m)
    assert eng.generate(PROMPTS, SamplingParams(max_tokens=6, ignore_eos=True)) == want


def _tp_generate(rank, world, mesh_kw):
    from butterfly_amd.parallel.comm import Communicator

    mesh = Mesh(**mesh_kw)
    comm = Communicator.from_mesh(mesh) if world > 1 else None
    ecfg = EngineConfig(max_batch=8, max_seq_len=128, kv_cache_tokens=2048, use_graphs=False, seed=5)
    eng = LLMEngine(ModelConfig.from_preset("qwen3-tiny"), mesh, ecfg, comm=comm, device="cpu")
    set_qk_norm(eng.model)
    return eng.generate(PROMPTS, SamplingParams(max_tokens=6, ignore_eos=True))


def test_tensor_parallel_over_gloo_matches_single_process():
    want = _tp_generate(0, 1, {})
    for out in run_world(_tp_generate, 2, dict(tp=2)):
        assert out == want


def test_mxfp4_weights_match_dequantised_twin():
    a = tiny()
    a.quantize_weights("mxfp4")
    assert set(a.wscale) == {f"l{i}.{k}" for i in a.layer_ids for k in ("qkv_w", "o_w", "gu_w", "down_w")}
    b = build_model(a.cfg, device="cpu", dtype=torch.float32)
    for name, t in a.p.items():           # an ordinary model holding the dequantised values
        b.p[name].copy_(ref.dequantize_mxfp4(t, a.wscale[name], torch.float32) if name in a.wscale else t)
    la, da = prefill_decode(a, PROMPTS)
    lb, db = prefill_decode(b, PROMPTS)
    assert torch.equal(la, lb) and torch.equal(da, db)          # the same f32 operations on the same values


def test_lora_request_matches_merged_weights():
    m = tiny()
    m.enable_lora(2, 6)
    ad = make_adapter(m.cfg, 6, seed=1)
    m.load_lora(1, ad, scale=2.0)
    twin = merged_model(m, ad, 2.0, m.cfg)          # copies every tensor of m, then merges the projections
    base_p, base_d = prefill_decode(m, PROMPTS)
    got_p, got_d = prefill_decode(m, PROMPTS, lora=[1, 1, 1, 1])
    want_p, want_d = prefill_decode(twin, PROMPTS)
    for got, want, base in ((got_p, want_p, base_p), (got_d, want_d, base_d)):
        assert torch.allclose(got, want, atol=ATOL, rtol=RTOL)
        assert float((got - base).abs().max()) >= 10 * (ATOL + RTOL * float(base.abs().max()))


def test_cli_partition_and_generate(capsys):
    assert cli.main(["partition", "--model", "qwen3-32b", "--gpus", "8"]) == 0
    plan = json.loads(capsys.readouterr().out)
    assert plan["model"]["qk_norm"] is True and plan["tp"] * plan["pp"] * plan["dp"] == 8
    assert cli.main(["generate", "--model", "qwen3-tiny", "--max-tokens", "4", "--no-graphs", "--prompt", "Hello"]) == 0
