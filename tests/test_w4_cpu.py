"""OCP MXFP4 weight-only quantisation on the CPU reference path: the format against a
per-element definition, the reference GEMM, the model / engine / tensor-parallel wiring, the
refusals and the public interfaces (GPU kernels: test_w4_gpu.py)."""
import json
import math
import threading

import pytest
import torch

from butterfly_amd import ckpt, ops
from butterfly_amd.config import EngineConfig, ModelConfig
from butterfly_amd.engine import state
from butterfly_amd.engine.batch import make_decode_batch, make_prefill_batch
from butterfly_amd.engine.engine import LLMEngine, weight_dtype
from butterfly_amd.engine.sampler import SamplingParams
from butterfly_amd.models import Shard, build_model
from butterfly_amd.ops import reference as ref
from butterfly_amd.parallel.fake import FakeWorld
from butterfly_amd.parallel.mesh import Mesh
from butterfly_amd.utils import flags

KINDS = ("qkv_w", "o_w", "gu_w", "down_w")
GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
TIES = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)
LOGIT_PROMPTS = [[3, 1, 4, 1, 5, 9, 2, 6] * 9, list(range(1, 40)), [7]]
GEN_PROMPTS = [[3, 14, 15, 92, 65], [35, 89, 79, 32, 38, 46, 26], [43], [38, 32, 79, 50, 28, 84]]


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm()).item()


def edge_blocks():
    """[6, 32] bf16 blocks (shared with test_w4_gpu.py) and the (E, magnitude codes) they must give.
    0: every tie of the grid at E = 0 (amax 6), both signs, and 7 -> 6 needs amax in [4, 8): a
       value in (6, 8) saturates
    1: all zero
    2: amax 2^-130 (a bf16 subnormal): E clamps to -125, codes 0
    3: amax near the bf16 maximum: E = 125
    4: the ties again under a scale of 2^-9
    5: amax 1.5 * 2^-127 (subnormal) = .375 * 2^-125: rounds to code 1 (.5)"""
    b = torch.zeros(6, 32, dtype=torch.float32)
    ties = torch.tensor(TIES)
    b[0, :7], b[0, 7:14], b[0, 14], b[0, 15], b[0, 16] = ties, -ties, 7.0, -7.5, 6.0
    b[2, 3], b[2, 9] = 2.0 ** -130, -(2.0 ** -131)
    b[3, 0], b[3, 1], b[3, 2] = 3.0e38, -1.0e38, 2.0 ** 125
    b[4, :7], b[4, 7:14], b[4, 20] = ties * 2.0 ** -9, -ties * 2.0 ** -9, 4.0 * 2.0 ** -9
    b[5, 0], b[5, 1] = 1.5 * 2.0 ** -127, -(2.0 ** -127)
    bb = b.to(torch.bfloat16)
    tie_codes = [0, 2, 2, 4, 4, 6, 6]
    want = {0: (0, tie_codes + tie_codes + [7, 7, 7]), 1: (0, [0] * 32), 2: (-125, [0] * 32), 3: (125, None),
            4: (-9, tie_codes + tie_codes), 5: (-125, [1, 0])}
    return bb, want


def _per_element(w):
    """The definition, one element at a time in Python floats (exact for these magnitudes)."""
    N, K = w.shape
    code = torch.zeros(N, K, dtype=torch.uint8)
    scale = torch.zeros(N, K // 32, dtype=torch.uint8)
    for n in range(N):
        for b in range(K // 32):
            blk = [float(v) for v in w[n, 32 * b:32 * b + 32].double()]
            amax = max(abs(v) for v in blk)
            E = 0 if amax == 0 else min(125, max(-125, math.frexp(amax)[1] - 1 - 2))
            scale[n, b] = E + 127
            for j, v in enumerate(blk):
                t = math.ldexp(abs(v), -E)
                best = min(range(8), key=lambda c: (abs(GRID[c] - t), c & 1))   # nearest; a tie to the even code
                code[n, 32 * b + j] = best | (8 if math.copysign(1.0, v) < 0 else 0)
    return code, scale


def _unpack(code):
    return torch.stack((code & 15, code >> 4), dim=2).view(code.shape[0], -1)


def _clear_zero_sign(c):
    return torch.where((c & 7) == 0, torch.zeros_like(c), c)


def test_format_edges():
    blocks, want = edge_blocks()
    w = blocks.view(1, -1)
    code, scale = ref.quantize_mxfp4(w)
    assert code.dtype == torch.uint8 and code.shape == (1, w.shape[1] // 2)
    assert scale.dtype == torch.uint8 and scale.shape == (1, 6)
    c = _unpack(code).view(6, 32)
    for i, (E, mags) in want.items():
        assert int(scale[0, i]) == E + 127, (i, int(scale[0, i]))
        if mags is not None:
            assert (c[i, :len(mags)] & 7).tolist() == mags, i
    assert int(scale[0, 1]) == 127 and int(code.view(6, 16)[1].sum()) == 0     # the zero block
    assert (c[0, 7:14] >> 3).tolist() == [1] * 7 and (c[0, :7] >> 3).tolist() == [0] * 7
    deq = ref.dequantize_mxfp4(code, scale).view(6, 32)
    assert deq[0, 14] == 6 and deq[0, 15] == -6 and deq[0, 16] == 6
    assert deq[3, 0] == 6 * 2.0 ** 125 and deq[5, 0] == 2.0 ** -126 and deq[5, 1] == 0
    pc, ps = _per_element(w)
    assert torch.equal(scale, ps) and torch.equal(_clear_zero_sign(_unpack(code)), _clear_zero_sign(pc))


def test_format_random():
    g = torch.Generator().manual_seed(0)
    w = torch.randn(24, 128, generator=g) / math.sqrt(128)
    w = (w * torch.logspace(-4, 4, 24 * 4, base=2.0)[torch.randperm(96, generator=g)].view(24, 4, 1)
         .expand(24, 4, 32).reshape(24, 128)).to(torch.bfloat16)
    w[5, 32:64] = 0
    code, scale = ref.quantize_mxfp4(w)
    pc, ps = _per_element(w)
    assert torch.equal(scale, ps) and torch.equal(_clear_zero_sign(_unpack(code)), _clear_zero_sign(pc))
    # nibble order: element 2 i in the low nibble of byte i
    assert torch.equal(code[:, 0] & 15, _unpack(code)[:, 0]) and torch.equal(code[:, 0] >> 4, _unpack(code)[:, 1])
    deq = ref.dequantize_mxfp4(code, scale)
    assert deq.dtype == torch.float32 and deq.shape == w.shape
    assert torch.equal(deq.to(torch.bfloat16).float(), deq)                    # exact in bf16
    assert torch.equal(ref.dequantize_mxfp4(code, scale, torch.bfloat16).float(), deq)
    lut = torch.tensor(GRID + tuple(-v for v in GRID), dtype=torch.float64)
    want = lut[_unpack(code).long()] * torch.pow(2.0, scale.double() - 127).repeat_interleave(32, dim=1)
    assert torch.equal(deq.double(), want)
    # the e2m1 half-step: .25 * 2^E below 2 * 2^E, up to 1 * 2^E at the top; saturation cannot
    # occur below amax 6 * 2^E and costs at most amax / 4
    E = torch.pow(2.0, scale.float() - 127).repeat_interleave(32, dim=1)
    assert bool(((deq - w.float()).abs() <= 2 * E).all())
    assert _rel(deq, w.float()) < 0.2
    # fixed point: quantising the dequantised weights gives the same codes and scales
    c2, s2 = ref.quantize_mxfp4(deq)
    assert torch.equal(s2, scale) and torch.equal(_clear_zero_sign(_unpack(c2)), _clear_zero_sign(_unpack(code)))
    # the public op is the reference on the CPU
    c3, s3 = ops.quantize_mxfp4(w)
    assert torch.equal(c3, code) and torch.equal(s3, scale)
    assert torch.equal(ops.dequantize_mxfp4(code, scale), deq)
    with pytest.raises(ValueError):
        ref.quantize_mxfp4(w[:, :48])


@pytest.mark.parametrize("epi", ["none", "silu"])
def test_ref_linear_w4(epi):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(37, 256, generator=g)
    w = torch.randn(128, 256, generator=g) / 16 * torch.logspace(-6, 6, 128, base=2.0)[:, None]
    code, scale = ref.quantize_mxfp4(w)
    y = ref.linear_w4(x, code, scale, epilogue=epi)
    assert torch.equal(y, ref.linear(x, ref.dequantize_mxfp4(code, scale), None, epi))
    assert y.shape == (37, 64 if epi == "silu" else 128)
    out = torch.empty_like(y)
    assert ops.linear_w4(x, code, scale, epilogue=epi, out=out) is out and torch.equal(out, y)
    with pytest.raises(ValueError):
        ref.linear_w4(x, code, scale, epilogue="bias")
    with pytest.raises(ValueError):
        ops.linear_w4(x, code, scale, epilogue="bias")


def _twin(a, cfg, shard=Shard(), comm=None, seed=7):
    """An ordinary model holding the dequantised values of quantised model `a`."""
    b = build_model(cfg, shard, device="cpu", dtype=torch.float32, comm=comm)
    b.init_random(seed)
    for name, scale in a.wscale.items():
        b.p[name].copy_(ref.dequantize_mxfp4(a.p[name], scale, torch.float32))
    for name, t in a.p.items():
        if name not in a.wscale:
            assert torch.equal(t, b.p[name])
    return b


@pytest.mark.parametrize("preset", ["llama-tiny", "llama-small"])
def test_model_wiring(preset):
    cfg = ModelConfig.from_preset(preset)
    a = build_model(cfg, device="cpu", dtype=torch.float32)
    a.init_random(7)
    full, shapes = a.local_bytes(), {k: tuple(v.shape) for k, v in a.p.items()}
    freed = a.quantize_weights("mxfp4")
    assert a.weight_dtype == "mxfp4" and a.quantize_weights("mxfp4") == 0
    assert set(a.wscale) == {f"l{i}.{k}" for i in a.layer_ids for k in KINDS}
    for name, s in a.wscale.items():
        N, K = shapes[name]
        assert a.p[name].dtype == torch.uint8 and a.p[name].shape == (N, K // 2)
        assert s.dtype == torch.uint8 and s.shape == (N, K // 32)
    assert a.w8_shapes() == sorted({shapes[k] for k in a.wscale})            # logical K, not K / 2
    assert a.p["embed"].dtype == torch.float32 and a.head_weight.dtype == torch.float32
    assert not a.defer_qkv and not a.defer_reduce and a.rowscale_rows == 0
    b = _twin(a, cfg)
    assert a.local_bytes() < b.local_bytes() == full and freed == full - a.local_bytes()
    assert a.gemm_shapes() == b.gemm_shapes()
    bs = 32
    tables, slots, nxt = [], [], 0
    for p in LOGIT_PROMPTS:
        nb = (len(p) + 8 + bs - 1) // bs
        tables.append(list(range(nxt, nxt + nb)))
        nxt += nb
        slots.append([tables[-1][j // bs] * bs + j % bs for j in range(len(p))])
    ka, kb = a.allocate_kv_cache(nxt + 1, bs), b.allocate_kv_cache(nxt + 1, bs)
    fb = make_prefill_batch(LOGIT_PROMPTS, slots)
    la, lb = a.forward(fb, ka), b.forward(fb, kb)
    V = cfg.vocab_size
    assert torch.equal(la[:, :V], lb[:, :V])              # the same f32 operations on the same values
    toks = [int(t) for t in lb[:, :V].argmax(-1)]
    pos = [len(p) for p in LOGIT_PROMPTS]
    sl = [tables[i][pos[i] // bs] * bs + pos[i] % bs for i in range(len(LOGIT_PROMPTS))]
    mb = max(len(t) for t in tables)
    db = make_decode_batch(toks, pos, sl, tables, mb, mb * bs)
    assert torch.equal(a.forward(db, ka)[:, :V], b.forward(db, kb)[:, :V])


def _ecfg(wd, **kw):
    return EngineConfig(max_batch=8, max_seq_len=128, kv_cache_tokens=2048, use_graphs=False, seed=5,
                        weight_dtype=wd, **kw)


def _gen(eng, n=12):
    return eng.generate(GEN_PROMPTS, SamplingParams(max_tokens=n, ignore_eos=True))


def test_engine(monkeypatch):
    monkeypatch.delenv("BFLY_WEIGHT_DTYPE", raising=False)
    cfg = ModelConfig.from_preset("llama-tiny")
    eng = LLMEngine(cfg, engine_cfg=_ecfg("mxfp4"), device="cpu")
    assert eng.weight_dtype == "mxfp4" and eng.model.wscale and eng.model.weight_dtype == "mxfp4"
    got = _gen(eng)
    assert all(len(t) == 12 for t in got)
    twin = _twin(eng.model, cfg, seed=5)
    eng_b = LLMEngine(cfg, engine_cfg=_ecfg("bf16"), device="cpu", model=twin)
    assert eng_b.weight_dtype == "bf16" and not eng_b.model.wscale
    assert _gen(eng_b) == got
    fp8 = LLMEngine(cfg, engine_cfg=_ecfg("fp8"), device="cpu")
    assert eng.model.local_bytes() < fp8.model.local_bytes() < eng_b.model.local_bytes()
    handed = LLMEngine(cfg, engine_cfg=_ecfg("auto"), device="cpu", model=eng.model)
    assert handed.weight_dtype == "mxfp4"                    # an already quantised model
    plain = LLMEngine(cfg, engine_cfg=_ecfg("auto"), device="cpu")
    assert plain.weight_dtype == "bf16" and not plain.model.wscale
    monkeypatch.setenv("BFLY_WEIGHT_DTYPE", "mxfp4")
    flagged = LLMEngine(cfg, engine_cfg=_ecfg("auto"), device="cpu")
    assert flagged.weight_dtype == "mxfp4" and _gen(flagged) == got
    over = LLMEngine(cfg, engine_cfg=_ecfg("bf16"), device="cpu")
    assert over.weight_dtype == "bf16" and _gen(over) == _gen(plain)
    assert weight_dtype("MXFP4") == "mxfp4" and weight_dtype("fp8") == "fp8"
    for bad in ("int4", "nvfp4", "fp4"):
        with pytest.raises(ValueError, match="weight_dtype"):
            LLMEngine(cfg, engine_cfg=_ecfg(bad), device="cpu")


def test_tensor_parallel(tmp_path):
    """TP2: a scale block lies along K and no shard splits one, so the two ranks hold exactly the
    single-process model's dequantised weights and generate its tokens."""
    torch.set_num_threads(1)
    cfg = ModelConfig.from_preset("llama-tiny")
    mesh = Mesh(tp=2)
    single = LLMEngine(cfg, engine_cfg=_ecfg("mxfp4"), device="cpu")
    want = _gen(single)
    whole = build_model(cfg, device="cpu", dtype=torch.float32)
    whole.init_random(5)
    for name, scale in single.model.wscale.items():
        whole.p[name].copy_(ref.dequantize_mxfp4(single.model.p[name], scale))
    ckpt.save(whole, tmp_path / "dequantised")

    def quantised(r, c):
        eng = LLMEngine(cfg, mesh, _ecfg("mxfp4"), comm=c, device="cpu")
        m = eng.model
        assert m.wscale and m.tp == 2
        # this rank's slices of the single-process model's dequantised weights, read from its checkpoint
        shard = Shard(tp_rank=mesh.coord(r).tp, tp_size=2, layer_start=0, layer_end=cfg.num_layers)
        b = build_model(cfg, shard, device="cpu", dtype=torch.float32, comm=c)
        ckpt.load_into(b, tmp_path / "dequantised")
        same = all(torch.equal(ref.dequantize_mxfp4(m.p[k], s), b.p[k]) for k, s in m.wscale.items())
        return _gen(eng), same

    got = FakeWorld(mesh, timeout_s=120).run(quantised)
    assert got[0][0] == got[1][0] == want
    assert got[0][1] and got[1][1]


def test_refusals(tmp_path):
    for preset, word in (("mixtral-tiny", "MoE"), ("gpt2-tiny", "bias")):
        m = build_model(ModelConfig.from_preset(preset), device="cpu", dtype=torch.float32)
        m.init_random(1)
        with pytest.raises(ValueError, match=word):
            m.quantize_weights("mxfp4")
        assert not m.wscale and m.weight_dtype == "bf16"
        with pytest.raises(ValueError):
            LLMEngine(ModelConfig.from_preset(preset), engine_cfg=_ecfg("mxfp4"), device="cpu")
    cfg = ModelConfig.from_preset("llama-tiny")
    m = build_model(cfg, device="cpu", dtype=torch.float32)
    m.init_random(1)
    for bad in ("int4", "nvfp4"):
        with pytest.raises(ValueError):
            m.quantize_weights(bad)
    # a local projection whose K is no multiple of the scale block
    keep = m.p["l0.o_w"]
    m.p["l0.o_w"] = keep[:, :-16].contiguous()
    with pytest.raises(ValueError, match="multiple of the 32"):
        m.quantize_weights("mxfp4")
    assert not m.wscale and m.p["l0.qkv_w"].dtype == torch.float32            # nothing was quantised
    m.p["l0.o_w"] = keep
    # after packing
    m.packed["l0.o_w"] = keep
    with pytest.raises(ValueError, match="pack"):
        m.quantize_weights("mxfp4")
    m.packed.clear()
    ckpt.save(m, tmp_path / "plain")
    m.quantize_weights("mxfp4")
    with pytest.raises(ValueError, match="already"):
        m.quantize_weights("fp8")
    with pytest.raises(RuntimeError, match="quantis"):
        m.logical_params()
    with pytest.raises(RuntimeError, match="quantis"):
        ckpt.save(m, tmp_path / "quantised")
    with pytest.raises(RuntimeError, match="quantis"):
        ckpt.load_into(m, tmp_path / "plain")


def test_snapshot_round_trip():
    cfg = ModelConfig.from_preset("llama-tiny")
    eng = LLMEngine(cfg, engine_cfg=_ecfg("mxfp4"), device="cpu")
    want = _gen(LLMEngine(cfg, engine_cfg=_ecfg("mxfp4"), device="cpu"), n=8)
    rids = [eng.add_request(p, SamplingParams(max_tokens=8, ignore_eos=True)) for p in GEN_PROMPTS]
    for _ in range(3):
        eng.step()
    assert 0 < len(eng.requests[rids[0]].output) < 8
    snap = json.loads(json.dumps(state.snapshot(eng)))
    fresh = LLMEngine(cfg, engine_cfg=_ecfg("mxfp4"), device="cpu")
    state.restore(fresh, snap)
    while fresh.has_unfinished_global():
        fresh.step()
    assert [fresh.requests[r].output for r in rids] == want


def test_cli_choice(capsys):
    from butterfly_amd import cli

    assert cli.main(["generate", "--model", "llama-tiny", "--max-tokens", "4", "--no-graphs", "--prompt", "abc",
                     "--weight-dtype", "mxfp4"]) == 0
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines[0]["token_ids"]) == 4
    with pytest.raises(SystemExit):
        cli.main(["generate", "--model", "llama-tiny", "--weight-dtype", "int4"])
    capsys.readouterr()
    assert cli.main(["info"]) == 0
    info = json.loads(capsys.readouterr().out)
    assert "mxfp4" in info["weight_dtypes"] and "mxfp4" in flags.FLAGS["BFLY_WEIGHT_DTYPE"].help


def test_server_reports_weight_dtype():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient

    from butterfly_amd.api import LLM
    from butterfly_amd.server import ServingLoop, create_app

    llm = LLM("llama-tiny", engine_config=EngineConfig(max_batch=4, max_seq_len=128, kv_cache_tokens=1024,
                                                       use_graphs=False, weight_dtype="mxfp4"))
    loop = ServingLoop(llm)
    th = threading.Thread(target=loop.run, daemon=True)
    th.start()
    try:
        c = TestClient(create_app(loop))
        assert c.get("/v1/models").json()["data"][0]["weight_dtype"] == "mxfp4"
        r = c.post("/v1/completions", json={"prompt": [1, 2, 3], "max_tokens": 4}).json()
        assert len(r["choices"][0]["token_ids"]) == 4
    finally:
        loop.stop = True
        th.join(timeout=30)
