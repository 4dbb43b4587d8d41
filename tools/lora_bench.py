#!/usr/bin/env python3
"""Cost of the multi-LoRA delta (lora.hip shrink + expand), event-timed in one process with the
sides alternating (each timing: one replay of a graph holding the calls, no host in between).

Kernel mode (default): the four Llama-3-70B projections (QKV [10240, 8192], O [8192, 8192],
gate/up [57344, 8192], down [8192, 28672]) at M = 1, 16, 64 and 8192 rows, slot rank 16, with 1, 4
and min(M, 16) distinct adapters in every 16-row tile. Sides: `ops.lora_add_` on the projection's
output, and `ops.linear` of the same projection (epilogue none), the GEMM the delta is added to.
Weights and adapter tables rotate over enough copies to exceed the 256 MB Infinity Cache. One
JSON line per (projection, M, adapters, repeat): microseconds of the delta, its ratio to the
linear of that repeat, and the achieved bytes per second against the bytes the shapes require
(`required_bytes`: `a` and `b` once per (tile, distinct adapter), x, the K-split partials of t
written and read once, y read and written); a summary line with medians and spread follows.

Engine mode (--engine): Llama-3-70B on one GPU, B = 64 decode steps with no adapter rows, all rows
on one adapter, and the rows spread over 8 adapters (random adapters of rank 16 written straight
into the slots), the three alternating; milliseconds per decode step, wall clock over --steps
steps after --warmup.

usage: python tools/lora_bench.py [--m 1,16,64,8192] [--reps 5]
       python tools/lora_bench.py --engine [--batch 64] [--steps 24] [--warmup 6] [--reps 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from butterfly_amd import ops  # noqa: E402

PROJECTIONS = (("qkv", 10240, 8192, 3), ("o", 8192, 8192, 1), ("gate_up", 57344, 8192, 2), ("down", 8192, 28672, 1))
R, S = 16, 16
BF = torch.bfloat16


def timeit(fn, iters):
    for i in range(2):
        fn(i)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(iters):
            fn(i)
    g.replay()
    torch.cuda.synchronize()
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    st.record()
    g.replay()
    en.record()
    torch.cuda.synchronize()
    return st.elapsed_time(en) / iters * 1e3


def required_bytes(M, N, K, nseg, distinct):
    """Bytes the delta of one call has to move (module doc)."""
    J, tiles = nseg * R, (M + 15) // 16
    ks = torch.ops.bfly.lora_splitk(M, K)
    tables = tiles * distinct * (J * K + N * R) * 2
    return tables + M * K * 2 + 2 * ks * M * J * 4 + 2 * M * N * 2


def randn_bf16(*shape):
    out = torch.empty(*shape, dtype=BF, device="cuda")
    flat = out.view(-1)
    for i in range(0, flat.numel(), 1 << 26):
        flat[i:i + (1 << 26)] = (torch.randn(min(1 << 26, flat.numel() - i), device="cuda") * 0.02).to(BF)
    return out


def kernels(a):
    ms = [int(m) for m in a.m.split(",")]
    for name, N, K, nseg in PROJECTIONS:
        J = nseg * R
        wc = max(2, -(-320 * 2 ** 20 // (N * K * 2)))
        tc = max(2, min(24, -(-320 * 2 ** 20 // (S * (J * K + N * R) * 2))))
        w = randn_bf16(wc, N, K)
        ta, tb = randn_bf16(tc, S, J, K), randn_bf16(tc, S, N, R)
        n = torch.arange(N, device="cuda")
        seg = {1: n * 0, 2: (n // 16) % 2, 3: (n >= 8192).long() + (n >= 9216).long()}[nseg].to(torch.uint8)
        scale = torch.full((S,), 2.0, device="cuda")
        for M in ms:
            x, y = randn_bf16(M, K), randn_bf16(M, N)
            out = torch.empty(M, N, dtype=BF, device="cuda")
            iters = 4 if M > 256 else 48
            seen: dict = {}
            for d in sorted({1, min(4, M), min(16, M)}):
                idx = (torch.arange(M, device="cuda") % 16 % d).to(torch.int32)
                need = required_bytes(M, N, K, nseg, d)
                for rep in range(a.reps):
                    lin = timeit(lambda i: ops.linear(x, w[i % wc], out=out), iters)
                    us = timeit(lambda i: ops.lora_add_(y, x, ta[i % tc], tb[i % tc], seg, scale, idx), iters)
                    seen.setdefault(d, []).append((us, us / lin, lin))
                    print(json.dumps({"proj": name, "N": N, "K": K, "M": M, "adapters_per_tile": d, "rep": rep,
                                      "delta_us": round(us, 2), "linear_us": round(lin, 2), "vs_linear": round(us / lin, 3),
                                      "required_MB": round(need / 1e6, 2), "GBps": round(need / us / 1e3, 1)}), flush=True)
            for d, v in seen.items():
                us, ratio, lin = ([t[i] for t in v] for i in range(3))
                print(json.dumps({"summary": True, "proj": name, "M": M, "adapters_per_tile": d,
                                  "delta_us_median": round(statistics.median(us), 2), "delta_us_min": round(min(us), 2),
                                  "delta_us_max": round(max(us), 2), "linear_us_median": round(statistics.median(lin), 2),
                                  "vs_linear_median": round(statistics.median(ratio), 3),
                                  "vs_linear_min": round(min(ratio), 3), "vs_linear_max": round(max(ratio), 3),
                                  "GBps_median": round(required_bytes(M, N, K, nseg, d) / statistics.median(us) / 1e3, 1)}),
                      flush=True)
        del w, ta, tb
        torch.cuda.empty_cache()


def engine(a):
    from butterfly_amd.config import EngineConfig, ModelConfig
    from butterfly_amd.engine.engine import LLMEngine
    from butterfly_amd.engine.sampler import SamplingParams

    cfg = ModelConfig.from_preset(a.model)
    B = a.batch
    eng = LLMEngine(cfg, engine_cfg=EngineConfig(max_batch=B, max_seq_len=a.prompt_len + 4 * (a.steps + a.warmup) + 64,
                                                 max_prefill_tokens=8192, max_loras=8, max_lora_rank=R), device="cuda")
    m = eng.model
    h, I = cfg.hidden_size, cfg.intermediate_size
    shapes = {"attn.q_proj": (cfg.q_size, h), "attn.k_proj": (cfg.kv_size, h), "attn.v_proj": (cfg.kv_size, h),
              "attn.o_proj": (h, cfg.q_size), "mlp.gate_proj": (I, h), "mlp.up_proj": (I, h), "mlp.down_proj": (h, I)}
    for slot in range(8):
        g = torch.Generator(device="cuda").manual_seed(slot)
        t = {}
        for i in range(cfg.num_layers):
            for k, (N, K) in shapes.items():
                t[f"layers.{i}.{k}.lora_A"] = torch.randn(R, K, device="cuda", generator=g) * 0.01
                t[f"layers.{i}.{k}.lora_B"] = torch.randn(N, R, device="cuda", generator=g) * 0.01
        m.load_lora(slot, t, 2.0)
        eng.loras[f"adapter-{slot}"] = slot
        del t
    sides = {"no_adapter": lambda i: None, "one_adapter": lambda i: "adapter-0", "eight_adapters": lambda i: f"adapter-{i % 8}"}
    seen: dict = {}
    n = a.steps + a.warmup
    for rep in range(a.reps):
        for tag, pick in sides.items():
            rids = [eng.add_request([(7 * i + j) % 1000 + 1 for j in range(a.prompt_len)],
                                    SamplingParams(max_tokens=n + 8, ignore_eos=True, lora=pick(i))) for i in range(B)]
            while any(eng.requests[r].n_gen < a.warmup for r in rids):
                eng.step()
            torch.cuda.synchronize()
            t0, steps = time.perf_counter(), 0
            while steps < a.steps:
                eng.step()
                steps += 1
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) / steps * 1e3
            while eng.has_unfinished():
                eng.step()
            for r in rids:
                eng.requests.pop(r, None)
            seen.setdefault(tag, []).append(ms)
            print(json.dumps({"engine": a.model, "batch": B, "case": tag, "rep": rep, "ms_per_step": round(ms, 3),
                              "lora_graphs": sorted(eng.runner.lora_graphs), "graphs": eng.runner.captured_buckets}),
                  flush=True)
    for tag, v in seen.items():
        print(json.dumps({"summary": True, "engine": a.model, "batch": B, "case": tag,
                          "ms_per_step_median": round(statistics.median(v), 3), "ms_min": round(min(v), 3),
                          "ms_max": round(max(v), 3),
                          "vs_no_adapter": round(statistics.median(v) / statistics.median(seen["no_adapter"]), 3)}), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", default="1,16,64,8192")
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--engine", action="store_true")
    ap.add_argument("--model", default="llama3-70b")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--prompt-len", type=int, default=128)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=6)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lora_bench: needs a GPU")
    assert ops.load_library()
    if a.reps is None:
        a.reps = 3 if a.engine else 5
    engine(a) if a.engine else kernels(a)


if __name__ == "__main__":
    main()
