#!/usr/bin/env python3
"""Cost of per-token logprobs, event-timed in one process with the sides alternating.

kernel (default)  ops.logprobs_partial + ops.logprobs_merge on bf16 logits [64, 128256] and
                  [1, 128256] for N = 0, 5, 20, against ops.sample (greedy) on the same logits: the
                  existing kernel that reads the same bytes once. The logits rotate over 20 copies
                  (328 MB at 64 rows, more than the 256 MB Infinity Cache). One JSON line per
                  (rows, case, repeat): microseconds, and the ratio to the yardstick of that repeat.
--step            one engine (default Llama-3-70B, one GPU, 64 sequences, decode graphs with the
                  sampler captured): --steps timed decode steps with logprobs=5 on every row against
                  none, --reps alternating runs and a closing plain run (the requests' field is switched
                  between runs; the graphs are the same, the logprobs kernels run eagerly after each
                  replay). One JSON line per run, and a summary line with each logprobs run's
                  difference from the mean of the plain runs around it (the step grows with the context).

usage: python tools/logprobs_bench.py [--rows 64,1] [--vocab 128256] [--n 0,5,20]
       python tools/logprobs_bench.py --step [--model llama3-70b] [--batch 64] [--steps 32] [--reps 3]
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


def timeit(fn, iters):
    for i in range(3):
        fn(i)
    torch.cuda.synchronize()
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    st.record()
    for i in range(iters):
        fn(i)
    en.record()
    torch.cuda.synchronize()
    return st.elapsed_time(en) / iters * 1e3


def kernel(a):
    V, copies = a.vocab, 20
    for R in [int(r) for r in a.rows.split(",")]:
        lg = [(torch.randn(R, V, device="cuda") * 4).to(torch.bfloat16) for _ in range(copies)]
        ids = torch.randint(0, V, (R,), device="cuda", dtype=torch.int32)

        def lp(n):
            def fn(i):
                rec = ops.logprobs_partial(lg[i % copies], ids, n)
                return ops.logprobs_merge(rec.view(1, R, -1))
            return fn

        cases = [("sample_greedy", lambda i: ops.sample(lg[i % copies]))]
        cases += [(f"logprobs_n{n}", lp(int(n))) for n in a.n.split(",")]
        for rep in range(a.reps):
            base = None
            for tag, fn in cases:
                us = timeit(fn, a.iters)
                base = us if base is None else base
                print(json.dumps({"rows": R, "vocab": V, "case": tag, "rep": rep, "us": round(us, 2),
                                  "vs_sample": round(us / base, 2),
                                  "GBps": round(R * V * 2 / us / 1e3, 1)}), flush=True)
        del lg
        torch.cuda.empty_cache()


def step(a):
    from butterfly_amd.config import EngineConfig, ModelConfig
    from butterfly_amd.engine.engine import LLMEngine
    from butterfly_amd.engine.sampler import SamplingParams

    cfg = ModelConfig.from_preset(a.model)
    B = a.batch
    gen = a.warmup + (2 * a.reps + 1) * (a.steps + 2) + 16
    max_seq = a.prompt_len + gen + 8
    ecfg = EngineConfig(max_batch=B, max_seq_len=max_seq, max_prefill_tokens=max(a.prompt_len, B * a.prompt_len // 4),
                        kv_cache_tokens=B * (max_seq + 32), graph_batch_sizes=[B])
    eng = LLMEngine(cfg, engine_cfg=ecfg)
    assert eng.async_pp and eng.runner.sample_fn is not None
    params = SamplingParams(max_tokens=gen, ignore_eos=True)      # shared by every request: one switch
    g = torch.Generator().manual_seed(1234)
    for _ in range(B):
        eng.add_request(torch.randint(0, cfg.vocab_size, (a.prompt_len,), generator=g).tolist(), params)
    eng.precapture_decode(B)
    streak = 0
    while eng.scheduler.num_waiting > 0 or streak < 1:
        streak = streak + 1 if eng.step().kind == "decode" else 0
    for _ in range(a.warmup):
        eng.step()
    runs = {"none": [], "logprobs5": []}
    for rep in range(a.reps + 1):
        for tag, n in (("none", None), ("logprobs5", 5))[:2 if rep < a.reps else 1]:
            params.logprobs = n
            for _ in range(2):          # the step in flight and the one applied late settle
                eng.step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                out = eng.step()
                assert out.kind == "decode" and len(out.new_tokens) == B
                assert (out.logprobs is not None) == (n is not None)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) / a.steps * 1e3
            runs[tag].append(ms)
            print(json.dumps({"model": cfg.name, "batch": B, "case": tag, "rep": rep, "steps": a.steps,
                              "ms_per_step": round(ms, 4)}), flush=True)
    params.logprobs = None
    # the context grows through the runs and the step with it (attention): every logprobs run is
    # compared with the mean of the plain runs before and after it
    none, lp5 = runs["none"], runs["logprobs5"]
    diffs = [lp5[i] - (none[i] + none[i + 1]) / 2 for i in range(a.reps)]
    print(json.dumps({"summary": True, "ms_per_step": {k: round(statistics.median(v), 4) for k, v in runs.items()},
                      "drift_ms_per_run": round((none[-1] - none[0]) / (2 * a.reps), 4),
                      "differences_ms": [round(d, 4) for d in diffs],
                      "difference_ms": round(statistics.median(diffs), 4)}), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", action="store_true", help="time whole decode steps instead of the kernels")
    ap.add_argument("--rows", default="64,1")
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--n", default="0,5,20")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--model", default="llama3-70b")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--prompt-len", type=int, default=128)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=4)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("logprobs_bench: needs a GPU")
    assert ops.load_library()
    (step if a.step else kernel)(a)


if __name__ == "__main__":
    main()
