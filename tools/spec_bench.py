#!/usr/bin/env python
"""Speculative decoding measurements on one MI355X (results: profiles/spec/).

  (a) --what kernel: ops.attn_verify against ops.attn_prefill_paged on the same rows and against
      QN calls of ops.attn_decode; ctx in {1k, 8k}, B in {1, 16}, QN in {2, 4, 8}, bf16 and FP8
      cache, Llama-3 heads (Hq = 32 or 64 over Hkv = 8).
  (b) --what step: the eager verify step of an engine with spec_tokens = k against the graph
      decode step of the SAME engine with spec_tokens = 0, random-init weights, B in {1, 4, 16},
      k in {1, 3, 7}; the break-even acceptance per cell is (t_verify / t_decode - 1) / k: the
      fraction of the k drafts that must be accepted for the verify step to pay for itself.

Event timing, the sides of a comparison alternating inside one loop (so clock and thermal drift
hits them alike), medians over --iters rounds after --warmup. One JSON line per cell.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from butterfly_amd import ops  # noqa: E402
from butterfly_amd.config import EngineConfig, ModelConfig  # noqa: E402
from butterfly_amd.engine.engine import LLMEngine  # noqa: E402
from butterfly_amd.engine.sampler import SamplingParams  # noqa: E402

DEV = "cuda"


def alternate(fns: dict, warmup: int, iters: int) -> dict:
    """Median microseconds of each callable, timed with events, one call of each per round."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(iters):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) * 1e3)
    return {k: statistics.median(v) for k, v in times.items()}


def bench_kernel(args, out) -> None:
    D, BS, scale = 128, 32, 128 ** -0.5
    for Hq, Hkv in ((32, 8), (64, 8)):
        for fp8 in (False, True):
            for ctx in (1024, 8192):
                for B in (1, 16):
                    for QN in (2, 4, 8):
                        if QN * (Hq // Hkv) > 64:
                            continue
                        g = torch.Generator(device=DEV).manual_seed(1)
                        nblk = (ctx + QN + BS - 1) // BS
                        dt = torch.float8_e4m3fn if fp8 else torch.bfloat16
                        kc = torch.randn(B * nblk, Hkv, BS, D, device=DEV, generator=g).to(torch.bfloat16).to(dt)
                        vc = torch.randn(B * nblk, Hkv, D, BS, device=DEV, generator=g).to(torch.bfloat16).to(dt)
                        tables = torch.randperm(B * nblk, device=DEV, generator=g).to(torch.int32).view(B, nblk)
                        q = torch.randn(B, QN, Hq, D, device=DEV, generator=g).to(torch.bfloat16)
                        ctx_l = torch.full((B,), ctx, dtype=torch.int32, device=DEV)
                        qlen = torch.full((B,), QN, dtype=torch.int32, device=DEV)
                        cu = torch.arange(0, (B + 1) * QN, QN, dtype=torch.int32, device=DEV)
                        pos = (ctx - 1 + torch.arange(QN, device=DEV)).repeat(B).to(torch.int32)
                        q3 = q.view(B * QN, Hq, D)
                        o4, o3 = torch.empty_like(q), torch.empty_like(q3)
                        od = torch.empty(B, Hq, D, dtype=torch.bfloat16, device=DEV)
                        rows = [q[:, t].contiguous() for t in range(QN)]
                        lens = [ctx_l + t for t in range(QN)]

                        def verify():
                            ops.attn_verify(q, kc, vc, tables, ctx_l, qlen, scale, ctx, out=o4)

                        def paged():
                            ops.attn_prefill_paged(q3, kc, vc, tables, cu, pos, QN, scale, out=o3)

                        def decode():
                            for t in range(QN):
                                ops.attn_decode(rows[t], kc, vc, tables, lens[t], scale, ctx + QN, out=od)

                        t = alternate({"verify": verify, "paged": paged, "decode_x_qn": decode}, args.warmup, args.iters)
                        rec = dict(what="kernel", Hq=Hq, Hkv=Hkv, kv="fp8" if fp8 else "bf16", ctx=ctx, B=B, QN=QN,
                                   us={k: round(v, 2) for k, v in t.items()},
                                   paged_over_verify=round(t["paged"] / t["verify"], 3),
                                   decode_over_verify=round(t["decode_x_qn"] / t["verify"], 3))
                        print(json.dumps(rec), file=out, flush=True)
                        print(json.dumps(rec), flush=True)


class _Fixed:
    """Always proposes k tokens (their values do not change a step's cost)."""

    def propose(self, tokens, k):
        return [int(tokens[-1 - i % len(tokens)]) for i in range(k)]


def bench_step(args, out) -> None:
    for model in args.models.split(","):
        cfg = ModelConfig.from_preset(model)
        for B in (1, 4, 16):
            for k in (1, 3, 7):
                if (k + 1) * (cfg.num_heads // cfg.num_kv_heads) > 64:
                    continue
                ecfg = EngineConfig(max_batch=B, max_seq_len=args.ctx + 1024, kv_cache_tokens=B * (args.ctx + 1056),
                                    graph_batch_sizes=[B], seed=0, spec_tokens=k, spec_max_rows=B * (k + 1))
                eng = LLMEngine(cfg, engine_cfg=ecfg, device=DEV)
                prompts = [[(7 * i + j) % 1000 + 1 for j in range(args.ctx)] for i in range(B)]
                for p in prompts:
                    eng.add_request(p, SamplingParams(max_tokens=900, ignore_eos=True))
                while eng.scheduler.num_waiting or any(q.n_gen == 0 for q in eng.requests.values()):
                    eng.step()
                fixed, off = _Fixed(), type("Off", (), {"propose": lambda self, t, k: []})()
                t = {"decode": [], "verify": []}
                for it in range(args.warmup + args.iters):
                    for side, prop in (("decode", off), ("verify", fixed)):      # the same engine, alternating
                        eng.proposer = prop
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record()
                        kind = eng.step().kind
                        b.record()
                        b.synchronize()
                        assert kind == side, (kind, side)
                        if it >= args.warmup:
                            t[side].append(a.elapsed_time(b) * 1e3)
                td, tv = statistics.median(t["decode"]), statistics.median(t["verify"])
                rec = dict(what="step", model=model, B=B, k=k, ctx=args.ctx, decode_us=round(td, 1), verify_us=round(tv, 1),
                           ratio=round(tv / td, 3), break_even_acceptance=round((tv / td - 1) / k, 3))
                print(json.dumps(rec), file=out, flush=True)
                print(json.dumps(rec), flush=True)
                eng.close()
                del eng
                torch.cuda.empty_cache()


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--what", choices=["kernel", "step"], default="kernel")
    ap.add_argument("--models", default="llama3-8b,llama3-70b")
    ap.add_argument("--ctx", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default="profiles/spec/kernel_times.jsonl")
    a = ap.parse_args()
    assert torch.cuda.is_available() and ops.load_library()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "a") as out:
        (bench_kernel if a.what == "kernel" else bench_step)(a, out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
