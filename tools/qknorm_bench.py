#!/usr/bin/env python3
"""Cost of the per-head QK-norm inside the RoPE + KV-append kernel (Qwen3), event-timed in one
process with the sides alternating (each timing: one replay of a graph holding the calls, no host
in between).

ops.rope_kv with q_norm / k_norm (rope.hip, QKNORM) against the unchanged ops.rope_kv, which moves
the same bytes, at the Qwen3-32B head counts (64 Q heads, 8 KV heads, head_dim 128): T = 1, 64 and
8192 rows, a bf16 and an FP8 KV cache, from a bf16 QKV row ("plain") and from 8 split-K slabs of
the QKV GEMM ("sk8"). The row buffer is rotated in place call after call, as it comes out of the
QKV GEMM in a step: nothing is done to push it out of the caches. One JSON line per (T, cache,
form, repeat) with the microseconds of both sides and their ratio, and a closing summary line per
(T, cache, form) with the median and the spread of the repeats.

usage: python tools/qknorm_bench.py [--tokens 1,64,8192] [--sk 8] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from butterfly_amd import ops  # noqa: E402
from butterfly_amd.ops import reference as ref  # noqa: E402


def timeit(fn, iters):
    """Microseconds per call of `iters` calls captured into one graph and replayed: at decode
    sizes a call finishes in a few us, less than the host needs to issue it."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    g.replay()
    torch.cuda.synchronize()
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    st.record()
    g.replay()
    en.record()
    torch.cuda.synchronize()
    return st.elapsed_time(en) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", default="1,64,8192")
    ap.add_argument("--heads", default="64,8,128", help="Hq,Hkv,D")
    ap.add_argument("--sk", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=0, help="calls per graph (0: 200 up to 64 rows, else 20)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("qknorm_bench: needs a GPU")
    assert ops.load_library()
    Hq, Hkv, D = (int(x) for x in a.heads.split(","))
    BS, max_pos, eps = 32, 40960, 1e-6
    row = (Hq + 2 * Hkv) * D
    cos, sin = ref.rope_tables(D, max_pos, 1e6, device="cuda")
    qw = (0.25 + 1.75 * torch.rand(D, device="cuda")).to(torch.bfloat16)
    kw = (0.25 + 1.75 * torch.rand(D, device="cuda")).to(torch.bfloat16)
    for T in [int(t) for t in a.tokens.split(",")]:
        iters = a.iters or (200 if T <= 64 else 20)
        nblk = (T + BS - 1) // BS + 1
        pos = torch.randint(0, max_pos, (T,), dtype=torch.int32, device="cuda")
        slots = torch.randperm(nblk * BS, device="cuda")[:T].to(torch.int32)
        qkv = torch.randn(T, row, device="cuda").to(torch.bfloat16)
        slabs = torch.randn(a.sk, T, row, device="cuda")
        for cache in ("bf16", "fp8"):
            dt = torch.float8_e4m3fn if cache == "fp8" else torch.bfloat16
            kc = torch.zeros(nblk, Hkv, BS, D, dtype=torch.bfloat16, device="cuda").to(dt)
            vc = torch.zeros(nblk, Hkv, D, BS, dtype=torch.bfloat16, device="cuda").to(dt)
            for form in ("plain", f"sk{a.sk}"):
                src = qkv if form == "plain" else ops.Partial(slabs, torch.empty_like(qkv))
                sides = [("rope_kv", lambda: ops.rope_kv(src, pos, cos, sin, Hq, Hkv, slots, kc, vc)),
                         ("rope_qknorm_kv", lambda: ops.rope_kv(src, pos, cos, sin, Hq, Hkv, slots, kc, vc,
                                                                q_norm=qw, k_norm=kw, eps=eps))]
                seen = []
                for rep in range(a.reps):
                    us = {tag: timeit(fn, iters) for tag, fn in sides}
                    seen.append((us["rope_kv"], us["rope_qknorm_kv"]))
                    print(json.dumps({"T": T, "cache": cache, "form": form, "rep": rep, "iters": iters,
                                      "rope_kv_us": round(us["rope_kv"], 2),
                                      "rope_qknorm_kv_us": round(us["rope_qknorm_kv"], 2),
                                      "ratio": round(us["rope_qknorm_kv"] / us["rope_kv"], 3)}), flush=True)
                base, new = [x for x, _ in seen], [y for _, y in seen]
                ratio = [y / x for x, y in seen]
                print(json.dumps({"summary": True, "T": T, "cache": cache, "form": form,
                                  "rope_kv_us_median": round(statistics.median(base), 2),
                                  "rope_kv_us_min": round(min(base), 2), "rope_kv_us_max": round(max(base), 2),
                                  "rope_qknorm_kv_us_median": round(statistics.median(new), 2),
                                  "rope_qknorm_kv_us_min": round(min(new), 2), "rope_qknorm_kv_us_max": round(max(new), 2),
                                  "ratio_median": round(statistics.median(ratio), 3),
                                  "ratio_min": round(min(ratio), 3), "ratio_max": round(max(ratio), 3)}), flush=True)
        del qkv, slabs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
