#!/usr/bin/env python3
"""Cost of the presence / frequency / repetition penalty kernel, event-timed in one process with
the sides alternating (each timing: one replay of a graph holding the calls, no host in between).

ops.apply_penalties on bf16 logits [64, 128256] and [1, 128256] with token histories of 128, 1100
and 4096 tokens per row (half of them prompt, ids uniform over the vocabulary), and with no
history at all (slot -1: the kernel's plain copy), against ops.sample (greedy) on the same logits:
the existing kernel that reads the same bytes once. The logits rotate over enough copies to exceed
the 256 MB Infinity Cache (at least 20, at least 320 MB). One JSON line per (rows, case, repeat):
microseconds, the ratio to the yardstick of that repeat, and the logits bytes read per second; a
closing summary line per (rows, case) with the median and the spread of the repeats.

usage: python tools/penalties_bench.py [--rows 64,1] [--vocab 128256] [--hist 128,1100,4096]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from butterfly_amd import ops  # noqa: E402


def timeit(fn, iters):
    """Microseconds per call of `iters` calls captured into one graph and replayed: both sides
    finish in about 10 us, less than the host needs to issue a call, so eager issue would time
    the host."""
    for i in range(3):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="64,1")
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--hist", default="128,1100,4096")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("penalties_bench: needs a GPU")
    assert ops.load_library()
    V = a.vocab
    lens = [int(h) for h in a.hist.split(",")]
    width = (max(lens) + 3) // 4 * 4
    i32 = dict(dtype=torch.int32, device="cuda")
    for R in [int(r) for r in a.rows.split(",")]:
        copies = max(20, -(-320 * 2 ** 20 // (R * V * 2)))
        lg = torch.empty(copies, R, V, dtype=torch.bfloat16, device="cuda")
        for c in range(copies):
            lg[c] = (torch.randn(R, V, device="cuda") * 4).to(torch.bfloat16)
        hist = torch.randint(0, V, (R, width), **i32)
        last = torch.randint(0, V, (R,), **i32)
        params = ops.penalty_params([(1.3, 0.7, 0.4)] * R).cuda()
        rows = torch.arange(R, **i32)

        def pen(n):
            slots = rows if n else torch.full((R,), -1, **i32)
            ln, pl = torch.full((R,), n, **i32), torch.full((R,), n // 2, **i32)
            return lambda i: ops.apply_penalties(lg[i % copies], hist, slots, ln, pl, last, params)

        cases = [("sample_greedy", lambda i: ops.sample(lg[i % copies])), ("penalties_copy", pen(0))]
        cases += [(f"penalties_h{n}", pen(n)) for n in lens]
        seen: dict = {}
        iters = max(a.iters, copies)         # a replay walks every copy at least once
        for rep in range(a.reps):
            base = None
            for tag, fn in cases:
                us = timeit(fn, iters)
                base = us if base is None else base
                seen.setdefault(tag, []).append((us, us / base))
                print(json.dumps({"rows": R, "vocab": V, "copies": copies, "case": tag, "rep": rep, "us": round(us, 2),
                                  "vs_sample": round(us / base, 2), "GBps": round(R * V * 2 / us / 1e3, 1)}),
                      flush=True)
        for tag, v in seen.items():
            us, ratio = [x for x, _ in v], [y for _, y in v]
            print(json.dumps({"summary": True, "rows": R, "case": tag, "us_median": round(statistics.median(us), 2),
                              "us_min": round(min(us), 2), "us_max": round(max(us), 2),
                              "vs_sample_median": round(statistics.median(ratio), 2),
                              "vs_sample_min": round(min(ratio), 2), "vs_sample_max": round(max(ratio), 2)}),
                  flush=True)
        del lg
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
