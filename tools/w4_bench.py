#!/usr/bin/env python3
"""MXFP4 weight-only GEMMs against the FP8 and the bf16 GEMMs on the Llama-3-70B projections,
event-timed in one process, the sides alternating, three repeats each (tools/w8_bench.py's
method). Weight copies rotate over > 1 GiB of bf16 so every call streams from HBM. Prints one JSON
line per (shape, M, case, repeat), then one per (shape, M, case) with the median and the spread
(max - min) / median of the repeats: microseconds and weight bytes per second (bf16: 2 N K bytes,
FP8: N K + 4 N, MXFP4: N K / 2 + N K / 32).

cases   bf16          ops.linear on the row-major bf16 weight (tuned plan table)
        w8            ops.linear_w8
        w4            ops.linear_w4: the native kernel up to its row limit, else the dequantise route
        w4_native     the native kernel whatever the row count (64-row tiles), --route
        w4_deq        dequantise into a scratch + ops.linear whatever the row count, --route
        w4_sk<S>      the native kernel with a forced split-K factor, --sweep

usage: python tools/w4_bench.py [--shapes qkv,o,gate_up,down] [--m 1,16,64] [--route] [--sweep]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from butterfly_amd import ops  # noqa: E402

SHAPES = {"qkv": (10240, 8192, "none"), "o": (8192, 8192, "none"), "gate_up": (57344, 8192, "silu"),
          "down": (8192, 28672, "none")}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="qkv,o,gate_up,down")
    ap.add_argument("--m", default="1,16,64")
    ap.add_argument("--route", action="store_true", help="time both routes whatever the row limit says")
    ap.add_argument("--sweep", action="store_true", help="add the native kernel with forced split-K factors")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("w4_bench: needs a GPU")
    assert ops.load_library()
    L = torch.ops.bfly
    ms = [int(m) for m in a.m.split(",")]
    ws = torch.zeros(16 * max(ms + [256]) * 8192 + 16, dtype=torch.float32, device="cuda")   # forced split-K slabs
    for name in a.shapes.split(","):
        N, K, e = SHAPES[name]
        epi = ops.EPILOGUES[e]
        copies = max(2, (1 << 30) // (N * K) + 1)
        Ws = [torch.randn(N, K, device="cuda", dtype=torch.bfloat16) * 0.02 for _ in range(copies)]
        Q8 = [ops.quantize_fp8(w) for w in Ws]
        Q4 = [ops.quantize_mxfp4(w) for w in Ws]
        ops.reserve_w8_workspace("cuda", max(ms), [(N, K)])
        ops.reserve_w8_workspace("cuda", max(ms), [(N, K)], "mxfp4")
        scratch = torch.empty(N, K, device="cuda", dtype=torch.bfloat16) if a.route else None
        nbytes = {"bf16": 2 * N * K, "w8": N * K + 4 * N, "w4": N * K // 2 + N * K // 32}
        for M in ms:
            x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16)
            out = torch.empty(M, N // 2 if e == "silu" else N, device="cuda", dtype=torch.bfloat16)
            cases = [("bf16", "bf16", lambda i: ops.linear(x, Ws[i % copies], epilogue=e, out=out)),
                     ("w8", "w8", lambda i: ops.linear_w8(x, *Q8[i % copies], epilogue=e, out=out)),
                     ("w4", "w4", lambda i: ops.linear_w4(x, *Q4[i % copies], epilogue=e, out=out))]
            if a.route:
                need = L.gemm_w4_workspace_size(M, N, K) // 4 + 1
                wn = torch.zeros(need, dtype=torch.float32, device="cuda")

                def deq(i):
                    L.dequant_mxfp4(*Q4[i % copies], scratch)
                    ops.linear(x, scratch, epilogue=e, out=out)

                cases += [("w4_native", "w4", lambda i: L.gemm_w4(x, *Q4[i % copies], out, epi, wn, True)),
                          ("w4_deq", "w4", deq)]
            if a.sweep and L.gemm_w4_check(M, N, K, epi) == 0:
                for sk in (1, 2, 4, 8, 16):
                    if sk * 4 > K // 256 or sk * M * N > ws.numel():
                        continue
                    cases.append((f"w4_sk{sk}", "w4",
                                  lambda i, sk=sk: L.gemm_w4(x, *Q4[i % copies], out, epi, ws, False, sk)))
            times = {tag: [] for tag, _, _ in cases}
            for rep in range(a.reps):
                for tag, kind, fn in cases:
                    us = timeit(fn, a.iters)
                    times[tag].append(us)
                    print(json.dumps({"shape": name, "N": N, "K": K, "M": M, "case": tag, "rep": rep,
                                      "us": round(us, 2), "TBps": round(nbytes[kind] / us / 1e6, 3)}), flush=True)
            for tag, kind, _ in cases:
                med = statistics.median(times[tag])
                print(json.dumps({"shape": name, "M": M, "case": tag, "median_us": round(med, 2),
                                  "spread": round((max(times[tag]) - min(times[tag])) / med, 3),
                                  "TBps": round(nbytes[kind] / med / 1e6, 3),
                                  "w4_splitk": L.gemm_w4_splitk(M, N, K, epi),
                                  "w4_native": L.gemm_w4_check(M, N, K, epi) == 0}), flush=True)
        del Ws, Q8, Q4, scratch
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
