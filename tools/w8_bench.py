#!/usr/bin/env python3
"""FP8 e4m3 weight-only GEMMs against the bf16 GEMMs on the Llama-3-70B projections, event-timed
in one process, the sides alternating, three repeats each. Weight copies rotate over > 1 GiB so
every call streams from HBM. Prints one JSON line per (shape, M, case, repeat): microseconds and
weight bytes per second (bf16 cases: 2 N K bytes, FP8 cases: N K bytes).

cases   bf16          ops.linear on the row-major bf16 weight (tuned plan table)
        bf16_packed   ops.linear with the pack_w256 copy (where the plan has a packed form)
        w8            ops.linear_w8: the native kernel up to its row limit, else the dequantise route
        w8_native     the native kernel forced above its row limit (64-row tiles), --route
        w8_sk<S>      the native kernel with a forced split-K factor, --sweep

usage: python tools/w8_bench.py [--shapes qkv,o,gate_up,down] [--m 1,16,64] [--route] [--sweep]
"""
import argparse
import json
import os
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
    ap.add_argument("--route", action="store_true", help="add the forced native kernel (row-tiled above its limit)")
    ap.add_argument("--sweep", action="store_true", help="add the native kernel with forced split-K factors")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("w8_bench: needs a GPU")
    assert ops.load_library()
    L = torch.ops.bfly
    ms = [int(m) for m in a.m.split(",")]
    ws = torch.zeros(16 * 256 * 8192 + 16, dtype=torch.float32, device="cuda")   # forced split-K slabs
    for name in a.shapes.split(","):
        N, K, e = SHAPES[name]
        epi = ops.EPILOGUES[e]
        copies = max(2, (1 << 30) // (N * K) + 1)
        Ws = [torch.randn(N, K, device="cuda", dtype=torch.bfloat16) * 0.02 for _ in range(copies)]
        Ps = [ops.pack_w256(w) for w in Ws]
        Qs = [ops.quantize_fp8(w) for w in Ws]
        ops.reserve_w8_workspace("cuda", max(ms), [(N, K)])
        for M in ms:
            x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16)
            out = torch.empty(M, N // 2 if e == "silu" else N, device="cuda", dtype=torch.bfloat16)
            cases = [("bf16", 2, lambda i: ops.linear(x, Ws[i % copies], epilogue=e, out=out)),
                     ("w8", 1, lambda i: ops.linear_w8(x, *Qs[i % copies], epilogue=e, out=out))]
            if L.gemm_packed_check(M, N, K, epi) == 0:
                cases.insert(1, ("bf16_packed", 2, lambda i: ops.linear(x, Ws[i % copies], epilogue=e, out=out,
                                                                        packed=Ps[i % copies])))
            if a.route and L.gemm_w8_check(M, N, K, epi) != 0:
                need = L.gemm_w8_workspace_size(M, N, K) // 4 + 1
                wn = torch.zeros(need, dtype=torch.float32, device="cuda")
                cases.append(("w8_native", 1, lambda i: L.gemm_w8(x, *Qs[i % copies], out, epi, wn, True)))
            if a.sweep and L.gemm_w8_check(M, N, K, epi) == 0:
                for sk in (1, 2, 4, 8, 16):
                    if sk * 4 > K // 128 or sk * M * N > ws.numel():
                        continue
                    cases.append((f"w8_sk{sk}", 1,
                                  lambda i, sk=sk: L.gemm_w8(x, *Qs[i % copies], out, epi, ws, False, sk)))
            for rep in range(a.reps):
                for tag, width, fn in cases:
                    us = timeit(fn, a.iters)
                    print(json.dumps({"shape": name, "N": N, "K": K, "M": M, "case": tag, "rep": rep,
                                      "us": round(us, 2), "TBps": round(N * K * width / us / 1e6, 3),
                                      "w8_splitk": L.gemm_w8_splitk(M, N, K, epi)}), flush=True)
        del Ws, Ps, Qs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
