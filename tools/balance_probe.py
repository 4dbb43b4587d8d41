#!/usr/bin/env python3
"""Is the M = 64 decode gate/up GEMM (Llama-3-70B: N = 57344 = 448 column tiles of 128, K = 8192)
bound by the uneven spread of its 448 workgroups over 256 CUs (192 CUs run two, 64 run one)?

Times the table's tile plan for the same K at N = 256 .. 512 tiles of 128 columns: if the time
tracks the tile count per CU (448 tiles as slow as 512) the kernel is bound per CU and a
balanced decomposition (stream-K over 256 workgroups) would pay; if it tracks the bytes, it
would not. Weight copies cycle through > 1 GiB so every call streams from HBM.

--mixed: the grid of two tile widths instead (gemm.hip gemm_tile_mixed_kernel): uniform 448 tiles
of 128 columns against 256 tiles of 128 plus 256 of 96 at N = 57344, on the row-major and on the
pack_w256 weight, and where the 512 workgroups of that launch shape land (tools/probes/
balance_mixed.hip records every workgroup's XCC, CU and width): the mixed grid only balances the
CUs if each ends with one wide and one narrow tile.

usage: python tools/balance_probe.py [--k 8192] [--m 64] [--mixed]
"""
import argparse
import collections
import ctypes
import json
import subprocess
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from butterfly_amd import ops  # noqa: E402


def timeit(fn, iters=20):
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


def placement(N, K, wide=128, narrow=96):
    """Launch the placement probe on the mixed grid of [N, K] and count, per CU, the widths of
    the workgroups it ran."""
    here = os.path.dirname(os.path.abspath(__file__))
    co = os.path.join(here, "probes", "balance_mixed.hsaco")
    if not os.path.exists(co):   # git-ignored build product: compile it (gfx950, no GPU needed)
        subprocess.run(["hipcc", "--genco", "--offload-arch=gfx950", "-O3", co[:-6] + ".hip", "-o", co], check=True)
    hip = ctypes.CDLL("libamdhip64.so")
    mod, fn = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipModuleLoad(ctypes.byref(mod), co.encode()) == 0
    assert hip.hipModuleGetFunction(ctypes.byref(fn), mod, b"placement") == 0
    nwide = N // (wide + narrow)
    grid = 2 * nwide
    w = torch.randn(N, K, device="cuda", dtype=torch.bfloat16)
    rec = torch.zeros(grid, 4, dtype=torch.int32, device="cuda")
    sink = torch.zeros(grid, dtype=torch.int32, device="cuda")
    vals = (ctypes.c_void_p(w.data_ptr()), ctypes.c_int(K), ctypes.c_int(nwide), ctypes.c_int(wide),
            ctypes.c_int(narrow), ctypes.c_void_p(rec.data_ptr()), ctypes.c_void_p(sink.data_ptr()))
    args = (ctypes.c_void_p * len(vals))(*[ctypes.addressof(v) for v in vals])
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = []
    for _ in range(3):
        assert hip.hipModuleLaunchKernel(fn, grid, 1, 1, 256, 1, 1, 0, stream, args, None) == 0
        torch.cuda.synchronize()
        per_cu = collections.defaultdict(list)
        for xcc, cu, width, _ in rec.cpu().tolist():
            per_cu[(xcc, cu)].append(width)
        kinds = collections.Counter("+".join(str(v) for v in sorted(ws, reverse=True)) for ws in per_cu.values())
        cols = collections.Counter(sum(ws) for ws in per_cu.values())
        out.append({"grid": grid, "cus": len(per_cu), "xccs": len({k[0] for k in per_cu}),
                    "tiles_per_cu": dict(kinds), "columns_per_cu": {str(k): v for k, v in sorted(cols.items())}})
    return out


def mixed(M, K):
    N = 57344
    silu = ops.EPILOGUES["silu"]
    nbytes = N * K * 2
    copies = max(2, (1 << 30) // nbytes + 1)
    x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16)
    out = torch.empty(M, N // 2, device="cuda", dtype=torch.bfloat16)
    bm = 16 if M <= 16 else 32 if M <= 32 else 64
    plans = {"uniform_448x128": [1, 3, 0, 2 if bm == 64 else 1, bm, 128, 1], "mixed_256x128+256x96": [8, 3, 0, 96, bm, 128, 1]}
    for layout in ("row_major", "packed"):
        Ws = [torch.randn(N, K, device="cuda", dtype=torch.bfloat16) * 0.02 for _ in range(copies)]
        if layout == "packed":
            Ws = [ops.pack_w256(w) for w in Ws]
        for rep in range(3):     # alternate the two grids
            for name, pl in plans.items():
                us = timeit(lambda i: torch.ops.bfly.gemm_with_plan(x, Ws[i % copies], out, pl, silu, None, None,
                                                                     layout == "packed"), iters=40)
                print(json.dumps({"weight": layout, "plan": name, "M": M, "N": N, "K": K, "rep": rep,
                                  "us": round(us, 2), "TBps": round(nbytes / us / 1e6, 3)}), flush=True)
        del Ws
    for row in placement(N, K):
        print(json.dumps({"placement": row}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=8192)
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--mixed", action="store_true", help="uniform 448 against mixed 512 workgroups, and their placement")
    a = ap.parse_args()
    assert ops.load_library()
    K, M = a.k, a.m
    if a.mixed:
        return mixed(M, K)
    plans = {"tile64x128_wk2": [1, 3, 0, 2, 64, 128, 1], "tile64x128_wk1": [1, 3, 0, 1, 64, 128, 1],
             "tile64x256_wk2": [1, 3, 0, 2, 64, 256, 1]}
    x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16)
    for tiles in (256, 320, 384, 448, 512, 640, 768):
        N = tiles * 128
        nbytes = N * K * 2
        copies = max(2, (1 << 30) // nbytes + 1)
        Ws = [torch.randn(N, K, device="cuda", dtype=torch.bfloat16) * 0.02 for _ in range(copies)]
        out = torch.empty(M, N // 2, device="cuda", dtype=torch.bfloat16)
        for name, pl in plans.items():
            if N % pl[5]:
                continue
            us = min(timeit(lambda i: torch.ops.bfly.gemm_with_plan(x, Ws[i % copies], out, pl, ops.EPILOGUES["silu"], None))
                     for _ in range(3))
            print(json.dumps({"plan": name, "M": M, "N": N, "K": K, "tiles": N // pl[5],
                              "tiles_per_cu": round(N / pl[5] / 256, 3), "us": round(us, 2),
                              "TBps": round(nbytes / us / 1e6, 3)}), flush=True)
        del Ws


if __name__ == "__main__":
    main()
