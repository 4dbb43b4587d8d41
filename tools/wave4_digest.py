#!/usr/bin/env python3
"""sha256 digests of what the one-wave-per-SIMD GEMM (gemm_wave4_kernel: plan kinds 6 and 7, and
the grouped MoE gate/up GEMM) writes on seeded inputs: one JSON line per case. The kernels are
deterministic (every accumulator sees a fixed MFMA order, the split-K slabs are reduced in a
fixed order), so two builds that compute the same thing print the same lines: run it on each
build (BFLY_KERNEL_LIB names the other one's library) and compare line for line
(profiles/wave4_merge).

cases   kind 6 through gemm_with_plan on test_gemm_big_tile's shapes, split-K 1-3, epilogues
        none / bias / silu; kind 7 on one shape per instantiated ring configuration (ragged M
        above one row tile, K-tiles past both rings), split-K 1 and 3; ops.moe_sparse_ffn on the
        first two test_moe_sparse_ffn_big_tile cases. With split-K the f32 slabs are hashed too.

usage: python tools/wave4_digest.py > digest.jsonl
"""
import hashlib
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from butterfly_amd import ops  # noqa: E402

BIG_SHAPES = [(600, 512, 1024), (256, 768, 192), (77, 256, 128), (1000, 1280, 4096), (300, 512, 256),
              (520, 512, 128), (257, 256, 320)]
MID4_CFGS = [(128, 128, 4, 6), (128, 128, 3, 7), (128, 128, 2, 8), (256, 128, 3, 4), (256, 128, 2, 6),
             (128, 256, 4, 3), (128, 256, 2, 4)]
MOE_CASES = [(4096, 8, 0, 512, 256, False), (3000, 8, 0, 256, 512, True)]


def bf(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).cuda()


def sha(t):
    return hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def gemm_case(plan, M, N, K, epi, b, x, w):
    sk = plan[6]
    out = torch.full((M, N // 2 if epi == "silu" else N), float("nan"), dtype=torch.bfloat16, device="cuda")
    off = torch.ops.bfly.gemm_slab_offset()
    ws = torch.zeros(off + sk * M * N, dtype=torch.float32, device="cuda")
    torch.ops.bfly.gemm_with_plan(x, w, out, plan, ops.EPILOGUES[epi], ws, b if epi == "bias" else None)
    row = {"plan": plan, "M": M, "N": N, "K": K, "epi": epi, "out": sha(out)}
    if sk > 1:
        row["slabs"] = sha(ws[off:])
    print(json.dumps(row), flush=True)


def main():
    if not torch.cuda.is_available():
        sys.exit("wave4_digest: needs a GPU")
    assert ops.load_library(), ops._load_error
    for M, N, K in BIG_SHAPES:
        x, w, b = bf(M, K, seed=60), bf(N, K, scale=1.0 / math.sqrt(K), seed=61), bf(N, seed=62)
        for epi in ("none", "bias", "silu"):
            for sk in (1, 2, 3):
                if K // 64 >= 2 * sk:
                    gemm_case([6, 0, 0, 0, 256, 256, sk], M, N, K, epi, b, x, w)
    for bm, bn, sa, sb in MID4_CFGS:
        M, N, K = bm + 9, 3 * bn, 64 * (sa + sb + 3)
        x, w, b = bf(M, K, seed=147), bf(N, K, scale=1.0 / math.sqrt(K), seed=148), bf(N, seed=149)
        for epi in ("none", "bias", "silu"):
            for sk in (1, 3):
                gemm_case([7, sa, sb, 0, bm, bn, sk], M, N, K, epi, b, x, w)
    for T, El, e0, H, F, skew in MOE_CASES:
        E, k = 8, 2
        g = torch.Generator().manual_seed(90 + T)
        p = torch.tensor([0.3, 0.25, 0.2, 0.08, 0.08, 0.0, 0.05, 0.04]) if skew else torch.full((E,), 1.0 / E)
        ids = torch.stack([torch.multinomial(p, k, replacement=False, generator=g) for _ in range(T)]).to(torch.int32)
        wt = torch.rand(T, k, generator=g)
        wt = (wt / wt.sum(1, keepdim=True)).float()
        x = bf(T, H, seed=84)
        gu = bf(El * 2 * F, H, scale=1.0 / math.sqrt(H), seed=85)
        dn = bf(H, El * F, scale=1.0 / math.sqrt(F), seed=86)
        y = ops.moe_sparse_ffn(x, ids.cuda(), wt.cuda(), gu, dn, e0, El, F)
        print(json.dumps({"moe_sparse_ffn": [T, El, e0, H, F, skew], "out": sha(y)}), flush=True)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
