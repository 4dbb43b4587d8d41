#!/usr/bin/env python3
"""sha256 digests of the weight-only decode GEMMs' outputs (FP8: ops.linear_w8, MXFP4:
ops.linear_w4) on seeded inputs: one JSON line per case. Both kernels are deterministic (fixed
split-K slab order), so two builds that compute the same thing print the same lines: run it on
each build and compare the outputs line for line (profiles/wq).

cases   every format x shape x M x epilogue (none, silu) through ops.linear_w8 / ops.linear_w4
        (M <= 256 is the native kernel on all of these shapes), then forced split-K factors 1, 2
        and 4 at (256, 4096), M = 16, through torch.ops.bfly.gemm_w8 / gemm_w4 directly.
Inputs come from seeded CPU generators; the codes are the CPU reference quantiser's.

usage: python tools/wq_digest.py > digest.jsonl
"""
import hashlib
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from butterfly_amd import ops  # noqa: E402
from butterfly_amd.ops import reference as ref  # noqa: E402

SHAPES = [(256, 256), (384, 640), (2048, 1024), (256, 4096)]
MS = [1, 5, 16, 17, 33, 64, 65, 128, 200, 256]
FORMATS = {"w8": (ref.quantize_fp8, ops.linear_w8, "gemm_w8", "gemm_w8_workspace_size"),
           "w4": (ref.quantize_mxfp4, ops.linear_w4, "gemm_w4", "gemm_w4_workspace_size")}


def sha(t):
    return hashlib.sha256(t.contiguous().cpu().view(torch.int16).numpy().tobytes()).hexdigest()


def main():
    if not torch.cuda.is_available():
        sys.exit("wq_digest: needs a GPU")
    assert ops.load_library(), ops._load_error
    L = torch.ops.bfly
    for fmt, (quant, linear, op, ws_size) in FORMATS.items():
        for N, K in SHAPES:
            g = torch.Generator(device="cpu").manual_seed(N * 7 + K)
            w = torch.randn(N, K, generator=g) / math.sqrt(K)
            w = (w * torch.logspace(-6, 6, N, base=2.0)[torch.randperm(N, generator=g)][:, None]).to(torch.bfloat16)
            code, scale = (t.cuda() for t in quant(w))
            xs = {M: torch.randn(M, K, generator=g).to(torch.bfloat16).cuda() for M in MS}
            for M in MS:
                for epi in ("none", "silu"):
                    assert getattr(L, op + "_check")(M, N, K, ops.EPILOGUES[epi]) == 0
                    y = linear(xs[M], code, scale, epilogue=epi)
                    print(json.dumps({"fmt": fmt, "N": N, "K": K, "M": M, "epi": epi, "sha256": sha(y)}), flush=True)
            if (N, K) == (256, 4096):
                M = 16
                ws = torch.zeros(4 * M * N, dtype=torch.float32, device="cuda")
                for sk in (1, 2, 4):
                    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device="cuda")
                    getattr(L, op)(xs[M], code, scale, out, 0, ws, False, sk)
                    print(json.dumps({"fmt": fmt, "N": N, "K": K, "M": M, "epi": "none", "force_sk": sk,
                                      "sha256": sha(out)}), flush=True)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
