#!/usr/bin/env python3
"""Record what the GEMM host dispatcher (csrc/kernels/gemm.hip) decides, without a GPU.

    python tools/dump_gemm_plans.py            # rewrite tests/golden/gemm_plans.json
    python tools/dump_gemm_plans.py --emit     # this process's environment only, JSON on stdout

tests/test_gemm_plan_golden.py re-derives the same data and compares it with the fixture, so a
change of the planner or of plan validation that was not meant shows up as a diff of the file.
Re-record it only with a change that is meant to move a plan (a new table row, a new kernel).

The environment switches of gemm.hip are parsed once per process, so every variant in VARIANTS
is dumped by a fresh child process started with that environment.
"""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "gemm_plans.json")

# token counts: the edges of the planner's buckets (1, 16, 32, 64, 128, 256, 512) and of its tiles
MS = [1, 2, 4, 5, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 511, 512, 513,
      1024, 4100, 8192]
PRESETS = [("llama3-70b", 1), ("llama3-70b", 2), ("llama3-70b", 8), ("llama3-8b", 1), ("llama3-8b", 4),
           ("mixtral-8x7b", 1), ("gpt2-small", 1), ("llama-small", 1), ("llama-tiny", 1)]
VARIANTS = {
    "default": {},
    "tuned_off": {"BFLY_GEMM_TUNED": "0"},
    "mixed_off": {"BFLY_GEMM_MIXED_TILES": "0"},
    "mixed_all": {"BFLY_GEMM_MIXED_TILES": "2"},
    "plan_override": {"BFLY_GEMM_PLAN": "8192,8192,64:1,3,0,2,64,128,8;57344,8192,64:3,4,8,8,128,224,1"},
}
SWITCHES = ("BFLY_GEMM_TUNED", "BFLY_GEMM_MIXED_TILES", "BFLY_GEMM_PLAN")

# Plans below are [kind, mt, nt, wk, bm, bn, sk], the order of gemm_plan_check / gemm_with_plan.
# kPackedTuned of gemm.hip (its "keep row-major" rows carry no plan).
PACKED_TUNED = [(8192, 8192, 64, [1, 3, 1, 2, 64, 128, 4]), (57344, 8192, 64, [8, 3, 0, 96, 64, 128, 1])]
# tests/test_gemm_mixed_tiles_gpu.py::test_shapes_without_a_width_solution_are_refused
REFUSAL = [(64, 1792, 192, [8, 3, 0, 96, 64, 128, 1]), (64, 1792 + 32, 192, [8, 3, 0, 96, 64, 128, 1]),
           (64, 7 * 224, 192, [8, 3, 0, 96, 64, 128, 1]), (64, 240 * 8, 192, [8, 3, 0, 112, 64, 128, 1]),
           (64, 1792, 192, [8, 3, 0, 96, 64, 128, 4])]
# One instantiated plan per kind with a token count it takes; 2 (retired) and 9 (never existed)
# show what an unknown kind does. N = 17920 is a multiple of every tile width (256, 224, 160, 128, 80).
BASE = [(17, [0, 2, 2, 4, 0, 0, 1]), (64, [1, 3, 0, 2, 64, 128, 2]), (100, [3, 4, 8, 8, 128, 224, 1]),
        (300, [4, 0, 0, 0, 256, 256, 1]), (200, [5, 3, 0, 0, 128, 128, 2]), (300, [6, 0, 0, 0, 256, 256, 1]),
        (200, [7, 4, 6, 0, 128, 128, 2]), (64, [8, 3, 0, 96, 64, 128, 1]), (64, [2, 3, 0, 2, 64, 128, 1]),
        (64, [9, 3, 0, 2, 64, 128, 1])]
BASE_N, BASE_K = 17920, 1024
# a value no kernel is instantiated for, per field (mt, nt, wk, bm, bn); none of them is zero, the
# checks divide by some of these fields
BOGUS = {1: 7, 2: 7, 3: 3, 4: 48, 5: 48}


def shapes():
    sys.path.insert(0, ROOT)
    from tests.test_gemm_plans import model_shapes

    seen = []
    for preset, tp in PRESETS:
        for s in model_shapes(preset, tp):
            if s not in seen:
                seen.append(s)
    return [list(s) for s in seen]


def explicit_plans():
    """(M, N, K, plan) cases of the plan-check grid, each once."""
    cases = []
    for ln in open(os.path.join(ROOT, "csrc", "kernels", "gemm_tuned.inc")):
        m = re.match(r"\{" + ", ".join([r"(\d+)"] * 10) + r"\}", ln)
        if m:
            v = [int(x) for x in m.groups()]
            cases.append((v[2], v[0], v[1], v[3:]))
    seen, out = set(), []
    for M, N, K, p in cases:           # every distinct plan, on the first shape that carries it
        if tuple(p) not in seen:
            seen.add(tuple(p))
            out.append((M, N, K, p))
    out += [(M, N, K, p) for N, K, M, p in PACKED_TUNED] + REFUSAL
    for M, p in BASE:
        out.append((M, BASE_N, BASE_K, p))
        for f, v in BOGUS.items():
            q = list(p)
            q[f] = v
            out.append((M, BASE_N, BASE_K, q))
    return out


def plan_check_rows(ops):
    rows = []
    for M, N, K, p in explicit_plans():
        sk = p[6]
        split4 = p[:6] + [4]
        # the plan on its shape; on a K of fewer K-tiles than its split; both again with split-K 4
        for q, k in ((p, K), (p, 64 * max(1, sk - 1)), (split4, K), (split4, 192)):
            res = [int(ops.gemm_plan_check(q, M, N, k, epi, packed)) for packed in (False, True) for epi in range(4)]
            rows.append(q + [M, N, k] + res)
    return rows


def emit():
    import torch

    from butterfly_amd import ops as bops

    if not bops.load_library():
        raise SystemExit(bops._load_error)
    ops = torch.ops.bfly
    out = []
    for N, K, epi in shapes():
        rows = []
        for M in MS:
            rows.append([M] + [int(v) for v in ops.gemm_plan(M, N, K)] + [int(ops.gemm_workspace_size(M, N, K))]
                        + [int(ops.gemm_check(M, N, K, e)) for e in range(3)]
                        + [int(ops.gemm_rowscale_check(M, N, K, e)) for e in range(3)]
                        + [int(ops.gemm_packed_check(M, N, K, e)) for e in (0, 2, 3)])
        out.append([N, K, epi, rows])
    doc = {"shapes": out}
    if not any(os.environ.get(k) for k in SWITCHES):
        doc["plan_checks"] = plan_check_rows(ops)   # explicit plans do not read the environment
    return doc


def collect(variant):
    """The dump of one variant, from a child process with that environment."""
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(VARIANTS[variant])
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--emit"], env=env, capture_output=True,
                         text=True, cwd=ROOT)
    if res.returncode != 0:
        raise RuntimeError(f"dump of {variant} failed:\n{res.stderr}")
    return json.loads(res.stdout.splitlines()[-1])


COLUMNS = {
    "default.shapes": "[N, K, epilogue of the model, rows in the order of MS of [M, gemm_plan x 7 (kind, mt, nt, bm, "
                      "bn, sk, wk), gemm_workspace_size, gemm_check epi 0-2, gemm_rowscale_check epi 0-2, "
                      "gemm_packed_check epi 0, 2, 3]]",
    "default.plan_checks": "[plan x 7 (kind, mt, nt, wk, bm, bn, sk), M, N, K, gemm_plan_check row-major epi 0-3, "
                           "packed epi 0-3]",
    "changes": "per variant, the rows that differ from the default: [index of the shape, [[index into MS, row]]]",
}


def load_fixture():
    """{variant: what emit() gives in that variant's environment}, from the fixture: the default in
    full, every other variant as the rows of the shapes table that differ from it."""
    with open(FIXTURE) as f:
        doc = json.load(f)
    out = {"default": doc["default"]}
    for name, changes in doc["changes"].items():
        shapes = [[N, K, epi, list(rows)] for N, K, epi, rows in doc["default"]["shapes"]]
        for si, rows in changes:
            for mi, row in rows:
                shapes[si][3][mi] = row
        out[name] = {"shapes": shapes}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--emit", action="store_true")
    a = ap.parse_args()
    if a.emit:
        print(json.dumps(emit(), separators=(",", ":")))
        return
    docs = {name: collect(name) for name in VARIANTS}
    base = docs["default"]["shapes"]
    changes = {}
    for name, doc in docs.items():
        if name == "default":
            continue
        assert [s[:3] for s in doc["shapes"]] == [s[:3] for s in base]
        changes[name] = [[si, [[mi, row] for mi, row in enumerate(s[3]) if row != base[si][3][mi]]]
                         for si, s in enumerate(doc["shapes"]) if s[3] != base[si][3]]

    def lines(rows, per_line=1):
        text = [json.dumps(r, separators=(",", ":")) for r in rows]
        return ",\n".join(",".join(text[i:i + per_line]) for i in range(0, len(text), per_line))

    os.makedirs(os.path.dirname(FIXTURE), exist_ok=True)
    with open(FIXTURE, "w") as f:
        f.write('{\n"columns": ' + json.dumps(COLUMNS) + ',\n"default": {\n"shapes": [\n' + lines(base))
        f.write('\n],\n"plan_checks": [\n' + lines(docs["default"]["plan_checks"], 4) +'\n]\n},\n"changes": {\n')
        f.write(",\n".join(f'"{name}": [\n{lines(ch)}\n]' for name, ch in changes.items()))
        f.write("\n}\n}\n")
    assert load_fixture() == docs
    print(f"wrote {FIXTURE} ({os.path.getsize(FIXTURE)} bytes)")


if __name__ == "__main__":
    main()
