#!/usr/bin/env python3
"""Compare the kernels of two device assembly listings of one source file, position by position.

    hipcc <flags> -S --cuda-device-only csrc/kernels/gemm.hip -o parent.s     (on each tree)
    python tools/asm_kernel_diff.py parent.s new.s [--stats NAME_REGEX]

A refactor of a kernel file should leave the code object's kernels in their order and, for the
kernels it did not mean to change, leave their instructions alone. For every kernel (in the order
of emission) this prints whether its instruction text is the same once the kernel's own symbol and
the function number in its local labels (.LBB<n>_, .LJTI<n>_) are taken out, with the register
lines of the metadata (.sgpr_count, .vgpr_count, .agpr_count, scratch, spills). --stats prints,
for the kernels whose demangled name matches the regex, instruction counts by mnemonic class and
the ordered s_waitcnt immediates, and writes <listing>.<n>.kloop.txt: the text of the innermost
loop with MFMAs (the K loop), register numbers taken out, for diffing.
"""
import argparse
import re
import subprocess
import sys


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return [re.sub(r"\(.*", "", o).replace("void bfly::", "") for o in out[: len(names)]]


def kernels(path):
    """[(symbol, [instruction lines])] in file order, and {symbol: {metadata key: value}}."""
    lines = open(path).read().split("\n")
    ks, meta, cur, sym = [], {}, None, None
    for i, ln in enumerate(lines):
        m = re.match(r"^(_Z\w+):\s*(;.*)?$", ln)
        if m and i >= 1 and cur is None and any(f".type\t{m.group(1)},@function" in p for p in lines[max(0, i - 6): i]):
            sym, cur = m.group(1), []
            continue
        if cur is not None:
            if re.match(r"^\.Lfunc_end\d+:", ln):
                ks.append((sym, cur))
                cur = None
                continue
            s = ln.split(";")[0].rstrip()
            if s.strip() and not s.strip().startswith((".p2align", ".loc", ".cfi", ".file")):
                cur.append(s)
    # amdhsa.kernels metadata: one "  - .key: value" list item per kernel
    keys = ("sgpr_count", "vgpr_count", "agpr_count", "private_segment_fixed_size", "sgpr_spill_count",
            "vgpr_spill_count", "group_segment_fixed_size")
    start = next((i for i, ln in enumerate(lines) if ln.startswith("amdhsa.kernels:")), len(lines))
    blk = {}
    for ln in lines[start + 1:]:
        if ln.startswith("  - ") or not ln.startswith("  "):
            if "symbol" in blk:
                meta[blk.pop("symbol")] = blk
            blk = {}
            if not ln.startswith("  "):
                break
        m = re.match(r"\s+(?:- )?\.(\w+):\s+(\S+)$", ln)
        if m and m.group(1) in keys:
            blk[m.group(1)] = int(m.group(2))
        elif m and m.group(1) == "symbol":
            blk["symbol"] = m.group(2)[:-3]
    return ks, meta


def norm(sym, body):
    out = []
    for s in body:
        s = s.replace(sym, "SYM")
        s = re.sub(r"\.L(BB|JTI)\d+_", r".L\1_", s)
        out.append(s)
    return out


def stats(body):
    c = {"total": 0, "v_mfma": 0, "ds_read_b128": 0, "buffer_load_lds": 0, "s_barrier": 0, "v_accvgpr": 0,
         "salu": 0, "valu": 0}
    waits = []
    for s in body:
        t = s.strip()
        if t.endswith(":") or t.startswith("."):
            continue
        op = t.split()[0]
        c["total"] += 1
        if op.startswith("v_mfma"):
            c["v_mfma"] += 1
        elif op == "ds_read_b128":
            c["ds_read_b128"] += 1
        elif op.startswith("buffer_load") and " lds" in t:
            c["buffer_load_lds"] += 1
        elif op == "s_barrier":
            c["s_barrier"] += 1
        elif op.startswith("v_accvgpr"):
            c["v_accvgpr"] += 1
        elif op == "s_waitcnt":
            waits.append(t.split(None, 1)[1])
        elif op.startswith("s_"):
            c["salu"] += 1
        elif op.startswith("v_"):
            c["valu"] += 1
    return c, waits


def k_loop(body):
    """Lines from a label to a backward branch to it: the shortest such span that holds MFMAs."""
    at = {s.strip()[:-1]: i for i, s in enumerate(body) if s.strip().endswith(":")}
    best = None
    for i, s in enumerate(body):
        m = re.match(r"\s+s_c?branch\w*\s+(\S+)", s)
        tgt = at.get(m.group(1)) if m else None
        if tgt is not None and tgt < i and any("v_mfma" in x for x in body[tgt:i]):
            if best is None or i - tgt < best[1] - best[0]:
                best = (tgt, i + 1)
    return body[best[0]: best[1]] if best else []


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--stats", default=None)
    a = ap.parse_args()
    (kp, mp), (kn, mn) = kernels(a.parent), kernels(a.new)
    dp, dn = demangle([k[0] for k in kp]), demangle([k[0] for k in kn])
    print(f"kernels: parent {len(kp)}, new {len(kn)}")
    same = differ = 0
    for i in range(max(len(kp), len(kn))):
        if i >= len(kp) or i >= len(kn):
            print(f"{i:3d} UNPAIRED {dp[i] if i < len(kp) else '-'} | {dn[i] if i < len(kn) else '-'}")
            differ += 1
            continue
        text = norm(*kp[i]) == norm(*kn[i])
        regs = mp.get(kp[i][0]) == mn.get(kn[i][0])
        same += text and regs
        differ += not (text and regs)
        tag = "same" if text and regs else "TEXT DIFFERS" if not text else "REGISTERS DIFFER"
        name = dp[i] if dp[i] == dn[i] else f"{dp[i]} -> {dn[i]}"
        print(f"{i:3d} {tag:16s} {name}")
        if not (text and regs):
            print(f"      parent {mp.get(kp[i][0])}\n      new    {mn.get(kn[i][0])}")
    print(f"same {same}, different {differ}")
    if a.stats:
        for side, ks, dm, meta, path in (("parent", kp, dp, mp, a.parent), ("new", kn, dn, mn, a.new)):
            for i, (sym, body) in enumerate(ks):
                if not re.search(a.stats, dm[i]):
                    continue
                c, waits = stats(body)
                loop = k_loop(norm(sym, body))
                lc, _ = stats(loop)
                loop_path = f"{path}.{i}.kloop.txt"
                with open(loop_path, "w") as f:
                    f.write("\n".join(re.sub(r"\b([vsa])\d+\b|\b([vsa])\[\d+:\d+\]", r"\1\2N", s) for s in loop) + "\n")
                print(f"{side} {i} {dm[i]}\n  {meta.get(sym)}\n  whole kernel {c}\n  K loop ({len(loop)} lines) {lc}\n"
                      f"  s_waitcnt: {' | '.join(waits)}\n  K loop written to {loop_path}")
    return 0 if differ == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
