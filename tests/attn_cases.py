"""Attention test inputs whose correct output names the keys that were read.

With random-normal Q/K/V and near-flat softmax rows the output is an average of n V rows: one
missing, extra or misplaced key moves it by ~1/n, far below a 2e-2 tolerance at the context
lengths where the kernels have their structure (splits, page streams, KV tiles, query blocks).
The families here make one key matter:

  needle   query head g is H[g] + 0.05 noise, the key at the chosen position is 2 H[g] (H the
           128 x 128 Sylvester Hadamard matrix, rows exactly orthogonal). scale * 2 * 128 = 22.6
           against random scores ~N(0, 1): the output is V[needle] to one bf16 rounding.
  poison   every cache slot a kernel must not read (stale slots of the last page, pages behind
           table entries past the needed ones, pool pages in no table) holds K = 48 at columns
           c % 16 == 0 (= 3 sum H[0..15]: scores 34 with every needle query, above the needle)
           and V = 256. Finite values, valid page indices: nothing here reads out of bounds.
  uniform  Q = 0, so p = 1/n exactly; V[j] = 64 e_(j mod 128): out[d] n / 64 counts the visible
           keys j = d (mod 128), and LSE = ln(#visible keys).
  causal needle  K[j] = 2 (1 + j // 128) H[j % 128], query head h of row j is
           H[(j + delta_h) % 128] + 0.05 noise: the latest visible member of the wanted class
           wins by 22.6 nats, so delta = 0 returns the diagonal, +1 / +2 want keys that the
           causal mask or the sequence end must hide, the negative ones reach 1, 63..65 and 128
           rows back. V is random in [-1/4, 1/4] (see _bounded_v).

Every constant is exact in bf16 and in e4m3: the FP8 variants are the same inputs cast with
.to(torch.float8_e4m3fn), and the reference runs over the cast values.

Pure torch, device-agnostic: the builders make CPU tensors, `reference_*` compute in fp64 on the
CPU (optionally emulating the kernels' roundings: P to bf16 before PV, output to bf16), and
`mutants_*` yield references with one key dropped, added or misplaced, which the criteria must
reject (tests/test_attn_cases_cpu.py).
"""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace

import torch

D, BS = 128, 32
SCALE = 1.0 / math.sqrt(D)
F8 = torch.float8_e4m3fn
DELTAS = (0, 1, 2, -1, -63, -64, -65, -128)
NOISE = 0.05
POISON_K, POISON_V = 48.0, 256.0


@functools.lru_cache(maxsize=None)
def hadamard() -> torch.Tensor:
    h = torch.ones(1, 1)
    while h.shape[0] < D:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return h


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g).to(torch.bfloat16).float()


def _bounded_v(g, *shape):
    """Causal-needle V: uniform in [-1/4, 1/4]. A row that sees no member of its wanted class is
    a soft mean over noise-only scores, and there the kernels' bf16 P (relative 2^-9 per term,
    2^-8 once normalised by the sum of the rounded terms) moves the output by up to
    2^-8 max|V|: 2^-10 with this V, inside the criterion's 1e-3 on every row. (With N(0, 1) V
    an exact kernel with bf16 P misses the criterion on rows that see 2..16 keys.)"""
    return ((torch.rand(*shape, generator=g) - 0.5) * 0.5).to(torch.bfloat16).float()


def _poison_k_row():
    r = torch.zeros(D)
    r[::16] = POISON_K
    return r


# ---------------------------------------------------------------------------------------
# Pass criteria: zero mismatching elements. Each returns (bad elements, worst err / tol).
# ---------------------------------------------------------------------------------------
def _mis(got, ref, atol, rtol):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = (got - ref).abs()
    tol = atol + rtol * ref.abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    if err.numel() == 0:
        return 0, 0.0
    return int((err > tol).sum()), float((err / tol).max())


def needle_mismatches(got, ref):
    """|got - ref| <= 1e-3 + 2^-7 |ref|: the mass off the needle is at most n e^-19, so the
    result is a V row to within one bf16 rounding (relative 2^-8; 2^-7 with the tie cases)."""
    return _mis(got, ref, 1e-3, 2.0 ** -7)


def uniform_mismatches(got, ref):
    """|got - ref| <= 1e-3 + 1.5e-2 |ref|: P rounded to bf16 and the output rounded to bf16
    bound the systematic error at 2 * 2^-9 = 0.4 %; one key more or less moves an entry by
    1 / ceil(n / 128) >= 3e-2 of its value for n <= 4096."""
    return _mis(got, ref, 1e-3, 1.5e-2)


def ones_mismatches(got, ref):
    """Uniform with V = 1: every p is exactly 1, so O / L is exactly 1 and the output is 1 to one
    bf16 step: |got - 1| <= 2^-7."""
    return _mis(got, ref, 2.0 ** -7, 0.0)


def lse_mismatches(lse, want, n_max):
    """|lse - ln(count)| <= 0.25 / (n_max + 1), a quarter of the gap between ln(n_max) and
    ln(n_max + 1); -inf (no visible key) must be -inf."""
    lse, want = lse.detach().cpu().double(), want.detach().cpu().double()
    assert lse.shape == want.shape, (lse.shape, want.shape)
    tol = 0.25 / (n_max + 1)
    fin = torch.isfinite(want)
    bad = int((torch.isfinite(lse) != fin).sum()) + int((lse[~fin] != want[~fin]).sum())
    err = (lse[fin] - want[fin]).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    worst = float(err.max() / tol) if err.numel() else 0.0
    return bad + int((err > tol).sum()), worst


def old_mismatches(got, ref):
    """The suite's former criterion for every attention test (documented as too weak)."""
    return _mis(got, ref, 2e-2, 2e-2)


# ---------------------------------------------------------------------------------------
# fp64 reference core
# ---------------------------------------------------------------------------------------
def raw_scores(q, k, scale=SCALE):
    """Unmasked scaled scores [Hq, R, n] in fp64 of q [R, Hq, D] against k [n, Hkv, D]."""
    q, k = q.double(), k.double()
    R, Hq, Hkv, n = q.shape[0], q.shape[1], k.shape[1], k.shape[0]
    return torch.einsum("rkgd,nkd->kgrn", q.view(R, Hkv, Hq // Hkv, D), k).reshape(Hq, R, n) * scale


def attend(q, k, v, vis, scale=SCALE, emulate=False, raw=None):
    """q [R, Hq, D], k / v [n, Hkv, D], vis [R, n] bool (row sees key). fp64 softmax attention
    -> (out [R, Hq, D], lse [R, Hq], scores [Hq, R, n] with -inf where hidden). A row that sees
    nothing gives a zero output and lse = -inf. `emulate`: round the unnormalised P (relative to
    the row max) to bf16 before PV, normalise by the unrounded sum, round the output to bf16 —
    the roundings the kernels make. `raw`: raw_scores(q, k, scale), when the caller kept them."""
    v = v.double()
    R, Hq, Hkv, n = q.shape[0], q.shape[1], k.shape[1], k.shape[0]
    G = Hq // Hkv
    s = raw_scores(q, k, scale) if raw is None else raw
    s = s.masked_fill(~vis[None], float("-inf"))
    m = s.amax(-1, keepdim=True) if n else torch.full((Hq, R, 1), float("-inf"), dtype=s.dtype)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    p = torch.exp(s - m)
    l = p.sum(-1)
    if emulate:
        p = p.to(torch.bfloat16).double()
    o = torch.einsum("kgrn,nkd->rkgd", p.view(Hkv, G, R, n), v).reshape(R, Hq, D)
    lt = l.transpose(0, 1)
    o = torch.where(lt.unsqueeze(-1) > 0, o / lt.clamp(min=1e-300).unsqueeze(-1), torch.zeros_like(o))
    if emulate:
        o = o.to(torch.bfloat16).double()
    lse = torch.where(l > 0, m.squeeze(-1) + torch.log(l.clamp(min=1e-300)), torch.full_like(l, float("-inf")))
    return o, lse.transpose(0, 1), s


def lead_nats(scores):
    """Per (head, row): top score minus runner-up among the visible keys, for the rows whose top
    score is a needle's (>= 16; random keys score ~N(0, 1)). -> (leads 1-D, number of rows)."""
    if scores.shape[-1] < 2:
        return scores.new_zeros(0), 0
    top = scores.topk(2, -1).values
    sel = top[..., 0] >= 16.0
    return (top[..., 0] - top[..., 1])[sel], int(sel.sum())


# ---------------------------------------------------------------------------------------
# Paged pool with holes and poison
# ---------------------------------------------------------------------------------------
def _build_pool(seq_k, seq_v, Hkv, seed, fp8, spare_entries=2, holes=6):
    """seq_k / seq_v: per sequence [n, Hkv, D] f32. Pages scattered by a random permutation over a
    pool with `holes` pages in no sequence; table rows are `spare_entries` wider than the longest
    sequence needs, the entries past a sequence's pages pointing at hole pages. Everything not
    written by a sequence's tokens is poison."""
    g = _gen(seed)
    nblk = [(k.shape[0] + BS - 1) // BS for k in seq_k]
    n_real = sum(nblk)
    pool = n_real + holes
    W = max(nblk) + spare_entries
    perm = torch.randperm(pool, generator=g)
    hole = perm[n_real:]
    kc = _poison_k_row().expand(pool, Hkv, BS, D).clone()
    vc = torch.full((pool, Hkv, D, BS), POISON_V)
    tables = torch.empty(len(seq_k), W, dtype=torch.int64)
    at = 0
    for b, (k, v) in enumerate(zip(seq_k, seq_v)):
        tables[b, :nblk[b]] = perm[at:at + nblk[b]]
        at += nblk[b]
        tables[b, nblk[b]:] = hole[(torch.arange(W - nblk[b]) + b) % holes]
        t = torch.arange(k.shape[0])
        pg, sl = tables[b, t // BS], t % BS
        kc[pg, :, sl, :] = k
        vc[pg, :, :, sl] = v
    dt = F8 if fp8 else torch.bfloat16
    return kc.to(torch.bfloat16).to(dt), vc.to(torch.bfloat16).to(dt), tables.to(torch.int32)


def _gather(kc, vc, table_row, nslots):
    """The first `nslots` cache slots behind a table row -> k, v [nslots, Hkv, D] fp64."""
    pages = table_row[: (nslots + BS - 1) // BS].long()
    Hkv = kc.shape[1]
    k = kc[pages].float().permute(1, 0, 2, 3).reshape(Hkv, -1, D)[:, :nslots]
    v = vc[pages].float().permute(1, 0, 3, 2).reshape(Hkv, -1, D)[:, :nslots]
    return k.transpose(0, 1).double(), v.transpose(0, 1).double()


def _gathered(c, seq, q, table_row, nslots):
    """_gather through a case's cache, with the raw scores of `q` against the gathered keys: the
    reference, its emulation and most mutants of a sequence read the same slots. The pool is
    widened to f32 once per case (FP8 -> f32 is slow on a CPU)."""
    if "pool" not in c.cache:
        c.cache["pool"] = (c.kc.float(), c.vc.float())
    key = ("kv", seq, tuple(table_row[: (nslots + BS - 1) // BS].tolist()), nslots)
    if key not in c.cache:
        k, v = _gather(*c.cache["pool"], table_row, nslots)
        c.cache[key] = (k, v, raw_scores(q, k))
    return c.cache[key]


# ---------------------------------------------------------------------------------------
# Decode
# ---------------------------------------------------------------------------------------
DECODE_LENS = (1, 31, 32, 33, 100, 416, 700)
DECODE_HEADS = ((16, 1), (12, 4), (8, 8), (64, 8))
DECODE_PARTS = (0, 128, 256, 4096)


def part_edges(n, part_tokens):
    """Split boundaries k * part_tokens inside a context of n keys. part_tokens = 0 is the
    launcher's own choice, which is 256 for every batch of the sweep (attn_decode_part_tokens:
    never below 256 while there is more than one split): both 128 and 256 are probed there."""
    parts = (128, 256) if part_tokens <= 0 else (part_tokens,)
    return sorted({e for p in parts for e in range(p, n, p)})


def needle_positions(n, part_tokens, count):
    """`count` key positions in [0, n), most telling first: the ends and the first key of the
    last (ragged) page, both sides of every split edge, one key in each of the 4 waves' page
    streams (pages 0..3), one in pages 1, 5, 9 (the three FP8 register sets of wave 1), then
    both sides of every page edge. A context shorter than `count` repeats its positions."""
    cand = [n - 1, (n - 1) // BS * BS, 0]
    edges = part_edges(n, part_tokens)
    cand += [e - 1 for e in edges]      # the 8-head layout holds the last key of EVERY split
    cand += edges
    cand += [p * BS + 13 for p in (0, 1, 2, 3, 5, 9)]
    for e in range(BS, n, BS):
        cand += [e - 1, e]
    cand += range(n)           # then any key: the heads of one kv head never share a position
    seen, out = set(), []
    for c in cand:
        if 0 <= c < n and c not in seen:
            seen.add(c)
            out.append(c)
    return [out[i % len(out)] for i in range(count)]


def decode_case(kind, Hq, Hkv, part_tokens, fp8, lens=DECODE_LENS, positions=None, v_ones=False,
                seed=100):
    """Cached; the uniform inputs do not depend on part_tokens, so those cases share their
    tensors and their reference."""
    if kind == "uniform":
        c = _decode_case(kind, Hq, Hkv, 0, fp8, lens, positions, v_ones, seed)
        return SimpleNamespace(**{**vars(c), "part_tokens": part_tokens})
    return _decode_case(kind, Hq, Hkv, part_tokens, fp8, lens, positions, v_ones, seed)


@functools.lru_cache(maxsize=None)
def _decode_case(kind, Hq, Hkv, part_tokens, fp8, lens, positions, v_ones, seed):
    """kind 'needle' | 'uniform'. `positions`: needle positions used for every sequence (default
    needle_positions per sequence). `v_ones`: uniform V = 1 instead of one-hot (contexts past
    4096, where a one-hot count is below the tolerance: the output must be 1, poison catches
    extra keys)."""
    g = _gen(seed + 7 * Hq + Hkv)
    G, B = Hq // Hkv, len(lens)
    H = hadamard()
    q = torch.zeros(B, Hq, D)
    pos = torch.full((B, Hq), -1, dtype=torch.int64)
    seq_k, seq_v = [], []
    for b, n in enumerate(lens):
        if kind == "needle":
            k, v = _randn(g, n, Hkv, D), _randn(g, n, Hkv, D)
            pl = list(positions) if positions is not None else needle_positions(n, part_tokens, Hq)
            for i in range(Hq):
                kv, gi = divmod(i, G)
                p = pl[i % len(pl)]
                assert 0 <= p < n
                pos[b, i] = p
                k[p, kv] = 2 * H[gi]
                q[b, i] = H[gi] + NOISE * torch.randn(D, generator=g)
        else:
            k = _randn(g, n, Hkv, D)
            v = torch.zeros(n, Hkv, D)
            if v_ones:
                v[:] = 1.0
            else:
                v[torch.arange(n), :, torch.arange(n) % D] = 64.0
        seq_k.append(k)
        seq_v.append(v)
    kc, vc, tables = _build_pool(seq_k, seq_v, Hkv, seed + 1, fp8)
    return SimpleNamespace(op="decode", kind=kind, q=q.to(torch.bfloat16), kc=kc, vc=vc, tables=tables,
                           ctx=list(lens), max_ctx=max(lens), part_tokens=part_tokens, pos=pos,
                           Hq=Hq, Hkv=Hkv, v_ones=v_ones, cache={})


def _decode_one(c, b, vis_fn=None, table_row=None, emulate=False):
    n = c.ctx[b]
    row = c.tables[b] if table_row is None else table_row
    q = c.q[b:b + 1].float()
    k, v, raw = _gathered(c, b, q, row, n + 1)      # one slot past ctx, for the mutants
    vis = torch.arange(n + 1) < n
    if vis_fn is not None:
        vis = vis_fn(vis.clone(), n)
    return attend(q, k, v, vis[None], emulate=emulate, raw=raw)


def reference_decode(c, emulate=False):
    """-> (out [B, Hq, D] fp64, [per-sequence scores])."""
    key = ("ref", emulate)
    if key not in c.cache:
        outs, scores = [], []
        for b in range(len(c.ctx)):
            o, _, s = _decode_one(c, b, emulate=emulate)
            outs.append(o[0])
            scores.append(s[:, 0, :c.ctx[b]])
        c.cache[key] = (torch.stack(outs), scores)
    return c.cache[key]


def mutants_decode(c):
    """(name, out) with ONE sequence computed wrongly, the longest (where one key weighs least)."""
    base = reference_decode(c)[0]
    b = max(range(len(c.ctx)), key=lambda i: c.ctx[i])
    n = c.ctx[b]
    nblk = (n + BS - 1) // BS

    def put(o):
        out = base.clone()
        out[b] = o[0][0]
        return out

    def hide(j):
        def f(vis, n):
            vis[j] = False
            return vis
        return f

    def extra(vis, n):
        vis[n] = True
        return vis

    # A dropped key shows in the uniform case wherever it is, in the needle case where a needle
    # sits: on the last key and on the key before every split edge in every layout of the sweep;
    # the 199 edges of the many-split case hold needles before 2 of them. With V = 1 every count
    # gives the same output: only extras show.
    probed = set(c.pos[b].tolist())
    if not c.v_ones:
        yield "drop_last", put(_decode_one(c, b, hide(n - 1)))
        for e in part_edges(n, c.part_tokens):
            if c.kind == "uniform" or e - 1 in probed:
                yield f"drop_split_edge_{e - 1}", put(_decode_one(c, b, hide(e - 1)))
    yield "one_past_ctx", put(_decode_one(c, b, extra))
    row = c.tables[b].clone()
    row[nblk - 1] = c.tables[b, nblk]
    yield "last_page_from_next_entry", put(_decode_one(c, b, table_row=row))
    if nblk >= 2 and not c.v_ones:
        row = c.tables[b].clone()
        row[nblk - 1] = c.tables[b, nblk - 2]
        yield "last_page_from_previous_entry", put(_decode_one(c, b, table_row=row))


# ---------------------------------------------------------------------------------------
# Varlen prefill
# ---------------------------------------------------------------------------------------
PREFILL_LENS = (1, 37, 300, 640, 2)
PREFILL_LK = (5, 0, 129, 64, 65)
PREFILL_LQ = (3, 2, 70, 257, 33)


def _causal_needle_qk(g, rows, Hq, Hkv):
    """rows: the index j of each row (global row, or position in its sequence). K[j] of kv head
    kv is 2 (1 + j // 128) H[(j + 5 kv) % 128], query head h of group member h % G wants the
    class delta[(h % G) % 8] rows away."""
    H = hadamard()
    G = Hq // Hkv
    T = rows.shape[0]
    k = torch.empty(T, Hkv, D)
    q = torch.empty(T, Hq, D)
    for kv in range(Hkv):
        k[:, kv] = (2 * (1 + rows // D)).float()[:, None] * H[(rows + 5 * kv) % D]
        for gi in range(G):
            d = DELTAS[gi % len(DELTAS)]
            q[:, kv * G + gi] = H[(rows + d + 5 * kv) % D] + NOISE * torch.randn(T, D, generator=g)
    return q, k


@functools.lru_cache(maxsize=None)
def prefill_case(kind, Hq, Hkv, causal=True, lens=PREFILL_LENS, lk=None, seed=200):
    """kind 'needle' (causal only) | 'uniform'. Non-causal: `lens` query rows per sequence, `lk`
    keys per sequence taken from other rows (cu_seqlens_k)."""
    g = _gen(seed + 7 * Hq + Hkv)
    lk = tuple(lens) if lk is None else tuple(lk)
    T, Tk = sum(lens), sum(lk)
    cu = [0]
    cuk = [0]
    for a, b in zip(lens, lk):
        cu.append(cu[-1] + a)
        cuk.append(cuk[-1] + b)
    if kind == "needle":
        assert causal
        q, k = _causal_needle_qk(g, torch.arange(T), Hq, Hkv)
        v = _bounded_v(g, Tk, Hkv, D)
    else:
        q = torch.zeros(T, Hq, D)
        k = _randn(g, Tk, Hkv, D)
        v = torch.zeros(Tk, Hkv, D)
        v[torch.arange(Tk), :, torch.arange(Tk) % D] = 64.0
    i32 = lambda a: torch.tensor(a, dtype=torch.int32)  # noqa: E731
    return SimpleNamespace(op="prefill", kind=kind, q=q.to(torch.bfloat16), k=k.to(torch.bfloat16),
                           v=v.to(torch.bfloat16), cu=i32(cu), cuk=i32(cuk), lens=tuple(lens), lk=lk,
                           causal=causal, max_seqlen=max(lens), Hq=Hq, Hkv=Hkv, cache={})


def _prefill_ref(c, mutant=None, emulate=False):
    """A mutant is wrong in the query heads of kv head 0 only (the other heads are the
    reference's): enough to be noticed, at 1 / Hkv of the work."""
    T = c.q.shape[0]
    if mutant is None:
        out = torch.zeros(T, c.Hq, D, dtype=torch.float64)
        lse = torch.full((T, c.Hq), float("-inf"), dtype=torch.float64)
        nh, nkv = c.Hq, c.Hkv
    else:
        base = reference_prefill(c)
        out, lse = base[0].clone(), base[1].clone()
        nh, nkv = c.Hq // c.Hkv, 1
    scores = []
    cu, cuk = c.cu.tolist(), c.cuk.tolist()
    Tk = c.k.shape[0]
    for i in range(len(c.lens)):
        a, b, ka, kb = cu[i], cu[i + 1], cuk[i], cuk[i + 1]
        L, n = b - a, kb - ka
        ext = min(n + 1, Tk - ka)                  # the next sequence's first key, for 'leak'
        if L == 0:
            continue
        row, col = torch.arange(L)[:, None], torch.arange(ext)[None, :]
        vis = (col < n).expand(L, ext)
        shift = {"shift_plus_1": 1, "shift_minus_1": -1}.get(mutant, 0)
        if c.causal:
            vis = vis & (col <= row + shift)
        if mutant == "leak_next_sequence":
            vis = vis | (col == n)
        if mutant == "drop_last":
            vis = vis & (col != n - 1)
        q, k = c.q[a:b].float(), c.k[ka:ka + ext].float()
        if ("raw", i) not in c.cache:
            c.cache["raw", i] = raw_scores(q, k)
        o, ls, s = attend(q[:, :nh], k[:, :nkv], c.v[ka:ka + ext, :nkv].float(), vis, emulate=emulate,
                          raw=c.cache["raw", i][:nh])
        out[a:b, :nh], lse[a:b, :nh] = o, ls
        scores.append(s)
    return out, lse, scores


def reference_prefill(c, emulate=False):
    """-> (out [T, Hq, D] fp64, lse [T, Hq] fp64, [per-sequence scores])."""
    key = ("ref", emulate)
    if key not in c.cache:
        c.cache[key] = _prefill_ref(c, emulate=emulate)
    return c.cache[key]


def visible_counts(c):
    """Uniform case: the number of keys each row sees -> [T] (LSE must be its log)."""
    cnt = torch.zeros(c.q.shape[0], dtype=torch.float64)
    cu = c.cu.tolist()
    for i, (L, n) in enumerate(zip(c.lens, c.lk)):
        r = torch.arange(L, dtype=torch.float64)
        cnt[cu[i]:cu[i + 1]] = torch.minimum(r + 1, torch.tensor(float(n))) if c.causal else float(n)
    return cnt


def split_keys(c):
    """The keys of every sequence of a non-causal case cut in two chunks (first half, rest):
    [(k, v, cu_seqlens_k)] x 2."""
    cuk = c.cuk.tolist()
    parts = []
    for half in (0, 1):
        idx, cu2 = [], [0]
        for i, n in enumerate(c.lk):
            a = cuk[i] + (0 if half == 0 else n // 2)
            b = cuk[i] + (n // 2 if half == 0 else n)
            idx.extend(range(a, b))
            cu2.append(cu2[-1] + b - a)
        ix = torch.tensor(idx, dtype=torch.long)
        parts.append((c.k[ix].contiguous(), c.v[ix].contiguous(), torch.tensor(cu2, dtype=torch.int32)))
    return parts


def mutants_prefill(c):
    names = ["leak_next_sequence"]
    names += ["shift_plus_1", "shift_minus_1"] if c.causal else ["drop_last"]
    for m in names:
        o, lse, _ = _prefill_ref(c, mutant=m)
        yield m, o, lse


# ---------------------------------------------------------------------------------------
# Paged chunked prefill
# ---------------------------------------------------------------------------------------
PAGED_CHUNKS = ((0, 37), (31, 1), (95, 50), (700, 16), (250, 129))
PAGED_SINGLE = ((700, 129),)


@functools.lru_cache(maxsize=None)
def paged_case(kind, Hq, Hkv, fp8, chunks=PAGED_CHUNKS, seed=300):
    """(prefix, chunk) per sequence: the chunk's rows at positions prefix .. prefix + chunk - 1
    attend causally to the sequence's cached keys [0, position]."""
    g = _gen(seed + 7 * Hq + Hkv)
    seq_k, seq_v, qs, cu, pos = [], [], [], [0], []
    for pre, ch in chunks:
        n = pre + ch
        j = torch.arange(n)
        if kind == "needle":
            qa, k = _causal_needle_qk(g, j, Hq, Hkv)
            v = _bounded_v(g, n, Hkv, D)
            qs.append(qa[pre:])
        else:
            k = _randn(g, n, Hkv, D)
            v = torch.zeros(n, Hkv, D)
            v[j, :, j % D] = 64.0
            qs.append(torch.zeros(ch, Hq, D))
        seq_k.append(k)
        seq_v.append(v)
        cu.append(cu[-1] + ch)
        pos.extend(range(pre, n))
    kc, vc, tables = _build_pool(seq_k, seq_v, Hkv, seed + 1, fp8, holes=7)
    i32 = lambda a: torch.tensor(a, dtype=torch.int32)  # noqa: E731
    return SimpleNamespace(op="paged", kind=kind, q=torch.cat(qs).to(torch.bfloat16), kc=kc, vc=vc,
                           tables=tables, cu=i32(cu), pos=i32(pos), chunks=tuple(chunks),
                           max_q=max(ch for _, ch in chunks), Hq=Hq, Hkv=Hkv, cache={})


def _paged_ref(c, mutant=None, emulate=False):
    """A mutant is wrong in the query heads of kv head 0 only, as in _prefill_ref."""
    T = c.q.shape[0]
    if mutant is None:
        out = torch.zeros(T, c.Hq, D, dtype=torch.float64)
        nh, nkv = c.Hq, c.Hkv
    else:
        out = reference_paged(c)[0].clone()
        nh, nkv = c.Hq // c.Hkv, 1
    scores = []
    cu = c.cu.tolist()
    for s, (pre, ch) in enumerate(c.chunks):
        a, b = cu[s], cu[s + 1]
        n = pre + ch
        nblk = (n + BS - 1) // BS
        row = c.tables[s].clone()
        if mutant == "last_page_from_next_entry":
            row[nblk - 1] = c.tables[s, nblk]
        if mutant == "last_page_from_previous_entry" and nblk >= 2:
            row[nblk - 1] = c.tables[s, nblk - 2]
        q = c.q[a:b].float()
        k, v, raw = _gathered(c, s, q, row, n + 1)  # one stale slot past the last key
        shift = {"shift_plus_1": 1, "shift_minus_1": -1}.get(mutant, 0)
        vis = torch.arange(n + 1)[None, :] <= (c.pos[a:b].long()[:, None] + shift)
        o, _, sc = attend(q[:, :nh], k[:, :nkv], v[:, :nkv], vis, emulate=emulate, raw=raw[:nh])
        out[a:b, :nh] = o
        scores.append(sc)
    return out, scores


def reference_paged(c, emulate=False):
    key = ("ref", emulate)
    if key not in c.cache:
        c.cache[key] = _paged_ref(c, emulate=emulate)
    return c.cache[key]


def mutants_paged(c):
    for m in ("shift_plus_1", "shift_minus_1", "last_page_from_next_entry", "last_page_from_previous_entry"):
        yield m, _paged_ref(c, mutant=m)[0]


# ---------------------------------------------------------------------------------------
# The cases the GPU file runs (tests/test_attention_gpu.py) and the CPU file proves sharp
# ---------------------------------------------------------------------------------------
MANY_SPLIT_PART = 32
MANY_SPLIT_CTX = (6400, 6368)      # 200 splits (200 % 4 == 0) and 199 (the combine's tail)


def many_split_positions(n):
    """Needles in splits 0, 63, 64, 127, 128 and the last one (first / last key of each: the
    combine kernel's 64- and 128-split strides), 8 positions for the 8 query heads."""
    p, last = MANY_SPLIT_PART, (n - 1) // MANY_SPLIT_PART
    return (0, 63 * p + p - 1, 64 * p, 127 * p + p - 1, 128 * p, n - 1, last * p, 128 * p - p // 2)


def many_split_case(kind, ctx, fp8):
    if kind == "needle":
        return decode_case("needle", 8, 1, MANY_SPLIT_PART, fp8, lens=(ctx,),
                           positions=many_split_positions(ctx), seed=400)
    return decode_case("uniform", 8, 1, MANY_SPLIT_PART, fp8, lens=(ctx,), v_ones=True, seed=400)


def strided_case():
    """Decode with q as a view into a fused QKV row; every context holds a needle per head."""
    return decode_case("needle", 8, 1, 0, False, lens=(9, 64, 250), seed=500)


PREFILL_CAUSAL_CASES = (("needle", 8, 1), ("needle", 16, 2), ("uniform", 8, 1), ("uniform", 16, 2))


def key_offsets_case():
    """Non-causal prefill, keys from other rows than the queries; one sequence has no keys."""
    return prefill_case("uniform", 8, 2, causal=False, lens=PREFILL_LQ, lk=PREFILL_LK)


PAGED_CASES = (
    # Hq, Hkv, chunks: the kernel launch_attn_prefill_paged picks
    (8, 1, PAGED_CHUNKS),      # LDS ring kernel, 9 x 1 x 5 = 45 workgroups <= 256: 8-page ring
    (64, 8, PAGED_CHUNKS),     # LDS ring kernel, 9 x 8 x 5 = 360 workgroups > 256: 4-page ring
    (8, 2, PAGED_SINGLE),      # one sequence: register kernel, G = 4 (1 head per wave)
    (8, 1, PAGED_SINGLE),      # one sequence: register kernel, G = 8 (2 heads per wave)
)


def decode_sweep():
    for kind in ("needle", "uniform"):
        for fp8 in (False, True):
            for Hq, Hkv in DECODE_HEADS:
                for pt in DECODE_PARTS:
                    yield kind, Hq, Hkv, pt, fp8


def mismatches_for(kind, v_ones=False):
    if v_ones:
        return ones_mismatches
    return needle_mismatches if kind == "needle" else uniform_mismatches
