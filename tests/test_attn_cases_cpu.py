"""The attention cases of tests/attn_cases.py are sharp: on the CPU, for every case the GPU file
runs, the criterion accepts the reference (also with the kernels' bf16 roundings emulated) and
rejects every reference with one key dropped, added or misplaced."""
import math

import pytest
import torch

from . import attn_cases as ac
from butterfly_amd.ops import reference as ref

MIN_LEAD = 16.0


def _accepts(mis, got, want, what):
    bad, worst = mis(got, want)
    assert bad == 0, f"{what}: {bad} mismatches, worst err/tol {worst:.3g}"


def _rejects(mis, got, want, what):
    bad, _ = mis(got, want)
    assert bad > 0, f"{what}: the criterion does not notice this mutant"
    return bad


def _check_leads(scores, min_rows, what):
    leads = [ac.lead_nats(s) for s in scores]
    rows = sum(n for _, n in leads)
    assert rows >= min_rows, f"{what}: {rows} needle rows, expected >= {min_rows}"
    lo = min(float(l.min()) for l, n in leads if n)
    assert lo >= MIN_LEAD, f"{what}: smallest lead {lo:.2f} nats"


def _ops_ref_decode(c):
    return ref.attn_decode(c.q, c.kc, c.vc, c.tables, torch.tensor(c.ctx), ac.SCALE)


def _check_decode_case(c, what):
    mis = ac.mismatches_for(c.kind, c.v_ones)
    want, scores = ac.reference_decode(c)
    _accepts(mis, _ops_ref_decode(c), want, what + " ops.reference")
    _accepts(mis, ac.reference_decode(c, emulate=True)[0], want, what + " bf16-P emulation")
    if c.kind == "needle":
        multi = sum(1 for n in c.ctx if n >= 2)
        _check_leads(scores, multi * c.Hq, what)
    names = []
    for name, out in ac.mutants_decode(c):
        _rejects(mis, out, want, f"{what} {name}")
        names.append(name)
    return names


@pytest.mark.parametrize("kind,Hq,Hkv,part_tokens,fp8", list(ac.decode_sweep()))
def test_decode_sweep_cases_are_sharp(kind, Hq, Hkv, part_tokens, fp8):
    c = ac.decode_case(kind, Hq, Hkv, part_tokens, fp8)
    names = _check_decode_case(c, f"decode {kind} Hq={Hq} Hkv={Hkv} pt={part_tokens} fp8={fp8}")
    edges = ac.part_edges(700, part_tokens)
    assert {"drop_last", "one_past_ctx", "last_page_from_next_entry",
            "last_page_from_previous_entry"} <= set(names)
    # every case, needle layouts included, rejects the drop of the key before EVERY split edge
    assert [n for n in names if n.startswith("drop_split_edge_")] == [f"drop_split_edge_{e - 1}" for e in edges]


def test_decode_needle_positions_cover_the_structure():
    """Over the parametrisation the needles of the 700-key sequence sit on the ends, both sides of
    every page and split edge, the first and last key of the ragged last page, one key in each
    wave's page stream and in each FP8 register set."""
    n = 700
    seen = set()
    for _, Hq, Hkv, pt, _ in ac.decode_sweep():
        pos = ac.needle_positions(n, pt, Hq)
        assert len(set(pos)) == Hq
        assert {n - 1, 672, 0} <= set(pos[:3])          # every head layout probes the last page
        seen |= set(pos)
    want = {0, n - 1, 672}
    for e in range(32, n, 32):
        want |= {e - 1, e}
    want |= {p * 32 + 13 for p in (0, 1, 2, 3, 5, 9)}
    assert want <= seen, sorted(want - seen)
    # a short sequence repeats its few positions instead of leaving heads without a needle
    assert ac.needle_positions(1, 128, 16) == [0] * 16


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("ctx", ac.MANY_SPLIT_CTX)
@pytest.mark.parametrize("kind", ["needle", "uniform"])
def test_decode_many_split_cases_are_sharp(kind, ctx, fp8):
    c = ac.many_split_case(kind, ctx, fp8)
    if kind == "needle":
        splits = sorted({p // ac.MANY_SPLIT_PART for p in c.pos[0].tolist()})
        last = (ctx - 1) // ac.MANY_SPLIT_PART
        assert splits == [0, 63, 64, 127, 128, last] and last + 1 > 128
    names = _check_decode_case(c, f"decode many splits {kind} ctx={ctx} fp8={fp8}")
    assert "one_past_ctx" in names and "last_page_from_next_entry" in names
    if kind == "uniform":      # a combine that loses the 3-split tail of 199 splits gives 196 / 199
        want = ac.reference_decode(c)[0]
        lost = (want * (196.0 / 199.0)).to(torch.bfloat16)
        assert ac.mismatches_for(kind, c.v_ones)(lost, want)[0] == want.numel()
    if kind == "needle":       # the needles on the last key of splits 63 and 127
        assert {"drop_last", "drop_split_edge_2047", "drop_split_edge_4095"} <= set(names)


def test_decode_strided_case_is_sharp():
    _check_decode_case(ac.strided_case(), "decode strided q")


PREFILL_CASES = [c + (True,) for c in ac.PREFILL_CAUSAL_CASES] + [("uniform", 8, 2, False)]


def _prefill(kind, Hq, Hkv, causal):
    return ac.prefill_case(kind, Hq, Hkv) if causal else ac.key_offsets_case()


@pytest.mark.parametrize("kind,Hq,Hkv,causal", PREFILL_CASES)
def test_prefill_cases_are_sharp(kind, Hq, Hkv, causal):
    c = _prefill(kind, Hq, Hkv, causal)
    what = f"prefill {kind} Hq={Hq} Hkv={Hkv} causal={causal}"
    mis = ac.mismatches_for(kind)
    want, want_lse, scores = ac.reference_prefill(c)
    kw = {} if causal else {"cu_seqlens_k": c.cuk}
    o, lse = ref.attn_prefill(c.q, c.k, c.v, c.cu, c.max_seqlen, ac.SCALE, causal, return_lse=True, **kw)
    _accepts(mis, o, want, what + " ops.reference")
    _accepts(mis, ac.reference_prefill(c, emulate=True)[0], want, what + " bf16-P emulation")
    n_max = max(c.lk)
    if kind == "uniform":
        cnt = ac.visible_counts(c)
        ln = torch.where(cnt > 0, torch.log(cnt.clamp(min=1)), torch.full_like(cnt, float("-inf")))
        ln = ln[:, None].expand(-1, Hq)
        assert ac.lse_mismatches(want_lse, ln, n_max)[0] == 0
        assert ac.lse_mismatches(lse, ln, n_max)[0] == 0
        if not causal:                         # the sequence without keys: zero output, LSE -inf
            a, b = c.cu[1].item(), c.cu[2].item()
            assert c.lk[1] == 0 and b > a
            assert torch.all(want[a:b] == 0) and torch.all(ln[a:b] == float("-inf"))
    else:
        # every row of the delta = 0 head sees its own key; most rows of the others see a member
        _check_leads(scores, sum(c.lens) * Hkv, what)
    for name, out, mlse in ac.mutants_prefill(c):
        _rejects(mis, out, want, f"{what} {name}")
        if kind == "uniform":
            assert ac.lse_mismatches(mlse, ln, n_max)[0] > 0, f"{what} {name}: LSE criterion blind"


def test_causal_shift_mutants_flag_nearly_every_row():
    """Shifting the causal mask by +1 changes the delta = +1 head on every row with a later key in
    its sequence; by -1 the delta = 0 head on every row."""
    c = ac.prefill_case("needle", 8, 1)
    want = ac.reference_prefill(c)[0]
    T = want.shape[0]
    muts = {name: out for name, out, _ in ac.mutants_prefill(c)}
    tol = 1e-3 + 2.0 ** -7 * want.abs()
    rows_p1 = ((muts["shift_plus_1"] - want).abs() > tol)[:, 1].any(-1).sum().item()
    rows_m1 = ((muts["shift_minus_1"] - want).abs() > tol)[:, 0].any(-1).sum().item()
    assert rows_p1 >= T - len(c.lens), rows_p1      # all but each sequence's last row
    assert rows_m1 >= T - len(c.lens), rows_m1


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("Hq,Hkv,chunks", ac.PAGED_CASES)
@pytest.mark.parametrize("kind", ["needle", "uniform"])
def test_paged_cases_are_sharp(kind, Hq, Hkv, chunks, fp8):
    c = ac.paged_case(kind, Hq, Hkv, fp8, chunks)
    what = f"paged {kind} Hq={Hq} Hkv={Hkv} nseq={len(chunks)} fp8={fp8}"
    mis = ac.mismatches_for(kind)
    want, scores = ac.reference_paged(c)
    o = ref.attn_prefill_paged(c.q, c.kc, c.vc, c.tables, c.cu, c.pos, c.max_q, ac.SCALE)
    _accepts(mis, o, want, what + " ops.reference")
    _accepts(mis, ac.reference_paged(c, emulate=True)[0], want, what + " bf16-P emulation")
    if kind == "needle":
        _check_leads(scores, c.q.shape[0] * Hkv, what)
    for name, out in ac.mutants_paged(c):
        _rejects(mis, out, want, f"{what} {name}")


def _merge_chunks(c, chunks):
    T = c.q.shape[0]
    acc = torch.zeros(T, c.Hq, ac.D, dtype=torch.float32)
    al = torch.full((T, c.Hq), float("-inf"), dtype=torch.float32)
    for k, v, cuk in chunks:
        o, lse = ref.attn_prefill(c.q, k, v, c.cu, c.max_seqlen, ac.SCALE, False, cu_seqlens_k=cuk, return_lse=True)
        ref.attn_lse_merge_(acc, al, o, lse)
    return acc, al


def test_lse_merge_case_is_sharp():
    """Attention over two key chunks merged by LSE equals attention over all keys; a merge whose
    first chunk lost its last key in one sequence does not."""
    c = ac.key_offsets_case()
    want, want_lse, _ = ac.reference_prefill(c)
    halves = ac.split_keys(c)
    assert sum(int(cuk[-1]) for _, _, cuk in halves) == sum(c.lk)
    acc, al = _merge_chunks(c, halves)
    _accepts(ac.uniform_mismatches, acc, want, "merged output")
    assert ac.lse_mismatches(al, want_lse, max(c.lk))[0] == 0
    # drop the last key of the first chunk of the longest sequence (129 keys: 64 + 65)
    (k, v, cuk), second = halves
    i = max(range(len(c.lk)), key=lambda j: c.lk[j])
    gone = int(cuk[i + 1]) - 1
    keep = torch.arange(k.shape[0]) != gone
    cuk2 = cuk.clone()
    cuk2[i + 1:] -= 1
    acc, al = _merge_chunks(c, [(k[keep].contiguous(), v[keep].contiguous(), cuk2), second])
    assert ac.uniform_mismatches(acc, want)[0] > 0
    assert ac.lse_mismatches(al, want_lse, max(c.lk))[0] > 0


def test_old_criterion_on_random_inputs_misses_one_key_at_700():
    """The gap these cases close: on the random-normal inputs of test_attn_decode_paged, a
    reference that drops the last key of the 700-key sequence, drops the key before a split
    edge, or includes one stale key past ctx moves the output by 0.01 .. 0.03 against
    atol = rtol = 2e-2. That test draws its block-table permutation unseeded, so whether a few
    elements fall outside is chance: for each mutant and head layout there is a permutation
    (among two) under which NOTHING is flagged, and never more than 1 % of the elements are."""
    lens = [1, 31, 32, 100, 700]

    def bf(*shape, seed):
        g = torch.Generator(device="cpu").manual_seed(seed)
        return torch.randn(*shape, generator=g).to(torch.bfloat16)

    for Hq, Hkv in ((16, 2), (64, 8)):
        mb = (max(lens) + 31) // 32
        nblk = len(lens) * mb + 3
        kc, vc = bf(nblk, Hkv, 32, 128, seed=24), bf(nblk, Hkv, 128, 32, seed=25)
        q = bf(len(lens), Hq, 128, seed=26)
        unnoticed = set()
        for perm_seed in (3, 7):
            bt = torch.randperm(nblk, generator=torch.Generator().manual_seed(perm_seed))
            bt = bt[: len(lens) * mb].view(len(lens), mb).to(torch.int32)
            want = ref.attn_decode(q, kc, vc, bt, torch.tensor(lens), ac.SCALE).double()
            k, v = ac._gather(kc, vc, bt[4], 701)
            for name, hide, show in (("drop_last", 699, None), ("drop_split_edge", 255, None),
                                     ("one_past_ctx", None, 700)):
                vis = torch.arange(701) < 700
                if hide is not None:
                    vis[hide] = False
                if show is not None:
                    vis[show] = True
                mut = want.clone()
                mut[4] = ac.attend(q[4:5].float(), k, v, vis[None])[0][0]
                bad, _ = ac.old_mismatches(mut, want)
                assert float((mut - want).abs().max()) > 2e-3, name      # the mutant did change the output
                assert bad <= 0.01 * mut[4].numel(), (name, perm_seed, bad)
                if bad == 0:
                    unnoticed.add(name)
        assert unnoticed == {"drop_last", "drop_split_edge", "one_past_ctx"}, (Hq, Hkv, unnoticed)


def test_hadamard_and_constants_are_exact():
    H = ac.hadamard()
    assert torch.equal(H @ H.t(), 128 * torch.eye(128))
    assert torch.equal(ac._poison_k_row(), 3 * H[:16].sum(0))
    vals = torch.tensor([ac.POISON_K, ac.POISON_V, 64.0, 1.0] + [2.0 * m for m in range(1, 9)])
    assert torch.equal(vals.to(torch.bfloat16).float(), vals)
    assert torch.equal(vals.to(ac.F8).float(), vals)
    assert math.isclose(ac.SCALE * 2 * 128, 22.627, abs_tol=1e-3)
