"""The attention kernels on inputs whose correct output names the keys that were read
(tests/attn_cases.py): needle + poison (which key is read, which must not be), uniform + poison
(how many keys are read, LSE = ln(count)), causal needle (the diagonal, the hidden keys after it,
the sequence boundary). Every criterion allows zero mismatching elements against an fp64
reference over the same bf16 / FP8 values; tests/test_attn_cases_cpu.py proves on the CPU that
each case rejects a reference with one key dropped, added or misplaced.

Each test prints its worst error as a fraction of the tolerance ("ATTN-FIGURE ...", pytest -s /
-rP) before it asserts. Measured on an MI355X, worst error / tolerance over all cases of a kind:

  decode needle 0.0000 (bf16 and FP8; 199 / 200 splits 0.0002), decode counts 0.18
  decode with V = 1 through 199 / 200 splits: exactly 1 (tolerance 2^-7)
  varlen prefill causal needle 0.35, counts 0.23, LSE 0.0022 (tolerance 0.25 / 641 = 3.9e-4)
  non-causal prefill with key offsets counts 0.065, LSE 0.0002 (tolerance 0.25 / 130)
  paged prefill needle 0.34 (FP8 0.33), counts 0.23
  LSE merge of two key chunks: output 0.13, LSE 0.0002
"""
import pytest
import torch

from butterfly_amd import ops

from . import attn_cases as ac

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(autouse=True, scope="module")
def _kernels_loaded():
    # GPU tests must run the HIP kernels: fail loudly if the library is missing
    assert ops.load_library(), "butterfly_amd/_C.so not built or failed to load"


def _check(label, mis, got, want, *extra):
    bad, worst = mis(got, want, *extra)
    print(f"ATTN-FIGURE {label}: worst err/tol {worst:.4f}, {bad} mismatches of {want.numel()}")
    assert bad == 0, f"{label}: {bad}/{want.numel()} mismatches, worst err/tol {worst:.3g}"


def _run_decode(c, q=None):
    q = c.q.to(DEV) if q is None else q
    ctx = torch.tensor(c.ctx, dtype=torch.int32, device=DEV)
    return ops.attn_decode(q, c.kc.to(DEV), c.vc.to(DEV), c.tables.to(DEV), ctx, ac.SCALE, c.max_ctx,
                           c.part_tokens)


@pytest.mark.parametrize("kind,Hq,Hkv,part_tokens,fp8", list(ac.decode_sweep()))
def test_attn_decode_position_sweep(kind, Hq, Hkv, part_tokens, fp8):
    """Paged decode, G = 16 / 3 / 1 / 8, contexts 1 .. 700 in one batch (the short ones leave
    empty splits), bf16 and FP8 caches. Needle: every (sequence, kv head, query head) reads its
    own position: the ends, both sides of split and page edges, the ragged last page, every wave's
    page stream; every slot that must not be read outscores the needle. Uniform: out n / 64
    counts the keys read per residue mod 128."""
    c = ac.decode_case(kind, Hq, Hkv, part_tokens, fp8)
    want = ac.reference_decode(c)[0]
    got = _run_decode(c)
    _check(f"decode {kind} Hq={Hq} Hkv={Hkv} part={part_tokens} {'fp8' if fp8 else 'bf16'}",
           ac.mismatches_for(kind), got, want)


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("ctx", ac.MANY_SPLIT_CTX)
@pytest.mark.parametrize("kind", ["needle", "uniform"])
def test_attn_decode_many_splits(kind, ctx, fp8):
    """200 and 199 splits (B = 1, Hkv = 1, 32-token splits): the combine kernel's 64- and
    128-split strides and its ns % 4 tail. Needles in splits 0, 63, 64, 127, 128 and the last;
    uniform with V = 1 must give 1 to one bf16 step (|got - 1| <= 2^-7: 196 / 199 from a lost
    tail is outside), poison shows any extra key."""
    c = ac.many_split_case(kind, ctx, fp8)
    assert (c.max_ctx + c.part_tokens - 1) // c.part_tokens in (199, 200)
    want = ac.reference_decode(c)[0]
    got = _run_decode(c)
    _check(f"decode many-splits {kind} ctx={ctx} {'fp8' if fp8 else 'bf16'}", ac.mismatches_for(kind, c.v_ones), got, want)


def test_attn_decode_strided_q_needle():
    # q as a view into a fused QKV row (row stride > Hq*D), as the model passes it
    c = ac.strided_case()
    B, Hq, Hkv = len(c.ctx), c.Hq, c.Hkv
    qkv = torch.full((B, (Hq + 2 * Hkv) * ac.D), 7.0, dtype=torch.bfloat16, device=DEV)
    q = qkv[:, : Hq * ac.D].view(B, Hq, ac.D)
    q.copy_(c.q)
    assert not q.is_contiguous()
    _check("decode strided q needle", ac.needle_mismatches, _run_decode(c, q), ac.reference_decode(c)[0])


def _run_prefill(c, k=None, v=None, cuk=None):
    kw = {} if c.causal else {"cu_seqlens_k": (c.cuk if cuk is None else cuk).to(DEV)}
    k = c.k if k is None else k
    v = c.v if v is None else v
    return ops.attn_prefill(c.q.to(DEV), k.to(DEV), v.to(DEV), c.cu.to(DEV), c.max_seqlen, ac.SCALE,
                            c.causal, return_lse=True, **kw)


def _ln_counts(c):
    cnt = ac.visible_counts(c)
    ln = torch.where(cnt > 0, torch.log(cnt.clamp(min=1)), torch.full_like(cnt, float("-inf")))
    return ln[:, None].expand(-1, c.Hq)


@pytest.mark.parametrize("kind,Hq,Hkv", ac.PREFILL_CAUSAL_CASES)
def test_attn_prefill_causal_cases(kind, Hq, Hkv):
    """Varlen flash prefill on sequences of 1, 37, 300, 640, 2 rows (64-key tiles, the 256-row
    query block, 32-row wave slices, the ring wrap; 1- and 2-row sequences next to long ones),
    G = 8 with one and two kv heads. Causal needle: the 8 heads of a group want the key 0, +1, +2,
    -1, -63, -64, -65, -128 rows away. Uniform: counts per residue, and LSE = ln(row + 1) to
    0.25 / 641 (measured worst error / tolerance: see the ATTN-FIGURE lines)."""
    c = ac.prefill_case(kind, Hq, Hkv)
    want = ac.reference_prefill(c)[0]
    got, lse = _run_prefill(c)
    label = f"prefill causal {kind} Hq={Hq} Hkv={Hkv}"
    _check(label, ac.mismatches_for(kind), got, want)
    if kind == "uniform":
        _check(label + " LSE", ac.lse_mismatches, lse, _ln_counts(c), max(c.lk))


def test_attn_prefill_key_offsets_uniform():
    """Non-causal with keys from other rows (cu_seqlens_k), 5, 0, 129, 64, 65 keys per sequence:
    counts per residue, LSE = ln(keys); the sequence without keys gives zeros and LSE = -inf."""
    c = ac.key_offsets_case()
    want = ac.reference_prefill(c)[0]
    got, lse = _run_prefill(c)
    _check("prefill non-causal uniform", ac.uniform_mismatches, got, want)
    _check("prefill non-causal uniform LSE", ac.lse_mismatches, lse, _ln_counts(c), max(c.lk))
    a, b = int(c.cu[1]), int(c.cu[2])
    assert torch.all(got[a:b] == 0) and torch.all(lse[a:b] == float("-inf"))


def test_attn_lse_merge_of_key_chunks():
    """K3's LSE and K16 end to end: attention over the two halves of every sequence's keys,
    merged by attn_lse_merge_, is attention over all keys (uniform criteria, unsplit reference)."""
    c = ac.key_offsets_case()
    want, want_lse, _ = ac.reference_prefill(c)
    acc = torch.zeros(want.shape, dtype=torch.float32, device=DEV)
    al = torch.full(want_lse.shape, float("-inf"), dtype=torch.float32, device=DEV)
    for k, v, cuk in ac.split_keys(c):
        o, lse = _run_prefill(c, k, v, cuk)
        ops.attn_lse_merge_(acc, al, o, lse)
    _check("lse merge output", ac.uniform_mismatches, acc, want)
    _check("lse merge LSE", ac.lse_mismatches, al, _ln_counts(c), max(c.lk))


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("Hq,Hkv,chunks", ac.PAGED_CASES)
@pytest.mark.parametrize("kind", ["needle", "uniform"])
def test_attn_prefill_paged_cases(kind, Hq, Hkv, chunks, fp8):
    """Chunked prefill over the paged cache: (prefix, chunk) = (0, 37), (31, 1), (95, 50),
    (700, 16), (250, 129) over a pool with holes (the LDS ring kernel at both ring depths), and
    the single sequence (700, 129) (the register kernel, 1 and 2 heads per wave). Causal
    needle by position in the sequence; uniform with poison in the stale slots of the last page
    and behind every spare table entry."""
    c = ac.paged_case(kind, Hq, Hkv, fp8, chunks)
    want = ac.reference_paged(c)[0]
    got = ops.attn_prefill_paged(c.q.to(DEV), c.kc.to(DEV), c.vc.to(DEV), c.tables.to(DEV), c.cu.to(DEV),
                                 c.pos.to(DEV), c.max_q, ac.SCALE)
    _check(f"paged {kind} Hq={Hq} Hkv={Hkv} nseq={len(chunks)} {'fp8' if fp8 else 'bf16'}",
           ac.mismatches_for(kind), got, want)
