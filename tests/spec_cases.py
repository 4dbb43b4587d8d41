"""The attn_verify cases of tests/test_spec_gpu.py, shared with tests/test_spec_cpu.py, which
proves them sharp (every mutant reference is rejected by the criterion the GPU test uses).

A verify call over QN rows per sequence is a paged chunk of attn_cases.paged_case with
(prefix, q_len) per sequence: row t sits at position prefix + t and sees keys [0, prefix + t],
which is ctx_lens = prefix + 1 and q_lens = q_len in the kernel's terms. q_len is ragged in
1 .. QN; the chunk sets cover prefix 0 / 31 / 32 / 33 (page edges), limits that straddle the
split edges of the forced part_tokens = 64 (63 / 64 / 65, 127 / 128 / 129), and a short sequence
beside a long one (whose later splits are empty for the short one)."""
import torch

from . import attn_cases as ac

PART = 64
HEADS = ((4, 2), (8, 2), (8, 1), (16, 16))      # G = 2, 4, 8, 1: with QN below 1 .. 4 column tiles
CHUNKS = {
    2: ((0, 1), (31, 2), (32, 2), (33, 1), (63, 2), (200, 2)),
    3: ((0, 3), (31, 1), (32, 3), (33, 2), (62, 3), (127, 2), (200, 3)),
    5: ((0, 5), (31, 4), (32, 1), (33, 5), (60, 5), (126, 3), (200, 2)),
    8: ((0, 8), (31, 8), (32, 5), (33, 1), (57, 8), (121, 8), (250, 7)),
}


def sweep():
    for kind in ("needle", "uniform"):
        for Hq, Hkv in HEADS:
            for QN in sorted(CHUNKS):
                for fp8 in (False, True):
                    yield kind, Hq, Hkv, QN, fp8


def case(kind, Hq, Hkv, QN, fp8):
    return ac.paged_case(kind, Hq, Hkv, fp8, chunks=CHUNKS[QN], seed=700 + QN)


def tiles(Hq, Hkv, QN):
    return (QN * (Hq // Hkv) + 15) // 16


def verify_inputs(c, QN):
    """The case in attn_verify's layout: q [B, QN, Hq, D] (padding rows repeat the sequence's
    last valid row), ctx_lens / q_lens [B] int32, max_ctx, and for every (b, t) the row of
    c.q whose reference output the kernel must reproduce there (padding: the last valid row's)."""
    cu = c.cu.tolist()
    B = len(c.chunks)
    q4 = torch.zeros(B, QN, c.Hq, ac.D, dtype=c.q.dtype)
    src = torch.zeros(B, QN, dtype=torch.long)
    for b, (pre, ql) in enumerate(c.chunks):
        assert 1 <= ql <= QN
        for t in range(QN):
            src[b, t] = cu[b] + min(t, ql - 1)
        q4[b] = c.q[src[b]]
    i32 = lambda a: torch.tensor(a, dtype=torch.int32)  # noqa: E731
    return dict(q=q4, ctx_lens=i32([pre + 1 for pre, _ in c.chunks]), q_lens=i32([ql for _, ql in c.chunks]),
                max_ctx=max(pre for pre, _ in c.chunks) + 1, src=src)


# ---------------------------------------------------------------------------------------
# Draft proposers of the engine tests
# ---------------------------------------------------------------------------------------
class OracleProposer:
    """Proposes what a reference run generated for the same prompts: every draft is right for
    as long as the speculative run reproduces that run. `extra`: tokens returned beyond the k
    asked for (the engine must cut them); `wrong`: every proposed token is the right one + 1
    (mod vocab), so no draft is ever accepted."""

    def __init__(self, prompts, outs, extra=0, wrong=False, vocab=0):
        self.full = [list(p) + list(o) for p, o in zip(prompts, outs)]
        self.plen = [len(p) for p in prompts]
        self.extra, self.wrong, self.vocab = extra, wrong, vocab
        self.calls = []

    def continuation(self, tokens, n):
        for full, pl in zip(self.full, self.plen):
            if len(tokens) >= pl and list(tokens) == full[:len(tokens)]:
                return full[len(tokens):len(tokens) + n]
        return []

    def propose(self, tokens, k):
        self.calls.append((len(tokens), k))
        d = self.continuation(tokens, k + self.extra)
        return [(t + 1) % self.vocab for t in d] if self.wrong else d


class RandomProposer:
    """Ragged drafts of 0 .. k tokens, each the right token with probability 1/2 and a random
    one otherwise: partial acceptance at every length."""

    def __init__(self, oracle, vocab, seed=0):
        self.oracle, self.vocab = oracle, vocab
        self.g = torch.Generator().manual_seed(seed)

    def _r(self, n):
        return int(torch.randint(0, n, (1,), generator=self.g))

    def propose(self, tokens, k):
        n = self._r(k + 1)
        right = self.oracle.continuation(tokens, n)
        return [right[i] if i < len(right) and self._r(2) else self._r(self.vocab) for i in range(n)]
