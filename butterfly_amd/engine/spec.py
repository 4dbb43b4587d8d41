"""Speculative decoding: draft proposers and the acceptance rule (host side).

The engine's sampling noise is keyed on (seed or request id, output index, token id), so "the
token the engine samples at output index i given the logits" is a deterministic function of the
logits. A verify step samples every row (row t of a sequence with the seed of output index
n_gen + t) and accepts the longest draft prefix whose tokens EQUAL the sampled ones: the emitted
tokens are exactly those of the non-speculative engine, greedy or seeded, with no rejection
sampling and no change of distribution. A wrong draft costs its rows, never correctness.

A proposer is any object with `propose(tokens: list, k: int) -> list` (at most k token ids that
might follow `tokens`); LLMEngine.proposer is replaceable. The default is prompt lookup.
"""
from __future__ import annotations

import numpy as np


class NgramProposer:
    """Prompt lookup: for n from ngram_max down to ngram_min, take the last n tokens of
    prompt + output, find their LATEST earlier occurrence that has at least one token after it,
    and propose the up to k tokens that follow it. The first n with a match wins; no match, no
    draft. No model, no device work: numpy over the sequence's own tokens."""

    def __init__(self, ngram_max: int = 4, ngram_min: int = 2):
        if ngram_min < 1 or ngram_min > ngram_max:
            raise ValueError(f"need 1 <= spec_ngram_min <= spec_ngram_max, got {ngram_min}, {ngram_max}")
        self.ngram_max, self.ngram_min = int(ngram_max), int(ngram_min)

    def propose(self, tokens: list, k: int) -> list:
        L = len(tokens)
        if k <= 0 or L < self.ngram_min + 1:
            return []
        t = np.asarray(tokens, dtype=np.int64)
        for n in range(min(self.ngram_max, L - 1), self.ngram_min - 1, -1):
            # windows starting at i in [0, L - n): the occurrence ends before the last token, so
            # at least one token follows it (i = L - n is the suffix itself)
            hit = np.ones(L - n, dtype=bool)
            for j in range(n):
                hit &= t[j:L - n + j] == t[L - n + j]
            idx = np.flatnonzero(hit)
            if idx.size:
                a = int(idx[-1]) + n
                return [int(x) for x in t[a:a + k]]
        return []


def accepted_prefix(draft: list, sampled: list) -> int:
    """Number of leading draft tokens that equal the tokens sampled at their positions:
    sampled[t] is the token of output index n_gen + t given draft[:t] was right."""
    a = 0
    while a < len(draft) and int(draft[a]) == int(sampled[a]):
        a += 1
    return a
