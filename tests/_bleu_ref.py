"""The `Counter` restatement of `torchtext.data.metrics.bleu_score` for ONE candidate sentence against ONE reference (what the
reference's `Metrics_analysis` calls per test case, Clustering.py:1590-1595), in exact integers and float64, and the generator of the
(candidate, reference) pairs the BLEU tests share.  torchtext itself forms the score in float32 and is not installed here."""
import math
from collections import Counter

import numpy as np

KS = (3, 512, 65536)
SUB = {3: 0.3, 512: 0.1, 65536: 0.05}                   # probability that a candidate id differs from the reference's
LENGTHS = (0, 1, 3, 4, 5, 8, 63, 64, 65, 255, 256, 257, 1000, 1024, 1025, 4095, 4096)       # candidate lengths
MAX_LEN = 4096


def ngram_counter(seq, n):
    seq = [int(v) for v in seq]
    return Counter(tuple(seq[i:i + n]) for i in range(len(seq) - n + 1))


def clipped_counts(cand, ref, max_n=4):
    """[sum((Counter(cand n-grams) & Counter(ref n-grams)).values()) for n = 1 .. max_n]"""
    return [sum((ngram_counter(cand, n) & ngram_counter(ref, n)).values()) for n in range(1, max_n + 1)]


def total_counts(cand_len, max_n=4):
    return [max(cand_len - n + 1, 0) for n in range(1, max_n + 1)]


def score_from_counts(clipped, total, cand_len, ref_len, weights=None):
    max_n = len(clipped)
    weights = [1.0 / max_n] * max_n if weights is None else weights
    if min(clipped) == 0:
        return 0.0
    log_pn = sum(w * math.log(c / t) for w, c, t in zip(weights, clipped, total))
    return math.exp(min(1.0 - ref_len / cand_len, 0.0)) * math.exp(log_pn)


def bleu(cand, ref, max_n=4, weights=None):
    return score_from_counts(clipped_counts(cand, ref, max_n), total_counts(len(cand), max_n), len(cand), len(ref), weights)


def corpus_bleu(pairs, max_n=4, weights=None):
    """torchtext's corpus of several sentences with one reference each: counts and lengths summed first"""
    clipped, total = np.zeros(max_n, np.int64), np.zeros(max_n, np.int64)
    lc = lr = 0
    for cand, ref in pairs:
        clipped += np.asarray(clipped_counts(cand, ref, max_n))
        total += np.asarray(total_counts(len(cand), max_n))
        lc, lr = lc + len(cand), lr + len(ref)
    return score_from_counts([int(v) for v in clipped], [int(v) for v in total], lc, lr, weights)


def clipping_directions(cand, ref, max_n=4):
    """(some n-gram has candidate count > reference count > 0, some n-gram has reference count > candidate count > 0)"""
    more = less = False
    for n in range(1, max_n + 1):
        c, r = ngram_counter(cand, n), ngram_counter(ref, n)
        for g, v in c.items():
            more |= v > r.get(g, 0) > 0
            less |= r.get(g, 0) > v > 0
    return more, less


def make_pair(rng, K, cand_len, sub=None, max_len=MAX_LEN):
    """A reference drawn uniformly over K; the candidate is the reference with each id replaced with probability `sub`, then cut or
    grown by up to 3 ids to exactly `cand_len` (so the reference's length differs from the candidate's by up to 3, inside
    [0, max_len])."""
    sub = SUB[K] if sub is None else sub
    delta = int(rng.integers(-3, 4))
    ref_len = min(max(cand_len + delta, 0), max_len)
    ref = rng.integers(0, K, ref_len, dtype=np.int64)
    cand = ref.copy()
    swap = rng.random(ref_len) < sub
    cand[swap] = rng.integers(0, K, int(swap.sum()), dtype=np.int64)
    if cand_len <= ref_len:
        cand = cand[:cand_len]
    else:
        cand = np.concatenate([cand, rng.integers(0, K, cand_len - ref_len, dtype=np.int64)])
    return cand, ref


def pairs_for(K, lengths=LENGTHS, per_length=1, seed=0, max_len=MAX_LEN):
    rng = np.random.default_rng(1000 * seed + K)
    return [make_pair(rng, K, L, max_len=max_len) for L in lengths for _ in range(per_length)]
