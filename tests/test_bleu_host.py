"""CPU-only: the `Counter` restatement of torchtext's bleu_score (tests/_bleu_ref.py) against hand values, `metrics.bleu_from_counts`
on CPU tensors against the restatement, and the refusals of `code_bleu` that need no GPU.

Tolerance 1e-12 relative: the counts are exact integers and both sides evaluate four logs, one weighted sum and two exps in float64;
the error is a few ulp (2.2e-16 each), amplified by an exponent below 10 in magnitude."""
import math
import os
import re

import numpy as np
import pytest
import torch

import _bleu_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-12


def test_restatement_against_hand_values():
    assert R.clipped_counts([1, 2, 3, 4, 5], [1, 2, 3, 4, 6]) == [4, 3, 2, 1]
    assert R.bleu([1, 2, 3, 4, 5], [1, 2, 3, 4, 6]) == pytest.approx(0.2 ** 0.25, rel=1e-15)       # (4/5 3/4 2/3 1/2)^(1/4)
    assert R.bleu([1, 2, 3, 4], [1, 2, 3, 4, 5, 6]) == pytest.approx(math.exp(-0.5), rel=1e-15)    # every precision 1, brevity 1 - 6/4
    assert R.clipped_counts([7] * 6, [7, 7]) == [2, 1, 0, 0] and R.bleu([7] * 6, [7, 7]) == 0.0
    for L in (4, 5, 64, 1000):
        seq = list(np.random.default_rng(L).integers(0, 7, L))
        assert R.bleu(seq, seq) == pytest.approx(1.0, rel=1e-15)
    for L in (0, 1, 2, 3):
        seq = list(range(L))
        assert R.bleu(seq, seq) == 0.0 and R.bleu(seq, [0, 1, 2, 3, 4]) == 0.0
    assert R.bleu([1, 2, 3, 4, 5], []) == 0.0


@pytest.mark.parametrize("K", R.KS)
def test_generated_pairs_exercise_the_score(K):
    """guards against a comparison of zeros with zeros: asserted on the restatement alone"""
    pairs = R.pairs_for(K, per_length=4)
    scores = [R.bleu(c, r) for c, r in pairs]
    assert sum(s > 0 for s in scores) * 2 >= len(scores), (K, sum(s > 0 for s in scores), len(scores))
    assert all(len(c) in R.LENGTHS and abs(len(c) - len(r)) <= 3 for c, r in pairs)
    if K == 3:
        dirs = [R.clipping_directions(c, r) for c, r in pairs]
        assert any(m for m, _ in dirs) and any(l for _, l in dirs)


@pytest.mark.parametrize("K", R.KS)
@pytest.mark.parametrize("max_n", [1, 2, 4])
def test_bleu_from_counts_on_the_cpu(K, max_n):
    from gesture2vec_amd.metrics import bleu_from_counts
    pairs = R.pairs_for(K, per_length=2)
    clipped = torch.tensor([R.clipped_counts(c, r, max_n) for c, r in pairs], dtype=torch.int64)
    lc = torch.tensor([len(c) for c, _ in pairs], dtype=torch.int64)
    lr = torch.tensor([len(r) for _, r in pairs], dtype=torch.int64)
    got = bleu_from_counts(clipped, lc, lr)
    assert got.dtype == torch.float64 and got.shape == (len(pairs),) and got.device.type == "cpu"
    want = np.array([R.bleu(c, r, max_n) for c, r in pairs])
    assert np.array_equal(got.numpy() == 0, want == 0)
    assert np.all(np.abs(got.numpy() - want) <= RTOL * want)
    weights = [0.4, 0.3, 0.2, 0.1][:max_n]
    got_w = bleu_from_counts(clipped, lc, lr, weights=weights).numpy()
    want_w = np.array([R.bleu(c, r, max_n, weights) for c, r in pairs])
    assert np.all(np.abs(got_w - want_w) <= RTOL * want_w)
    corpus = bleu_from_counts(clipped, lc, lr, corpus=True)
    want_c = R.corpus_bleu(pairs, max_n)
    assert corpus.dim() == 0 and want_c > 0 and abs(float(corpus) - want_c) <= RTOL * want_c
    with pytest.raises(ValueError, match="weights"):
        bleu_from_counts(clipped, lc, lr, weights=[1.0] * (max_n + 1))


def test_bleu_from_counts_zero_rows_and_shapes():
    from gesture2vec_amd.metrics import bleu_from_counts
    clipped = torch.tensor([[0, 0, 0, 0], [2, 1, 0, 0], [5, 4, 3, 2]])
    got = bleu_from_counts(clipped, torch.tensor([0, 6, 5]), torch.tensor([3, 2, 5]))
    assert got.tolist() == [0.0, 0.0, 1.0] and not torch.isnan(got).any()
    assert float(bleu_from_counts(clipped[:2], torch.tensor([0, 6]), torch.tensor([3, 2]), corpus=True)) == 0.0
    with pytest.raises(ValueError, match="clipped"):
        bleu_from_counts(clipped, torch.tensor([1, 2]), torch.tensor([1, 2, 3]))


def test_code_bleu_refusals_without_a_gpu():
    from gesture2vec_amd.metrics import code_bleu
    a = torch.zeros(2, 5, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        code_bleu(a, a, K=8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        code_bleu([a[0], a[1]], [a[0], a[1]], K=8)
    for K in (0, -1, 65537):
        with pytest.raises(ValueError, match="65536"):
            code_bleu(a, a, K=K)
    with pytest.raises(ValueError, match="max_n"):
        code_bleu(a, a, K=8, max_n=5)
    with pytest.raises(ValueError, match="int64"):
        code_bleu(a.float(), a, K=8)


def test_the_entry_is_declared():
    import ctypes as C
    from gesture2vec_amd import _lib
    assert "g2v_ngram_clipped_counts" in _lib.EXPORTS
    res, args = _lib._SIGS["g2v_ngram_clipped_counts"]
    assert res is C.c_int and args == [C.c_void_p] * 8 + [C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p]
    assert hasattr(_lib.load(), "g2v_ngram_clipped_counts")
    assert len(_lib.STRUCTS) == 10                                        # the entry brought no struct
    text = open(os.path.join(ROOT, "gesture2vec_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bngram\.hip\b", text, re.M)
