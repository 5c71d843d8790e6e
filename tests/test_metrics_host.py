"""CPU-only: the host half of gesture2vec_amd.metrics -- the four metric functions against the reference's own values
(tests/golden/metrics.npz, written by tests/golden/make_fixtures_metrics.py) and LatentMoments' state algebra on states built with
numpy."""
import os

import numpy as np
import pytest

import _metrics_inputs as MI


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "metrics.npz"))


@pytest.mark.parametrize("case", sorted(MI.FRECHET_CASES))
def test_frechet_distance_matches_the_reference(fx, case):
    """float64 np.mean / np.cov inputs, as the reference feeds its calculate_frechet_distance; bound: the project's parity bar"""
    from gesture2vec_amd.metrics import frechet_distance
    A, B = MI.frechet_inputs(case)
    assert [MI.sha256(A), MI.sha256(B)] == list(fx[f"frechet/{case}/sha256"]), "the regenerated inputs differ from the fixture's"
    assert list(fx[f"frechet/{case}/shape"]) == list(MI.FRECHET_CASES[case])
    assert min(A.shape[0], B.shape[0]) > A.shape[1]                     # parity is claimed for n > E only
    got = frechet_distance(np.mean(A, axis=0), np.cov(A, rowvar=False), np.mean(B, axis=0), np.cov(B, rowvar=False))
    ref = float(fx[f"frechet/{case}/value"])
    print(f"frechet {case}: got {got!r} ref {ref!r} rel {abs(got - ref) / abs(ref):.3e}")
    assert abs(got - ref) <= 1e-4 * abs(ref)


@pytest.mark.parametrize("case", sorted(MI.HIST_CASES))
def test_histogram_metrics_match_the_reference(fx, case):
    from gesture2vec_amd import metrics as M
    i1, i2 = MI.hist_inputs(case)
    assert [MI.sha256(i1), MI.sha256(i2)] == list(fx[f"hist/{case}/sha256"])
    h1, h2 = np.bincount(i1, minlength=MI.HIST_K), np.bincount(i2, minlength=MI.HIST_K)
    assert (h1 == 0).any() and (h2 == 0).any()

    def close(got, ref):
        assert abs(got - float(ref)) <= 1e-12 * abs(float(ref)), (got, float(ref))
    close(M.hellinger(h1, h2), fx[f"hist/{case}/hellinger"])
    close(M.wasserstein(h1, h2), fx[f"hist/{case}/wasserstein"])
    close(M.histogram_perplexity(h1), fx[f"hist/{case}/perplexity"][0])
    close(M.histogram_perplexity(h2), fx[f"hist/{case}/perplexity"][1])


def _np_state(x, shift):
    d = x.astype(np.float64) - shift.astype(np.float64)
    return {"E": x.shape[1], "n": np.int64(x.shape[0]), "shift": shift, "s1": d.sum(0), "s2": d.T @ d}


def test_moments_state_algebra_on_the_host():
    """three unequal parts, loaded and merged == the one-part state, and both == np.mean / np.cov, to float64 rounding"""
    from gesture2vec_amd.metrics import LatentMoments
    A, _ = MI.frechet_inputs("narrow")
    E = A.shape[1]
    shift = A[:256].mean(0).astype(np.float32)
    whole = LatentMoments(E, "cpu").load_state(_np_state(A, shift))
    parts = [LatentMoments(E, "cpu").load_state(_np_state(p, shift)) for p in (A[:100], A[100:733], A[733:])]
    merged = parts[0].merge(parts[1]).merge(parts[2])
    n, mu, cov = merged.finalize()
    n1, mu1, cov1 = whole.finalize()
    assert n == n1 == A.shape[0] and isinstance(merged.state()["n"], np.int64)
    scale = np.abs(cov1).max()
    assert np.abs(mu - mu1).max() <= 1e-13 * np.abs(mu1).max() and np.abs(cov - cov1).max() <= 1e-12 * scale
    A64 = A.astype(np.float64)
    assert np.abs(mu - A64.mean(0)).max() <= 1e-12 * np.abs(mu1).max()
    assert np.abs(cov - np.cov(A64, rowvar=False)).max() <= 1e-10 * scale
    st = merged.state()                                                  # state() -> load_state() round trip
    again = LatentMoments(E, "cpu").load_state(st)
    assert np.array_equal(again.state()["s2"], st["s2"]) and np.array_equal(again.state()["shift"], shift)
    calls = []
    again.all_reduce(lambda t: calls.append(str(t.dtype)) or t.mul_(2))   # a two-rank SUM of identical shards
    assert calls == ["torch.float64", "torch.int64"]
    n2, mu2, _ = again.finalize()
    assert n2 == 2 * n and np.abs(mu2 - mu).max() <= 1e-13 * np.abs(mu).max()


def test_moments_refuse_what_cannot_be_computed():
    import torch
    from gesture2vec_amd.metrics import LatentMoments
    A, _ = MI.frechet_inputs("narrow")
    E = A.shape[1]
    shift = np.zeros(E, np.float32)
    with pytest.raises(ValueError, match="at least 2 rows"):
        LatentMoments(E, "cpu").load_state(_np_state(A[:1], shift)).finalize()
    with pytest.raises(ValueError, match="at least 2 rows"):
        LatentMoments(E, "cpu", shift=shift).finalize()
    a = LatentMoments(E, "cpu").load_state(_np_state(A[:50], shift))
    b = LatentMoments(E, "cpu").load_state(_np_state(A[50:90], shift + np.float32(0.5)))
    with pytest.raises(ValueError, match="different shifts"):
        a.merge(b)
    with pytest.raises(ValueError, match="widths differ"):
        a.merge(LatentMoments(E + 1, "cpu"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        a.update(torch.from_numpy(A[:10]))
