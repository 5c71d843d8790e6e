"""CPU-only: the float64 restatement of the silhouette coefficient (tests/_silhouette_ref.py) against sklearn's recorded values
(tests/golden/silhouette.npz) and, where scikit-learn and scipy are installed, against sklearn itself; the API refuses CPU tensors."""
import os

import numpy as np
import pytest
import torch

import _kmeans_inputs as KI
import _silhouette_inputs as SI
import _silhouette_ref as SR

RECORDED = [("shipped", "nearest"), ("small", "nearest"), ("small", "skewed"), ("mid", "nearest")]


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "silhouette.npz"))


def check_rows(N):
    """every row up to 1500 rows; beyond, the rows of the planted pairs and 200 seeded ones (the restatement costs N x E per row)"""
    if N <= 1500:
        return np.arange(N)
    return np.unique(np.concatenate([np.arange(0, 70), np.random.default_rng(N).choice(N, 200, replace=False)]))


@pytest.mark.parametrize("name,which", RECORDED)
def test_restatement_equals_the_recorded_sklearn_values(fx, name, which):
    X, sets, _ = SI.case(name)
    lab = sets[which]
    assert KI.sha(X) == str(fx[f"{name}_sha_x"]) and KI.sha(lab) == str(fx[f"{name}_{which}_sha_labels"])
    assert np.array_equal(fx[f"{name}_{which}_labels"].astype(np.int64), lab)
    rows = check_rows(len(lab))
    s = SR.terms(SR.distances(X, rows), lab, rows)[2]
    err = float(np.abs(s - fx[f"{name}_{which}_s"][rows]).max())
    print(f"{name}/{which}: {len(rows)} rows, restatement within {err:.2e} of the recorded values")
    assert err <= 1e-12


def test_restatement_equals_sklearn():
    metrics = pytest.importorskip("sklearn.metrics")
    distance = pytest.importorskip("scipy.spatial.distance")
    X, sets, _ = SI.case("small")
    X64 = X.astype(np.float64)
    D = distance.cdist(X64, X64)
    mine = SR.distances(X)
    for which, lab in sets.items():
        sk = metrics.silhouette_samples(D, lab, metric="precomputed")
        err = float(np.abs(SR.terms(mine, lab)[2] - sk).max())
        print(f"small/{which}: restatement within {err:.2e} of sklearn")
        assert err <= 1e-12


def test_edge_rules_of_the_restatement():
    X = np.array([[0.0, 0.0], [3.0, 4.0], [3.0, 4.0], [9.0, 9.0]], np.float32)
    a, b, s = SR.terms(SR.distances(X), np.array([0, 1, 1, 2]))
    assert a[0] == 0.0 and s[0] == 0.0 and s[3] == 0.0          # clusters of one row
    assert a[1] == 0.0 and a[2] == 0.0 and b[1] == 5.0 and s[1] == 1.0
    a, b, s = SR.terms(SR.distances(np.ones((4, 2), np.float32)), np.array([0, 0, 1, 1]))
    assert not np.isnan(s).any() and np.all(s == 0.0)            # a = b = 0


def test_api_refuses_cpu_tensors():
    from gesture2vec_amd.silhouette import silhouette_samples, silhouette_score
    x, lab = torch.zeros(8, 4), torch.arange(8) % 2
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        silhouette_samples(x, lab)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        silhouette_score(x, lab, sample_size=4, random_state=0)
