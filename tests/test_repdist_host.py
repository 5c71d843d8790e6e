"""CPU-only: the float64 restatement of the pairwise-distance statistics (tests/_repdist_ref.py) against scipy's / numpy's recorded
values and the reference's own Rep_distance.txt numbers (tests/golden/repdist.npz), the edge-gap precondition and the hashes of
every fixture input, and the argument refusals of gesture2vec_amd.repdist that need no device."""
import os
import random

import numpy as np
import pytest
import torch

import _repdist_inputs as RI
import _repdist_ref as RR
from gesture2vec_amd import metrics, repdist


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "repdist.npz"))


@pytest.fixture(scope="module")
def sequence_rows(fx):
    N, E = (int(v) for v in fx["reference/shape"])
    X = RI.sequence(N, E, int(fx["reference/seeds"][0]))
    return X, RR.lag_distances(X), RR.stats(X)


@pytest.mark.parametrize("shape", RI.GENERIC, ids=RI.name_of)
def test_restatement_against_scipy(fx, shape):
    N, E = shape
    key = f"pdist/{RI.name_of(shape)}/"
    X = RI.clustered(N, E, int(fx[key + "seed"]))
    assert RI.sha256(X) == str(fx[key + "sha256"])
    ref = RR.stats(X)
    assert ref["count"] == N * (N - 1) // 2 and ref["nonfinite"] == 0
    for k in ("mean", "min", "max"):
        assert abs(ref[k] - float(fx[key + k])) <= RR.bar_sum(E) * float(fx[key + k]), k
    var = float(fx[key + "std"]) ** 2
    assert abs(ref["std"] - float(fx[key + "std"])) <= RR.bar_std(E, float(fx[key + "mean"]), var) * float(fx[key + "std"])
    assert abs(ref["sum_sq"] / ref["count"] - (var + float(fx[key + "mean"]) ** 2)) <= RR.bar_sq(E) * ref["sum_sq"] / ref["count"]
    hi = float(fx[key + "hi"])
    assert hi == RI.hist_hi(float(fx[key + "max"]))
    edges = repdist.histogram_edges(RI.HIST_BINS, (0.0, hi))
    assert np.array_equal(edges, np.histogram_bin_edges(ref["d"], RI.HIST_BINS, (0.0, hi)))
    assert RR.edge_gap(ref["d"], edges) > RR.EDGE_GAP                 # the precondition of equal histograms
    hist = RR.histogram(ref["d"], edges)
    assert np.array_equal(hist, fx[key + "hist"]) and int(hist.sum()) == ref["count"]


def test_histogram_rule_is_numpys():
    rng = np.random.default_rng(3)
    d = np.concatenate([rng.uniform(-1.0, 6.0, 5000), [0.5, 2.0, 5.0, 5.0, np.nan, np.inf, 0.0]])
    for edges in (np.linspace(0.5, 5.0, 8), np.array([0.0, 0.1, 2.0, 2.5, 5.0]), np.array([1.0, 3.0])):
        want = np.histogram(d[~np.isnan(d)], edges)[0]
        assert np.array_equal(RR.histogram(d, edges), want)
    assert RR.edge_gap(np.array([1.0, 2.0]), [0.0, 2.0 * (1 + 1e-10)]) < RR.EDGE_GAP < RR.edge_gap(np.array([1.0, 2.0]), [0.0, 2.1])
    assert RR.edge_gap(np.array([0.0, 2.0]), [0.0, 2.0], skip_equal=True) == 1.0


def test_restatement_against_the_reference(fx, sequence_rows):
    X, lagd, st = sequence_rows
    N, E = X.shape
    assert N >= 1004 and RI.sha256(X) == str(fx["reference/sha256"])
    seed = int(fx["reference/seeds"][1])
    ref_bar = float(fx["reference/ref_bar"])
    assert 0 < ref_bar < 1e-6                                         # float32 sums of ~1000 float32 values: 1e-7, not more
    for method in ("all", "random"):
        want = dict(zip(RR.KEYS, fx[f"reference/{method}"]))
        got = RR.representation_similarity(X, method, seed=seed, avg_total=st["mean"], lagd=lagd)
        assert abs(got["avg_dist_total"] - want["avg_dist_total"]) <= RR.bar_sum(E) * want["avg_dist_total"]
        for k in RR.NEIGHBOUR_KEYS:
            assert abs(got[k] - want[k]) <= ref_bar * abs(want[k]), (method, k)
        assert got["avg_20fs"] < got["avg_10fs"] < 0.2 * got["avg_dist_total"]      # the rows do follow each other in time
    random.seed(seed)
    assert random.sample(range(2, N - 2), 1000) == repdist.similarity_rows(N, "random", 1000, seed) == RR.similarity_rows(N, "random", 1000, seed)
    assert list(repdist.similarity_rows(N, "all")) == list(range(2, N - 2))


def test_lag_rules_of_the_restatement():
    X = RI.clustered(9, 5, 1)
    ids = np.array([0, 0, 0, 1, 2, 2, 2, 2, 2])
    out = RR.lag_distances(X, (1, 3, 9), ids)
    assert np.flatnonzero(~np.isnan(out[0])).tolist() == [1, 5, 6, 7] and np.isnan(out[1:]).all()
    assert np.flatnonzero(~np.isnan(RR.lag_distances(X, (3,))[0])).tolist() == [3, 4, 5]


def test_parse_report_round_trip(fx):
    vals = {m: dict(zip(RR.KEYS, (float(v) for v in fx[f"reference/{m}"]))) for m in ("all", "random")}
    text = "=====Representation similarity at the embedding space.=====\n\n"
    for m, r in vals.items():
        text += (f"\n\n==========================\nMethod: {m}\nRepresentation Similarity metric\navg_20fs={r['avg_20fs']} -- "
                 f"std_20fs={r['std_20fs']}\navg_10fs={r['avg_10fs']} -- std_10fs={r['std_10fs']}\n\nStandardized:\naverage distance "
                 f"total: {r['avg_dist_total']}\nstandardized distances\nnormal_avg_20fs={r['normal_avg_20fs']} -- normal_std_20fs="
                 f"{r['normal_std_20fs']}\nnormal_avg_10fs={r['normal_avg_10fs']} -- normal_std_10fs={r['normal_std_10fs']}\n\n\n")
    assert repdist.parse_report(text) == vals
    assert [ln for ln in text.splitlines() if ln and not any(c.isdigit() for c in ln)] == [str(h) for h in fx["reference/headings"]]


def test_refusals_that_need_no_device():
    x = torch.zeros(8, 4)
    for call in (lambda: repdist.pairwise_distance_stats(x), lambda: repdist.lag_distances(x),
                 lambda: repdist.representation_similarity(x), lambda: repdist.representation_report(x),
                 lambda: metrics.energy_distance(x, x), lambda: repdist.pairwise_distance_stats(np.zeros((8, 4), np.float32))):
        with pytest.raises(TypeError):
            call()
    with pytest.raises(ValueError, match="range"):
        repdist.histogram_edges(16)
    for bad in ([3.0, 2.0, 1.0], [0.0, 1.0, 1.0], [1.0], [[0.0, 1.0]], [0.0, float("nan")]):
        with pytest.raises(ValueError):
            repdist.histogram_edges(bad)
    for bins, rng in ((0, (0.0, 1.0)), (4, (1.0, 1.0)), (4, (0.0, float("inf"))), ([0.0, 1.0], (0.0, 1.0))):
        with pytest.raises(ValueError):
            repdist.histogram_edges(bins, rng)
    assert np.array_equal(repdist.histogram_edges(7, (0.5, 4.0)), np.linspace(0.5, 4.0, 8))
    with pytest.raises(ValueError, match="n_random"):
        repdist.similarity_rows(1003, "random", 1000, 0)
    assert len(repdist.similarity_rows(1004, "random", 1000, 0)) == 1000
    for kw in (dict(method="some"), dict(margin=1), dict(method="random", n_random=0)):
        with pytest.raises(ValueError):
            repdist.similarity_rows(100, **{"method": "all", **kw})
    with pytest.raises(ValueError):
        repdist.similarity_rows(4, "all")
