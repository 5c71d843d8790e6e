"""CPU-only: the float64 restatement of Ward's rounds (tests/_ward_ref.py) against sklearn's recorded tree and labels
(tests/golden/ward.npz) with the conditions the fixture must meet, the host bookkeeping of gesture2vec_amd/agglomerative.py (the sort
and relabelling of a merge log, the cut), the declarations the feature adds, the constructor's and fit's refusals and the options of
scripts/cluster_latents.py."""
import functools
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import _ward_inputs as WI
import _ward_ref as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("g2v_ward_max_rows", "g2v_ward_workspace", "g2v_ward_distances", "g2v_ward_rounds")


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "ward.npz"))


@functools.lru_cache(maxsize=None)
def _rounds(name, golden_dir):
    return WR.rounds(np.load(os.path.join(golden_dir, "ward.npz"))[f"{name}_x"])


@pytest.mark.parametrize("name", WI.FIXTURES)
def test_restatement_equals_the_recorded_sklearn_tree(fx, golden_dir, name):
    X, children, dist = fx[f"{name}_x"], fx[f"{name}_children"].astype(np.int64), fx[f"{name}_distances"]
    N = len(X)
    assert X.dtype == np.float32 and children.shape == (N - 1, 2) and dist.shape == (N - 1,) and dist.dtype == np.float64
    r = _rounds(name, golden_dir)
    got_children, got_dist = WR.tree(r["pairs"], r["heights"], N)
    gap_h, gap_sk = WR.height_gap(got_dist), WR.height_gap(dist)
    err = float(np.max(np.abs(got_dist - dist) / dist))
    print(f"{name}: {X.shape}, {r['rounds']} rounds, nn gap {r['nn_gap']:.2e}, height gap {gap_h:.2e} (sklearn's {gap_sk:.2e}), "
          f"heights off by {err:.1e}")
    assert r["nn_gap"] > WI.REL_GAP and gap_h > WI.REL_GAP and gap_sk > WI.REL_GAP
    assert np.array_equal(got_children, children)
    assert err < 1e-12                                            # two float64 evaluations of the same tree
    assert np.array_equal(r["sizes"][np.argsort(r["heights"], kind="stable")][-1:], [N])
    if name == "chain":
        assert r["rounds"] > 8                                    # check_every = 4 is outrun several times


@pytest.mark.parametrize("name", WI.FIXTURES)
def test_cuts_equal_the_recorded_sklearn_labels(fx, name):
    """the restated cut and the package's (agglomerative.hc_cut) against sklearn's labels_ at three n_clusters each"""
    from gesture2vec_amd.agglomerative import hc_cut
    children, N = fx[f"{name}_children"].astype(np.int64), len(fx[f"{name}_x"])
    assert tuple(fx[f"{name}_ks"]) == WI.KS[name]
    for k, labels in zip(fx[f"{name}_ks"], fx[f"{name}_labels"].astype(np.int64)):
        assert len(np.unique(labels)) == k
        assert np.array_equal(WR.cut(int(k), children, N), labels)
        assert np.array_equal(hc_cut(int(k), children, N), labels)
    if name == WI.THRESHOLD_ON:
        t, k = float(fx["threshold_t"]), int(fx["threshold_n_clusters"])
        assert int(np.count_nonzero(fx[f"{name}_distances"] >= t)) + 1 == k
        assert np.array_equal(hc_cut(k, children, N), fx["threshold_labels"].astype(np.int64))
    assert np.array_equal(hc_cut(1, children, N), np.zeros(N, dtype=np.int64))
    assert sorted(hc_cut(N, children, N)) == list(range(N))
    with pytest.raises(ValueError, match="more clusters than samples"):
        hc_cut(N + 1, children, N)


@pytest.mark.parametrize("name", WI.FIXTURES)
def test_tree_from_a_merge_log(fx, golden_dir, name):
    """the package's sort and relabelling of a log in round order (slots, heights) gives sklearn's children_"""
    from gesture2vec_amd.agglomerative import tree_from_log
    r = _rounds(name, golden_dir)
    N = len(fx[f"{name}_x"])
    children, dist = tree_from_log(r["pairs"].astype(np.int32), r["heights"], N)
    assert children.dtype == np.int64 and np.array_equal(children, fx[f"{name}_children"])
    assert np.all(np.diff(dist) >= 0) and np.array_equal(dist, np.sort(r["heights"]))
    assert not np.all(np.diff(r["heights"]) >= 0)                 # the log itself is not in height order: the sort is needed


def test_tree_from_a_log_with_ties_keeps_the_log_order():
    from gesture2vec_amd.agglomerative import tree_from_log
    pairs = np.array([(0, 1), (2, 3), (0, 2)])                    # two merges at one height, then their union at the same height
    children, dist = tree_from_log(pairs, np.array([1.0, 1.0, 1.0]), 4)
    assert children.tolist() == [[0, 1], [2, 3], [4, 5]] and dist.tolist() == [1.0, 1.0, 1.0]


def test_header_and_makefile_name_the_feature():
    from gesture2vec_amd import _lib
    for name in ENTRIES:
        assert name in _lib.EXPORTS, name
    mk = open(os.path.join(ROOT, "gesture2vec_amd", "csrc", "Makefile")).read()
    assert "ward.hip" in re.search(r"^SRCS\s*=(.*)$", mk, re.M)[1].split()
    C = _lib.C
    assert _lib._SIGS["g2v_ward_distances"] == (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                                           C.c_void_p])
    assert _lib._SIGS["g2v_ward_rounds"] == (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])


def test_row_limit_and_workspace():
    """the limit and the workspace are host functions of the library: no device is needed to ask them"""
    from gesture2vec_amd import ops
    from gesture2vec_amd.agglomerative import check_rows
    limit = ops.ward_max_rows()
    assert limit == 32768
    assert ops.ward_workspace(limit, 400) >= 8 * limit and ops.ward_workspace(limit + 1, 400) == 0
    assert ops.ward_workspace(0, 400) == 0 and ops.ward_workspace(64, 513) == 0 and ops.ward_workspace(64, 0) == 0
    assert ops.ward_workspace(2, 1) > 0 and ops.ward_workspace(64, 512) > 0
    check_rows(limit)
    with pytest.raises(ValueError, match=str(limit)):
        check_rows(limit + 1)


def test_constructor():
    from gesture2vec_amd.agglomerative import AgglomerativeClustering as AC
    ac = AC()
    assert (ac.n_clusters, ac.metric, ac.linkage, ac.distance_threshold, ac.compute_distances, ac.check_every) == \
        (2, "euclidean", "ward", None, False, 4)
    ac = AC(7, compute_distances=True, connectivity=None, memory=None, compute_full_tree="auto")
    assert ac.n_clusters == 7 and ac.compute_distances and ac.labels_ is None and ac.children_ is None and ac.n_clusters_ is None
    assert AC(n_clusters=None, distance_threshold=1.5, compute_full_tree=True).distance_threshold == 1.5
    with pytest.raises(TypeError):
        AC(3, "euclidean")                                        # keyword-only behind n_clusters, as sklearn's
    for name in ("connectivity", "memory"):
        with pytest.raises(TypeError, match=f"`{name}`"):
            AC(**{name: object()})
    with pytest.raises(TypeError, match="`compute_full_tree`"):
        AC(compute_full_tree=False)
    with pytest.raises(TypeError, match="`affinity`"):
        AC(affinity="euclidean")
    for linkage in ("complete", "average", "single"):
        with pytest.raises(ValueError, match="linkage"):
            AC(linkage=linkage)
    for metric in ("manhattan", "cosine", "precomputed"):
        with pytest.raises(ValueError, match="metric"):
            AC(metric=metric)
    with pytest.raises(ValueError, match="exactly one of n_clusters and distance_threshold"):
        AC(n_clusters=3, distance_threshold=1.0)
    with pytest.raises(ValueError, match="exactly one of n_clusters and distance_threshold"):
        AC(n_clusters=None)
    for k in (0, -2, 2.5):
        with pytest.raises(ValueError, match="n_clusters"):
            AC(n_clusters=k)
    for t in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="distance_threshold"):
            AC(n_clusters=None, distance_threshold=t)
    with pytest.raises(ValueError, match="check_every"):
        AC(check_every=0)
    with pytest.raises(RuntimeError, match="fit first"):
        AC().cut(3)
    again = pickle.loads(pickle.dumps(AC(5, compute_distances=True)))
    assert (again.n_clusters, again.compute_distances, again.labels_) == (5, True, None)


def test_api_refuses_cpu_tensors():
    from gesture2vec_amd.agglomerative import AgglomerativeClustering as AC
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        AC().fit(torch.zeros(8, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        AC().fit_predict(torch.zeros(8, 4))


def test_cluster_latents_help_names_ward():
    run = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "cluster_latents.py"), "--help"], capture_output=True,
                         text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    for opt in ("--checkpoint", "--chunks", "--n_clusters", "--scan-k", "--out", "--algorithm", "{kmeans,dbscan,ward}",
                "--distance-threshold", "--eps", "--min-samples"):
        assert opt in run.stdout, opt
