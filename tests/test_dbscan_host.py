"""CPU-only: the float64 rule of DBSCAN (tests/_dbscan_ref.py) against sklearn's recorded labels and core indices
(tests/golden/dbscan.npz) with the conditions the fixture must meet, the declarations the feature adds, the constructor's refusals and
the options of scripts/cluster_latents.py."""
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import _dbscan_inputs as DI
import _dbscan_ref as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("g2v_dbscan_max_rows", "g2v_dbscan_workspace", "g2v_dbscan_neighbors", "g2v_dbscan_propagate", "g2v_dbscan_labels")


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "dbscan.npz"))


@pytest.mark.parametrize("name", DI.FIXTURES)
def test_rule_equals_the_recorded_sklearn_labels(fx, name):
    X, eps, ms = fx[f"{name}_x"], float(fx[f"{name}_eps"]), int(fx[f"{name}_min_samples"])
    labels, core = fx[f"{name}_labels"].astype(np.int64), fx[f"{name}_core"].astype(np.int64)
    assert X.dtype == np.float32 and labels.shape == (X.shape[0],)
    gap = DR.closest_to_eps(X, eps)
    print(f"{name}: {X.shape}, closest pair to eps {gap:.2e} (relative)")
    assert gap > DI.REL_GAP                                       # sklearn's own rounding decides no pair
    ref = DR.fit(X, eps, ms)
    assert np.array_equal(ref["labels"], labels)
    assert np.array_equal(np.nonzero(ref["core"])[0], core)
    if name.startswith("blobs"):
        assert labels.max() >= 1 and (labels < 0).any()           # at least two clusters, at least one noise row
    if name == "chains":
        assert ref["rounds"] > 1
    if name == "contested":
        between = int(fx["contested_between"])
        near = DR.adjacency(X, eps)[between] & ref["core"]
        assert not ref["core"][between] and len(set(labels[near])) == 2 and labels[between] == labels[near].min()


def test_contested_row_takes_the_lower_id_under_permutations(fx):
    X, eps, ms = fx["contested_x"], float(fx["contested_eps"]), int(fx["contested_min_samples"])
    between = int(fx["contested_between"])
    seen = set()
    for seed in range(6):
        perm = np.random.default_rng(seed).permutation(len(X))
        ref = DR.fit(X[perm], eps, ms)
        at = int(np.nonzero(perm == between)[0][0])
        cores = np.nonzero(ref["core"])[0]
        assert len(cores) == 2 and ref["labels"][at] == 0 and list(ref["labels"][cores]) == [0, 1]
        seen.add(bool(perm[cores[0]] < perm[cores[1]]))
    assert seen == {True, False}                                  # either grid came first at least once


def test_edge_rules_of_the_rule():
    X = DI.blobs(64, 8, 1)[0]
    every = DR.fit(X, 0.9, 1)
    assert every["core"].all() and (every["labels"] >= 0).all()
    none = DR.fit(X, 0.9, 65)
    assert not none["core"].any() and (none["labels"] == -1).all()
    dup = np.repeat(X[:4], 3, axis=0)                             # bitwise duplicates: d = 0 <= any eps
    tiny = DR.fit(dup, 1e-30, 3)
    assert tiny["core"].all() and list(tiny["labels"]) == [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3]


def test_header_and_makefile_name_the_feature():
    from gesture2vec_amd import _lib
    for name in ENTRIES:
        assert name in _lib.EXPORTS, name
    mk = open(os.path.join(ROOT, "gesture2vec_amd", "csrc", "Makefile")).read()
    assert "dbscan.hip" in re.search(r"^SRCS\s*=(.*)$", mk, re.M)[1].split()
    C = _lib.C
    assert _lib._SIGS["g2v_dbscan_neighbors"] == (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_double, C.c_void_p,
                                                             C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p])


def test_constructor():
    from gesture2vec_amd.dbscan import DBSCAN
    db = DBSCAN()
    assert (db.eps, db.min_samples, db.metric) == (0.5, 5, "euclidean")
    db = DBSCAN(1.25, 7)
    assert (db.eps, db.min_samples) == (1.25, 7) and db.labels_ is None and db.n_clusters_ is None
    for name in ("sample_weight", "algorithm", "leaf_size", "p", "n_jobs"):
        with pytest.raises(TypeError, match=f"`{name}`"):
            DBSCAN(**{name: None})
    with pytest.raises(ValueError, match="metric"):
        DBSCAN(metric="manhattan")
    for eps in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="eps"):
            DBSCAN(eps=eps)
    for ms in (0, -3, 2.5):
        with pytest.raises(ValueError, match="min_samples"):
            DBSCAN(min_samples=ms)
    again = pickle.loads(pickle.dumps(DBSCAN(0.7, 3)))
    assert (again.eps, again.min_samples, again._dev) == (0.7, 3, {})


def test_api_refuses_cpu_tensors():
    from gesture2vec_amd.dbscan import DBSCAN
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DBSCAN().fit(torch.zeros(8, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DBSCAN().fit_predict(torch.zeros(8, 4))


def test_cluster_latents_help_keeps_the_old_options():
    run = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "cluster_latents.py"), "--help"], capture_output=True,
                         text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    for opt in ("--checkpoint", "--chunks", "--n_clusters", "--max_iter", "--n_init", "--seed", "--check_every", "--scan-k",
                "--silhouette-rows", "--no-silhouette", "--out", "--batch_rows", "--device"):
        assert opt in run.stdout, opt
    for opt in ("--algorithm", "{kmeans,dbscan}", "--eps", "--min-samples"):
        assert opt in run.stdout, opt
