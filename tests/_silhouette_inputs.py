"""Seeded inputs of the silhouette tests (tests/test_silhouette_host.py, tests/test_gpu_silhouette.py) and of
tests/golden/make_fixtures_silhouette.py, built on tests/_kmeans_inputs.py.  Everything is regenerated from the seeds; the fixture keeps
sha256 digests of what these functions return."""
import functools

import numpy as np

import _kmeans_inputs as KI

CASES = KI.CASES
N_PAIRS = 28                                          # near-duplicate pairs: row 11 + 2m = row 10 + 2m + rel * N(0, 1)
RELS = (0.0, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1)      # rel cycles through these; 0: a bitwise copy
SAMPLE = ("small", 3, 400)                            # (case, RandomState seed, sample_size) of the recorded sampled score


def plant_pairs(X, seed):
    """X with the near-duplicate pairs planted (as many of the 28 as the rows allow): the Gram form |x|^2 + |y|^2 - 2 x.y of such a
    pair's distance has lost most of its bits."""
    rng = np.random.default_rng(seed + 7700)
    X = np.array(X, dtype=np.float32, copy=True)
    for m in range(N_PAIRS):
        noise = rng.normal(size=X.shape[1])
        if 11 + 2 * m < X.shape[0]:
            X[11 + 2 * m] = (X[10 + 2 * m].astype(np.float64) + RELS[m % len(RELS)] * noise).astype(np.float32)
    return X


def nearest_labels(X, init):
    """labels of the nearest init row (float64, lowest index on ties)"""
    X64, C = X.astype(np.float64), init.astype(np.float64)
    d = (X64 * X64).sum(1)[:, None] - 2.0 * X64 @ C.T + (C * C).sum(1)[None, :]
    return d.argmin(1).astype(np.int64)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> X (N,E) fp32 with planted pairs, dict of label sets, n_clusters.  `nearest`: nearest-init labels with cluster 1 merged into
    cluster 0 (id 1 stays unused) and row 5 alone in a cluster of its own, id K; `skewed`: one cluster holds 90 % of the rows."""
    N, E, K, seed = CASES[name]
    X0, init = KI.make(N, E, K, seed)
    X = plant_pairs(X0, seed)
    lab = nearest_labels(X0, init)
    lab[lab == 1] = 0
    lab[5] = K
    rng = np.random.default_rng(seed + 9900)
    skewed = np.where(rng.random(N) < 0.9, K // 2, rng.integers(0, K, N)).astype(np.int64)
    X.setflags(write=False)
    return X, {"nearest": lab, "skewed": skewed}, K + 1
