"""Seeded inputs of the t-SNE / PCA tests (tests/test_tsne_host.py, tests/test_gpu_tsne.py) and of tests/golden/make_fixtures_tsne.py.
Everything is regenerated from the seeds; the fixture keeps sha256 digests of what these functions return."""
import functools
import hashlib

import numpy as np

BASE = (6, 120, 400, 0)            # clusters, rows per cluster, E, seed: the base case (720 x 400)
PERPLEXITY = 30.0
SMALL_N = 97                       # one ragged tile
N_DUP = 3                          # bitwise-duplicate pairs planted by rows(): row 2 m + 1 = row 2 m


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def clusters(n_clusters, per, E, seed, noise=0.35):
    """-> X (n_clusters * per, E) fp32 in a seeded row order, labels int64: Gaussian clusters, centres N(0, 1), noise N(0, noise^2)"""
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(n_clusters, E))
    lab = np.repeat(np.arange(n_clusters), per)
    X = centres[lab] + noise * rng.normal(size=(n_clusters * per, E))
    order = rng.permutation(len(lab))
    return np.ascontiguousarray(X[order], dtype=np.float32), lab[order].astype(np.int64)


@functools.lru_cache(maxsize=None)
def base():
    X, lab = clusters(*BASE)
    X.setflags(write=False)
    return X, lab


@functools.lru_cache(maxsize=None)
def small():
    """the first SMALL_N rows of the base case"""
    X, lab = base()
    return np.ascontiguousarray(X[:SMALL_N]), lab[:SMALL_N]


@functools.lru_cache(maxsize=None)
def rows(N, d, seed=0):
    """(N, d) fp32 clustered rows (8 clusters) with N_DUP bitwise-duplicate pairs planted at the front"""
    X, _ = clusters(8, -(-N // 8), d, 1000 * d + N + seed)
    X = np.array(X[:N], copy=True)
    for m in range(N_DUP):
        X[2 * m + 1] = X[2 * m]
    X.setflags(write=False)
    return X


def init_y(N, seed=0):
    """the fixed start of the recorded runs: sklearn's init="random" draw"""
    return (1e-4 * np.random.RandomState(seed).standard_normal(size=(N, 2))).astype(np.float32)
