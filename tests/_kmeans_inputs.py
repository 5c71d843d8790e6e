"""Seeded inputs of the k-means tests (tests/test_kmeans_host.py, tests/test_gpu_kmeans.py) and of tests/golden/make_fixtures_kmeans.py.
Everything is regenerated from the seeds; the fixture keeps sha256 digests of what these functions return."""
import hashlib

import numpy as np

# (N, E, K, seed): the fits recorded in tests/golden/kmeans.npz
CASES = {"shipped": (4133, 400, 300, 1), "small": (1500, 48, 16, 1), "mid": (2053, 400, 48, 3)}
# (N, E, K, data seed, RandomState seed) of the recorded k-means++ seeding
PP_CASE = (3000, 48, 24, 5, 2)          # (RandomState seeds 0 and 1 put a search target within 1e-6 of a cumulative sum)


def make(N, E, K, seed):
    """-> X (N,E) fp32 in (-1, 1): tanh of a mixture of max(K // 3, 4) Gaussians, and init (K,E): K distinct rows of X."""
    rng = np.random.default_rng(seed)
    cen = rng.normal(size=(max(K // 3, 4), E)) * 0.3
    X = np.tanh(cen[rng.integers(0, len(cen), N)] + 0.4 * rng.normal(size=(N, E))).astype(np.float32)
    init = X[rng.choice(N, K, replace=False)]
    return X, init


def fresh_rows(N, E, K, seed, rows=1000):
    """`rows` further rows of the same mixture (for predict): the generator of `make`, continued."""
    rng = np.random.default_rng(seed)
    cen = rng.normal(size=(max(K // 3, 4), E)) * 0.3
    rng.integers(0, len(cen), N)
    rng.normal(size=(N, E))
    rng.choice(N, K, replace=False)
    return np.tanh(cen[rng.integers(0, len(cen), rows)] + 0.4 * rng.normal(size=(rows, E))).astype(np.float32)


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def check_centers(fx, name, centers, bound):
    """against the recorded centres: whole for the small case, otherwise every `stride`-th element and the Frobenius norm"""
    c = np.asarray(centers, np.float64)
    rec = fx[f"{name}_centers"].astype(np.float64)
    got = c if rec.ndim == 2 else c.reshape(-1)[::int(fx["stride"])]
    assert got.shape == rec.shape
    err = float(np.abs(got - rec).max())
    nerr = abs(float(np.sqrt((c * c).sum())) - float(fx[f"{name}_centers_norm"]))
    print(f"{name}: centres within {err:.2e} of sklearn's (bound {bound:.2e}), norm differs by {nerr:.2e}")
    assert err <= bound
    assert nerr <= bound * np.sqrt(c.size)
