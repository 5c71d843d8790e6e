"""Seeded inputs of the DBSCAN tests (tests/golden/make_fixtures_dbscan.py records the fixture's rows themselves in
tests/golden/dbscan.npz; the GPU shape sweep draws from here).  Every generator returns (X fp32 (N, E), eps, min_samples)."""
import numpy as np

FIXTURES = ("blobs_193x37", "blobs_257x3", "blobs_300x400", "chains", "contested")
REL_GAP = 1e-4        # no pair of a fixture may lie within this of eps, relative: then sklearn's own rounding decides no pair


def blobs(N, E, seed, k=4):
    """k blobs whose spread lives in min(3, E) directions of the E columns (so that pair distances inside a blob are spread out
    instead of concentrated at one value), centres 12 from the origin, and N // 16 (>= 3) rows thrown 6 away from their centre.
    eps = 0.9 with min_samples = 5 leaves core, border and noise rows."""
    rng = np.random.default_rng(seed)
    dl = min(3, E)
    centres = rng.normal(size=(k, E))
    centres *= 12.0 / np.linalg.norm(centres, axis=1, keepdims=True)
    P = np.linalg.qr(rng.normal(size=(E, dl)))[0].T                       # (dl, E), orthonormal rows
    which = rng.integers(0, k, N)
    X = centres[which] + rng.normal(size=(N, dl)) @ P + 0.01 / np.sqrt(E) * rng.normal(size=(N, E))
    out = rng.choice(N, min(N, max(3, N // 16)), replace=False)
    away = rng.normal(size=(len(out), E))
    X[out] = centres[which[out]] + 6.0 * away / np.linalg.norm(away, axis=1, keepdims=True)
    return X.astype(np.float32), 0.9, 5


def chains(seed=0, lengths=(150, 90), spacing=0.8, E=5):
    """two chains of rows `spacing` apart, shuffled: eps = 1.0 and min_samples = 3 make every inner row core with exactly its two
    chain neighbours, so a label has to travel the length of a chain"""
    rng = np.random.default_rng(seed)
    rows = []
    for c, n in enumerate(lengths):
        p = np.zeros((n, E))
        p[:, 0] = spacing * np.arange(n)
        p[:, 1] = 50.0 * c
        rows.append(p)
    X = np.concatenate(rows)
    return X[rng.permutation(len(X))].astype(np.float32), 1.0, 3


def contested(seed=0):
    """two 3 x 3 grids of unit spacing in the planes z = 0 and z = 2.7, and one row between them at z = 1.35.  eps = 1.5,
    min_samples = 9: only the two grid centres are core (their grid, and the row between), the row between is within eps of both
    and core of neither, so it takes the id of the cluster opened first.  -> (X, eps, min_samples, index of the row between)"""
    g = np.array([(a, b, 0.0) for a in (-1.0, 0.0, 1.0) for b in (-1.0, 0.0, 1.0)])
    X = np.concatenate([g, g + np.array([0.0, 0.0, 2.7]), np.array([[0.0, 0.0, 1.35]])])
    perm = np.random.default_rng(seed).permutation(len(X))
    return X[perm].astype(np.float32), 1.5, 9, int(np.nonzero(perm == len(X) - 1)[0][0])
