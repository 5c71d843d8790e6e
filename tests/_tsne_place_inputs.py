"""Seeded inputs of the placement tests (tests/test_tsne_place_host.py, tests/test_gpu_tsne_place.py).  The rows are centred like PCA
scores: Gaussian clusters of unit noise whose centres differ by about 2.5 noise widths per axis, the mean of the fitted rows taken
out, so that |x|^2 stays small next to the gaps between neighbouring distances (the Gram form of the distances carries an error
proportional to |z|^2 + |x|^2).  Everything is regenerated from the seeds."""
import functools

import numpy as np

import _tsne_place_ref as PR

TAU = 4e-6                              # the allowed distance difference is TAU (|z_i|^2 + max_j |x_j|^2): ten times the 3e-7
                                        # rounding include/g2v.h documents for the Gram distances
MAIN = (1037, 48, 131)                  # N, d, M of the case the conditionals, gradient and trajectory tests share
PERPLEXITY, K = 5.0, 25
K_AFF = 15                              # min(N - 1, floor(3 * perplexity))
NEIGHBOUR_CASES = {                     # name -> (N, d, M, kk)
    "n1037": (1037, 48, 131, 25),
    "ld52": (1037, 50, 131, 25),        # on a pitch of 52 floats, junk in the spare columns
    "n26": (26, 8, 5, 25),
    "kk128": (300, 16, 70, 128),
    "n20011": (20011, 8, 67, 25),
}


def clusters(n_clusters, per_ref, per_new, d, seed):
    """-> X (n_clusters * per_ref, d) fp32, its labels, Z (n_clusters * per_new, d) fp32, its labels; both in a seeded row order"""
    rng = np.random.default_rng(seed)
    centres = (2.5 / np.sqrt(2.0)) * rng.normal(size=(n_clusters, d))
    lx, lz = np.repeat(np.arange(n_clusters), per_ref), np.repeat(np.arange(n_clusters), per_new)
    X = centres[lx] + rng.normal(size=(len(lx), d))
    Z = centres[lz] + rng.normal(size=(len(lz), d))
    ox, oz = rng.permutation(len(lx)), rng.permutation(len(lz))
    mean = X.mean(0)
    return (np.ascontiguousarray(X[ox] - mean, dtype=np.float32), lx[ox].astype(np.int64),
            np.ascontiguousarray(Z[oz] - mean, dtype=np.float32), lz[oz].astype(np.int64))


@functools.lru_cache(maxsize=None)
def rows(N, d, M, seed=0):
    """X (N, d), labels, Z (M, d), labels (8 clusters), read-only, with the planted cases of the neighbour test where they fit:
    Z[1] = X[3] bit for bit, and X[5] = X[4] bit for bit with Z[2] close to both"""
    X, lx, Z, lz = clusters(8, -(-N // 8), -(-M // 8), d, 7000 * d + N + M + seed)
    X, lx, Z, lz = np.array(X[:N]), lx[:N], np.array(Z[:M]), lz[:M]
    if N >= 6 and M >= 3:
        Z[1] = X[3]
        X[5] = X[4]
        Z[2] = X[4] + np.float32(0.01)
    for a in (X, lx, Z, lz):
        a.setflags(write=False)
    return X, lx, Z, lz


def fake_map(labels, seed=0, spread=3.0, apart=25.0):
    """an (N, 2) fp32 layout with the look of a fitted map: one blob of width `spread` per label, blob centres `apart` apart"""
    rng = np.random.default_rng(seed)
    n = int(labels.max()) + 1
    ang = 2.0 * np.pi * np.arange(n) / n
    centres = apart * np.stack([np.cos(ang), np.sin(ang)], 1)
    return (centres[labels] + spread * rng.normal(size=(len(labels), 2))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def main_case():
    """the shared case, with the restatement's own neighbours, conditionals and median start: dict(X, Y, Z, lx, lz, D, idx, d2, p, y0)"""
    N, d, M = MAIN
    X, lx, Z, lz = rows(N, d, M)
    Y = fake_map(lx, 1)
    D = PR.sqdist(Z, X)
    idx, d2 = PR.neighbors(D, max(K_AFF, K))
    p = PR.conditionals(d2[:, :K_AFF], PERPLEXITY).astype(np.float32)
    out = dict(X=X, Y=Y, Z=Z, lx=lx, lz=lz, D=D, idx=idx, d2=d2, p=p, y0=PR.start(Y, idx, p, "median", K))
    for a in out.values():
        a.setflags(write=False)
    return out


def tau(X, Z):
    """the per-row distance tolerance of the neighbour test"""
    X, Z = np.asarray(X, np.float64), np.asarray(Z, np.float64)
    return TAU * ((Z * Z).sum(1) + (X * X).sum(1).max())


def close_calls(D, X, Z, ranks):
    """share of the rows whose float64 distances of rank r and r + 1 (1-based) lie closer than tau_i for some r in `ranks`: there a
    neighbour list formed from fp32 Gram distances may legitimately differ from the float64 one"""
    S = np.sort(D, axis=1)
    t = tau(X, Z)
    bad = np.zeros(len(D), bool)
    for r in ranks:
        if r < S.shape[1]:
            bad |= (S[:, r] - S[:, r - 1]) < t
    return float(bad.mean())
