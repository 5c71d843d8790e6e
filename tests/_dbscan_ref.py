"""DBSCAN in float64 numpy, stated as a rule instead of sklearn's sequential `dbscan_inner` (the checker of
gesture2vec_amd/dbscan.py; sklearn itself is not imported).  With adj(i, j) <=> |x_i - x_j| <= eps (a row is its own neighbour):

    core(i)  <=>  #{j : adj(i, j)} >= min_samples
    root(i), for core i = the smallest index in i's connected component of the graph of core rows under adj
    the cluster id of a component = the rank of its root among all roots in ascending order
    a non-core row with a core neighbour gets the smallest cluster id among its core neighbours, any other non-core row -1

sklearn opens clusters in index order and finishes one before the next, and the first cluster to reach a border row keeps it: the
labels are equal, not merely equivalent.  Distances are sum (x_i - x_j)^2 in float64 from the fp32 rows."""
import numpy as np


def sq_distances(X):
    """(N, N) float64: sum_k (x_ik - x_jk)^2 from differences (no Gram form), symmetric, diagonal exactly 0"""
    X = np.asarray(X, dtype=np.float64)
    N = X.shape[0]
    D = np.empty((N, N))
    for a in range(0, N, 64):
        diff = X[a:a + 64, None, :] - X[None, :, :]
        D[a:a + 64] = np.einsum("ijk,ijk->ij", diff, diff)
    return D


def adjacency(X, eps):
    return sq_distances(X) <= float(eps) * float(eps)


def closest_to_eps(X, eps):
    """min over pairs i != j of | |x_i - x_j| / eps - 1 |: how far the input is from a pair that rounding could decide"""
    D = np.sqrt(sq_distances(X))
    off = ~np.eye(D.shape[0], dtype=bool)
    return float(np.abs(D[off] / float(eps) - 1.0).min()) if off.any() else np.inf


def dbscan(adj, min_samples):
    """adj (N, N) bool, symmetric with a true diagonal -> dict(labels int64 (N), core bool (N), counts int64 (N), roots int64 (N)
    (N where a row is not core), rounds = the rounds of min-propagation with pointer jumping until nothing changes, the last
    one included)"""
    adj = np.asarray(adj, dtype=bool)
    N = adj.shape[0]
    counts = adj.sum(1).astype(np.int64)
    core = counts >= int(min_samples)
    L = np.where(core, np.arange(N), N).astype(np.int64)
    to_core = adj & core[None, :]
    rounds = 0
    while True:
        rounds += 1
        nb = np.where(to_core, L[None, :], N).min(1)
        B = np.where(core, np.minimum(L, nb), N)
        A = np.where(B < N, B[np.minimum(B, N - 1)], N)          # pointer jumping
        if np.array_equal(A, L):
            break
        L = A
    rank = np.cumsum(L == np.arange(N)) - (L == np.arange(N))   # exclusive
    m = np.where(core, L, np.where(to_core, L[None, :], N).min(1))
    labels = np.where(m < N, rank[np.minimum(m, N - 1)], -1).astype(np.int64)
    return {"labels": labels, "core": core, "counts": counts, "roots": L, "rounds": rounds}


def fit(X, eps, min_samples):
    return dbscan(adjacency(X, eps), min_samples)
