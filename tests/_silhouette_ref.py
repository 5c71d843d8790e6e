"""float64 numpy restatement of sklearn.metrics.silhouette_samples (Euclidean) for the silhouette tests.  Distances come from the
differences x_i - x_j themselves, never from |x|^2 + |y|^2 - 2 x.y, so near-duplicate rows keep all their digits."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np


def distances(X, rows=None, budget=1 << 22):
    """(len(rows), N) float64 Euclidean distances from the rows `rows` (default: all) to every row.  Blocks of rows are dealt to up to
    16 threads (numpy releases the interpreter lock inside); each element is computed by one thread, so the result does not depend on
    how many there are."""
    X64 = np.asarray(X, np.float64)
    N, E = X64.shape
    rows = np.arange(N) if rows is None else np.asarray(rows)
    D = np.empty((len(rows), N), np.float64)
    block = max(1, min(16, budget // (N * E)))
    cols = max(1, budget // (block * E))                    # columns of D per temporary

    def one(a):
        mine = X64[rows[a:a + block], None, :]
        for c in range(0, N, cols):
            diff = mine - X64[None, c:c + cols, :]
            D[a:a + block, c:c + cols] = np.sqrt(np.einsum("ijk,ijk->ij", diff, diff))

    starts = range(0, len(rows), block)
    workers = min(16, os.cpu_count() or 1, len(starts))
    if workers <= 1:
        for a in starts:
            one(a)
    else:
        with ThreadPoolExecutor(workers) as ex:
            list(ex.map(one, starts))
    return D


def terms(D, labels, rows=None):
    """a, b, s of the rows `rows` (default: all) from their distance rows D (len(rows), N): a = mean distance to the other rows of the
    own cluster, b = lowest mean distance to another non-empty cluster, s = (b - a) / max(a, b); a = s = 0 in a cluster of one row,
    s = 0 where a = b = 0."""
    labels = np.asarray(labels)
    N = labels.shape[0]
    rows = np.arange(N) if rows is None else np.asarray(rows)
    _, inv = np.unique(labels, return_inverse=True)
    cnt = np.bincount(inv).astype(np.float64)
    sums = np.zeros((len(rows), len(cnt)), np.float64)
    for c in range(len(cnt)):
        sums[:, c] = D[:, inv == c].sum(1)
    ar, own = np.arange(len(rows)), inv[rows]
    n_own = cnt[own]
    a = np.where(n_own > 1, sums[ar, own] / np.maximum(n_own - 1.0, 1.0), 0.0)
    mean = sums / cnt[None, :]
    mean[ar, own] = np.inf
    b = mean.min(1)
    m = np.maximum(a, b)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where((m > 0) & (n_own > 1), (b - a) / m, 0.0)
    return a, b, s


def silhouette_samples(X, labels):
    return terms(distances(X), labels)[2]
