"""This project's own float64 numpy restatement of what csrc/map_quality.hip and gesture2vec_amd/embedding.py compute for the
quality of a map: the rank of listed neighbours among all rows (g2v_neighbor_ranks), the per-row penalties, trustworthiness and
continuity as sklearn 1.7 defines them (sklearn.manifold.trustworthiness, Euclidean), the variant for rows placed against a fitted
set, and DBSCAN's k-distance curve.  Distances come from differences, orders from a stable argsort (ties to the lower index).
Nothing here imports sklearn (tests/golden/make_fixtures_mapquality.py checks it against sklearn and records the results).

It also holds the inputs of the tests and the PRECONDITIONS an input has to meet before a device result may be compared with this
file entry for entry; the tests assert them again on the host, so a bad input fails loudly instead of being excused."""
import numpy as np

from _tsne_ref import sqdist

BAND = 64.0 * 2.0 ** -24        # NR_BAND of csrc/map_quality.hip: inside it the kernel decides again in float64
GRAM_ERR = 34.0 * 2.0 ** -24    # the worst case of the Gram form's fp32 d^2, in units of (n_i + n_j) (derived at NR_BAND)
REL_SEP = 1e-12                 # precondition (b)

# (N, d, k, c): two row blocks, the second of 3 rows, d % 4 != 0 and under one chunk | three blocks, chunks of 32 + 8 columns | the
# shipped width | odd everything, c = 3 | the k limit
SHAPES = ((67, 5, 3, 2), (130, 40, 5, 2), (193, 400, 5, 2), (257, 133, 12, 3), (257, 50, 127, 2))
PLACED = (130, 40, 5, 2, 37)    # N, d, k, c, M
EXACT_N, EXACT_D, EXACT_K = 96, 6, 5


def name_of(shape):
    return "g%dx%d_k%d_c%d" % tuple(shape[:4])


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def generic(N, d, c, seed, M=0):
    """-> X (N, d), Y (N, c) fp32: 8 Gaussian clusters and a noisy random projection of them; with M, also M new rows near drawn
    rows of X and their noisy projections (Z (M, d), y (M, c))"""
    g = np.random.default_rng(seed)
    centres = 2.0 * g.standard_normal((8, d))
    X = centres[g.integers(0, 8, N)] + g.standard_normal((N, d))
    P = g.standard_normal((d, c))
    Y = X @ P / np.sqrt(d) + 0.3 * g.standard_normal((N, c))
    X, Y = X.astype(np.float32), Y.astype(np.float32)
    if not M:
        return X, Y
    Z = X[g.integers(0, N, M)].astype(np.float64) + 0.5 * g.standard_normal((M, d))
    y = Z @ P / np.sqrt(d) + 0.3 * g.standard_normal((M, c))
    return X, Y, Z.astype(np.float32), y.astype(np.float32)


def exact_grid(seed=0):
    """-> X (96, 6), Y (96, 2) fp32 of small integers: many exactly equal distances, bitwise duplicate rows in both spaces, and in
    Y eight copies of one row at indices 0 .. 7, so that with k = 5 rows 6 and 7 are not among their own k + 1 nearest"""
    g = np.random.default_rng(seed)
    X = g.integers(0, 3, (EXACT_N, EXACT_D)).astype(np.float32)
    Y = g.integers(0, 5, (EXACT_N, 2)).astype(np.float32)
    Y[:8] = Y[0]
    X[10], X[50], X[51] = X[3], X[3], X[20]
    Y[10], Y[60] = Y[3], Y[33]
    return X, Y


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def cross_sqdist(Z, X):
    """float64 (M, N) squared distances of the rows of Z to the rows of X, from differences"""
    Z, X = np.asarray(Z, np.float64), np.asarray(X, np.float64)
    D = np.empty((Z.shape[0], X.shape[0]))
    for a in range(0, Z.shape[0], 16):
        diff = Z[a:a + 16, None, :] - X[None, :, :]
        D[a:a + 16] = np.einsum("ijk,ijk->ij", diff, diff)
    return D


def nearest(D, k, exclude_diagonal):
    """the k nearest columns of every row of D under (d^2, index): int32 (M, k)"""
    D = np.array(D)
    if exclude_diagonal:
        np.fill_diagonal(D, np.inf)
    return np.argsort(D, axis=1, kind="stable")[:, :k].astype(np.int32)


def ranks_from(D, idx, self_rows=None):
    """g2v_neighbor_ranks on the float64 distances D (M, N): 1 + #{l != self[m] : (D[m, l], l) < (D[m, j], j)}, j = idx[m][s];
    0 where j is outside [0, N) or equal to self[m]"""
    M, N = D.shape
    rank = np.zeros(idx.shape, np.int32)
    for m in range(M):
        order = np.argsort(D[m], kind="stable")
        pos = np.empty(N, np.int64)
        pos[order] = np.arange(N)
        sf = -1 if self_rows is None else int(self_rows[m])
        for s, j in enumerate(idx[m]):
            if 0 <= j < N and j != sf:
                rank[m, s] = 1 + pos[j] - (1 if 0 <= sf < N and pos[sf] < pos[j] else 0)
    return rank


def neighbor_ranks(X, Z, idx, self_rows=None):
    return ranks_from(cross_sqdist(Z, X), idx, self_rows)


def penalties(rank, k):
    return np.clip(rank.astype(np.int64) - k, 0, None).sum(axis=1)


def score(total, rows, N, k):
    """sklearn's closing expression"""
    return 1.0 - float(total) * (2.0 / (rows * k * (2.0 * N - 3.0 * k - 1.0)))


def map_quality(X, Y, k):
    """-> dict(nn_y, nn_x, rank_t, rank_c, penalty_t, penalty_c, trustworthiness, continuity)"""
    N = X.shape[0]
    DX, DY = sqdist(X), sqdist(Y)
    me = np.arange(N)
    nn_y, nn_x = nearest(DY, k, True), nearest(DX, k, True)
    rank_t, rank_c = ranks_from(DX, nn_y, me), ranks_from(DY, nn_x, me)
    pt, pc = penalties(rank_t, k), penalties(rank_c, k)
    return {"nn_y": nn_y, "nn_x": nn_x, "rank_t": rank_t, "rank_c": rank_c, "penalty_t": pt, "penalty_c": pc,
            "trustworthiness": score(pt.sum(), N, N, k), "continuity": score(pc.sum(), N, N, k)}


def placement_quality(X_ref, Y_ref, Z, y, k):
    N, M = X_ref.shape[0], Z.shape[0]
    DX, DY = cross_sqdist(Z, X_ref), cross_sqdist(y, Y_ref)
    nn_y, nn_x = nearest(DY, k, False), nearest(DX, k, False)
    rank_t, rank_c = ranks_from(DX, nn_y), ranks_from(DY, nn_x)
    pt, pc = penalties(rank_t, k), penalties(rank_c, k)
    return {"nn_y": nn_y, "nn_x": nn_x, "rank_t": rank_t, "rank_c": rank_c, "penalty_t": pt, "penalty_c": pc,
            "trustworthiness": score(pt.sum(), M, N, k), "continuity": score(pc.sum(), M, N, k)}


def k_distances(X, k):
    """the distance of every row to its k-th nearest row counting itself, ascending"""
    return np.sort(np.sqrt(np.sort(sqdist(X), axis=1)[:, k - 1]))


def kneighbors_other(X, k):
    """-> (distances (N, k) float64, indices (N, k)): the k nearest OTHER rows under (d^2, index)"""
    D = sqdist(X)
    nn = nearest(D, k, True)
    return np.sqrt(D[np.arange(X.shape[0])[:, None], nn]), nn


# ---- the preconditions -----------------------------------------------------------------------------------------------------------------
def _norms(A):
    return (np.asarray(A, np.float64) ** 2).sum(axis=1)


def selection_margin(ref, k, queries=None):
    """Precondition (a), in the space the neighbours are SELECTED in: per query row the gap between the d^2 of its k-th and its
    (k + 1)-th nearest (other) reference row, over 2 BAND (n_i + max n).  g2v_tsne_place_neighbors selects on the Gram form, and
    documents that inside that margin a row may take another's place.  -> the smallest such ratio; it has to exceed 1."""
    own = queries is None
    D = sqdist(ref) if own else cross_sqdist(queries, ref)
    if own:
        np.fill_diagonal(D, np.inf)
    S = np.sort(D, axis=1)
    nq, nmax = _norms(ref if own else queries), _norms(ref).max()
    return float(((S[:, k] - S[:, k - 1]) / (2.0 * BAND * (nq + nmax))).min())


def closest_compared(D, idx, self_rows=None):
    """Precondition (b), in the space the ranks are COUNTED in: the smallest relative difference between a listed threshold D[m, j]
    and any other distance of that row that is not bitwise equal to it (the order of a float64 sum may move the last bits of
    either).  It has to exceed REL_SEP."""
    best = np.inf
    for m in range(D.shape[0]):
        row = np.array(D[m])
        if self_rows is not None and 0 <= self_rows[m] < len(row):
            row[self_rows[m]] = np.inf
        for j in idx[m]:
            if 0 <= j < len(row) and np.isfinite(row[j]):
                diff = np.abs(row - row[j])
                diff = diff[(diff > 0) & np.isfinite(diff)]
                if len(diff):
                    best = min(best, float(diff.min() / max(row[j], np.finfo(np.float64).tiny)))
    return best


def band_pairs(X, Z, idx, self_rows=None):
    """-> (sure, may): the pairs (m, l), l != self[m], whose float64 d^2 lies so close to a threshold D[m, j], j = idx[m][s] != l,
    that the kernel MUST decide them again (within (BAND - GRAM_ERR) (n_m + n_l): its fp32 value is inside the band whatever its
    error) and those it MAY (within BAND + GRAM_ERR).  g2v_neighbor_ranks reports a count between the two."""
    D = cross_sqdist(Z, X)
    nsum = _norms(Z)[:, None] + _norms(X)[None, :]
    M, N = D.shape
    sure, may = np.zeros((M, N), bool), np.zeros((M, N), bool)
    cols = np.arange(N)
    for m in range(M):
        sf = -1 if self_rows is None else int(self_rows[m])
        for j in idx[m]:
            if 0 <= j < N and j != sf:
                gap = np.abs(D[m] - D[m, j])
                other = (cols != j) & (cols != sf)
                sure[m] |= other & (gap <= (BAND - GRAM_ERR) * nsum[m])
                may[m] |= other & (gap <= (BAND + GRAM_ERR) * nsum[m])
    return int(sure.sum()), int(may.sum())


def exact_in_fp32(A):
    """the exact family's stand-in for (a): small integers, so that norms, Gram products and d^2 are exact in fp32 and the
    selection itself is exact"""
    A = np.asarray(A, np.float64)
    return bool((A == np.round(A)).all() and 4.0 * A.shape[1] * float(np.abs(A).max()) ** 2 < 2.0 ** 24)
