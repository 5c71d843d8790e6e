"""The float64 restatement of gesture2vec_amd/repdist.py in numpy (no scipy): every distance is the square root of a float64 sum of
squared DIFFERENCES of the fp32 rows widened to float64, never a Gram form, so it carries E ulps of one chain and nothing else.

    pair_d2                    d^2 over the pairs i < j of X (pdist's order) or over all pairs of X and Y (row-major)
    stats                      what pairwise_distance_stats returns, with np.std for the standard deviation
    histogram                  numpy.histogram's bin rule, written out
    edge_gap                   the precondition of equal histograms: how close, relatively, any distance comes to any edge
    lag_distances              the neighbour distances with their NaN rules
    representation_similarity  the reference's nine numbers for one method, in float64

Bars (derived in the issue of this feature from pair_dist.hpp's statement |delta d^2| <= 8 E 2^-53 d^2 for a pair that is not near):
BAR_SUM(E) = 8 E 2^-53 for sum, mean, min, max; BAR_SQ(E) = 16 E 2^-53 for sum_sq; BAR_STD = BAR_SQ mean^2 / var; 4 E 2^-53 per lag
distance.  EDGE_GAP = 1e-9: four orders above the per-pair bound."""
import random

import numpy as np

EDGE_GAP = 1e-9
KEYS = ("avg_20fs", "std_20fs", "avg_10fs", "std_10fs", "avg_dist_total", "normal_avg_20fs", "normal_std_20fs", "normal_avg_10fs",
        "normal_std_10fs")
NEIGHBOUR_KEYS = tuple(k for k in KEYS if k != "avg_dist_total")


def bar_sum(E):
    return 8 * E * 2.0 ** -53


def bar_sq(E):
    return 16 * E * 2.0 ** -53


def bar_std(E, mean, var):
    return bar_sq(E) * mean * mean / var


def bar_lag(E):
    return 4 * E * 2.0 ** -53


def pair_d2(X, Y=None):
    X64 = np.asarray(X, dtype=np.float64)
    if Y is None:
        out = [((X64[i + 1:] - X64[i]) ** 2).sum(axis=1) for i in range(X64.shape[0] - 1)]
        return np.concatenate(out) if out else np.zeros(0)
    Y64 = np.asarray(Y, dtype=np.float64)
    return np.concatenate([((Y64 - X64[i]) ** 2).sum(axis=1) for i in range(X64.shape[0])])


def stats(X, Y=None):
    d2 = pair_d2(X, Y)
    with np.errstate(invalid="ignore"):
        d = np.sqrt(d2)
    n = int(d.size)
    res = {"count": n, "nonfinite": int((~np.isfinite(d)).sum()), "d": d}
    if n == 0:
        res.update(sum=0.0, sum_sq=0.0, min=float("inf"), max=float("-inf"), mean=float("nan"), std=float("nan"))
        return res
    ok = d[~np.isnan(d)]
    res.update(sum=float(d.sum()), sum_sq=float(d2.sum()), min=float(ok.min()) if ok.size else float("inf"),
               max=float(ok.max()) if ok.size else float("-inf"), mean=float(d.mean()), std=float(d.std()))
    return res


def histogram(d, edges):
    """numpy.histogram's rule: bin b holds edges[b] <= d < edges[b + 1], the last bin also d == edges[-1]; anything else, NaN
    included, is in no bin"""
    edges = np.asarray(edges, dtype=np.float64)
    bins = edges.size - 1
    d = np.asarray(d, dtype=np.float64)
    d = d[~np.isnan(d)]
    b = np.searchsorted(edges, d, side="right") - 1
    b[d == edges[-1]] = bins - 1
    keep = (d >= edges[0]) & (d <= edges[-1])
    return np.bincount(b[keep], minlength=bins).astype(np.int64)


def edge_gap(d, edges, skip_equal=False):
    """min over (distance, edge) of |d - e| / max(d, |e|); with skip_equal a distance that IS an edge does not count (only where
    both sides are known to be exact)"""
    d = np.asarray(d, dtype=np.float64)
    d = d[np.isfinite(d)]
    gap = np.inf
    for e in np.asarray(edges, dtype=np.float64):
        diff = np.abs(d - e)
        scale = np.maximum(d, abs(e))
        use = scale > 0
        if skip_equal:
            use &= diff > 0
        if use.any():
            gap = min(gap, float((diff[use] / scale[use]).min()))
    return gap                                                   # (a distance 0 on an edge 0 is 0 on every side: bitwise equal rows)


def lag_distances(X, lags=(1, 2), clip_ids=None):
    X64 = np.asarray(X, dtype=np.float64)
    N = X64.shape[0]
    out = np.full((len(lags), N), np.nan)
    for l, lag in enumerate(lags):
        for i in range(lag, N - lag):
            if clip_ids is not None and not (clip_ids[i - lag] == clip_ids[i] == clip_ids[i + lag]):
                continue
            out[l, i] = (np.sqrt(((X64[i - lag] - X64[i]) ** 2).sum()) + np.sqrt(((X64[i + lag] - X64[i]) ** 2).sum())) / 2
    return out


def similarity_rows(N, method, n_random=1000, seed=None, margin=2):
    rows = range(margin, N - margin)
    return list(rows) if method == "all" else random.Random(seed).sample(rows, n_random)


def representation_similarity(X, method="all", n_random=1000, seed=None, margin=2, clip_ids=None, avg_total=None, lagd=None):
    if avg_total is None:
        avg_total = stats(X)["mean"]
    if lagd is None:
        lagd = lag_distances(X, (1, 2), clip_ids)
    rows = np.asarray(similarity_rows(X.shape[0], method, n_random, seed, margin), dtype=np.int64)
    res = {"avg_dist_total": float(avg_total)}
    for l, tag in ((0, "20fs"), (1, "10fs")):
        v = lagd[l, rows]
        if clip_ids is not None:
            v = v[~np.isnan(v)]
        res[f"avg_{tag}"], res[f"std_{tag}"] = float(np.mean(v)), float(np.std(v))
        res[f"normal_avg_{tag}"], res[f"normal_std_{tag}"] = float(np.mean(v / avg_total)), float(np.std(v / avg_total))
    return res
