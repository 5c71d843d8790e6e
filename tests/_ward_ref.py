"""A float64 numpy restatement of Ward clustering by rounds of mutual nearest neighbours (csrc/ward.hip, gesture2vec_amd/
agglomerative.py): the distances from differences, the rounds with scipy's Ward update on unsquared distances, scipy's relabelling of
the merges and sklearn's cut.  It shares no code with the package.  Every round scans every active row afresh (the device keeps a
cache that reducibility allows; equal trees show the cache right), and the pairs of a round are merged one after the other (the
device merges them at once; equal in exact arithmetic, ~1e-16 apart in float64)."""
import heapq

import numpy as np


def distances(X):
    """(N, N) float64 unsquared distances of the rows widened to float64, from differences; +inf on the diagonal"""
    X = np.asarray(X, dtype=np.float64)
    D = np.empty((len(X), len(X)))
    for i in range(len(X)):
        D[i] = np.sqrt(((X - X[i]) ** 2).sum(1))
    np.fill_diagonal(D, np.inf)
    return D


def _ward(dxi, dyi, dxy, nx, ny, ni):
    t = 1.0 / (nx + ny + ni)
    return np.sqrt(np.maximum((ni + nx) * t * dxi * dxi + (ni + ny) * t * dyi * dyi - ni * t * dxy * dxy, 0.0))


def rounds(X):
    """-> dict(pairs (N - 1, 2) slots in round order, heights, sizes, rounds, nn_gap): nn_gap is the smallest relative gap between
    the best and the second-best neighbour of any row in any round (inf where a row has one neighbour left)"""
    D = distances(X)
    N = len(D)
    size = np.ones(N, dtype=np.int64)
    pairs, heights, sizes = [], [], []
    n_rounds, nn_gap = 0, np.inf
    while len(pairs) < N - 1:
        act = np.nonzero(size > 0)[0]
        sub = D[np.ix_(act, act)]
        nn = act[np.argmin(sub, axis=1)]                          # (argmin: the first of equal values = the smallest index)
        if len(act) > 2:
            two = np.partition(sub, 1, axis=1)[:, :2]
            with np.errstate(invalid="ignore", divide="ignore"):
                gap = (two[:, 1] - two[:, 0]) / two[:, 0]
            nn_gap = min(nn_gap, float(np.nanmin(np.where(np.isfinite(gap), gap, np.inf))))
        nn_of = dict(zip(act.tolist(), nn.tolist()))
        found = [(i, j) for i, j in nn_of.items() if j > i and nn_of[j] == i]
        assert found, "no mutual pair"
        n_rounds += 1
        for i, j in found:
            h = D[i, j]
            k = np.nonzero(size > 0)[0]
            k = k[(k != i) & (k != j)]
            v = _ward(D[i, k], D[j, k], h, size[i], size[j], size[k])
            D[i, k] = v
            D[k, i] = v
            size[i] += size[j]
            size[j] = 0
            D[j, :] = np.inf
            D[:, j] = np.inf
            pairs.append((i, j))
            heights.append(h)
            sizes.append(size[i])
    return {"pairs": np.array(pairs, dtype=np.int64), "heights": np.array(heights), "sizes": np.array(sizes), "rounds": n_rounds,
            "nn_gap": nn_gap}


def height_gap(heights):
    """the smallest relative difference between consecutive sorted heights"""
    h = np.sort(np.asarray(heights, dtype=np.float64))
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.min((h[1:] - h[:-1]) / h[1:])) if len(h) > 1 else np.inf


def tree(pairs, heights, N):
    """scipy's label(): the merges in ascending height (stable), each naming the current clusters of its two rows through a
    union-find, the smaller id first; merge t makes node N + t -> (children (N - 1, 2), distances)"""
    order = np.argsort(np.asarray(heights), kind="stable")
    parent = list(range(2 * N - 1))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    children = np.empty((N - 1, 2), dtype=np.int64)
    for t, at in enumerate(order):
        a, b = find(int(pairs[at][0])), find(int(pairs[at][1]))
        children[t] = (min(a, b), max(a, b))
        parent[a] = parent[b] = N + t
    return children, np.asarray(heights, dtype=np.float64)[order]


def _leaves(node, children, N):
    out, stack = [], [node]
    while stack:
        n = stack.pop()
        if n < N:
            out.append(n)
        else:
            stack.extend(children[n - N])
    return out


def cut(n_clusters, children, N):
    """sklearn's _hc_cut: labels in the order of its heap of negated node ids"""
    nodes = [-(int(max(children[-1])) + 1)]
    for _ in range(n_clusters - 1):
        these = children[-nodes[0] - N]
        heapq.heappush(nodes, -int(these[0]))
        heapq.heappushpop(nodes, -int(these[1]))
    label = np.zeros(N, dtype=np.int64)
    for i, node in enumerate(nodes):
        label[_leaves(-node, children, N)] = i
    return label


def fit(X):
    """-> dict(children, distances, rounds, nn_gap, height_gap)"""
    r = rounds(X)
    children, dist = tree(r["pairs"], r["heights"], len(X))
    return {"children": children, "distances": dist, "rounds": r["rounds"], "nn_gap": r["nn_gap"], "height_gap": height_gap(dist)}
