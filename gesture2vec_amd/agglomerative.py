"""Ward agglomerative clustering of latent rows on the device, with the tree and the labels of
`sklearn.cluster.AgglomerativeClustering(linkage="ward", n_clusters=k).fit(latents)`: the last sklearn branch of the reference's
clustering switch (`Clustering.py:751-755`).  sklearn and scipy are not imported.

sklearn's Ward tree is `scipy.cluster.hierarchy.ward`: a float64 condensed distance matrix and a serial nearest-neighbour chain.  Ward
linkage is reducible, so clusters that are each other's nearest neighbour may be merged at any time, and all such pairs at once.
`fit` is two kinds of calls (csrc/ward.hip):

    ops.ward_distances   the dense float64 matrix of unsquared distances (8 N^2 bytes), formed once on the float64 MFMA
    ops.ward_rounds      rounds of: nearest active neighbour of every cluster that needs it, all mutual pairs logged and merged with
                         scipy's Ward update in place; `check_every` rounds are enqueued per read-back of the merge count

The O(N) bookkeeping of the tree runs on the host in numpy: the merge log is sorted by height (a stable sort, the log's order breaks
ties), relabelled as scipy relabels it (merge i makes node N + i, the smaller id first in `children_[i]`), and cut as sklearn's
`_hc_cut` cuts it, so label numbers are sklearn's own.  One fitted tree answers every k: `cut(k)`.

fp32 distances are not enough for this: on the recorded inputs a row's best and second-best neighbour differ by as little as 5.8e-6
relative and consecutive heights by 3.7e-6 (tests/golden/ward.npz, 300 rows of width 400), so the matrix and the updates are float64.

Labels are those of `_hc_cut` over the full tree, which is what sklearn does for every n_clusters when no `connectivity` is given
(it then sets compute_full_tree to True whatever was asked for).

Exact ties (duplicate rows, rows on a grid): the nearest neighbour is then the one with the smallest index and mutual pairs at one
height are ordered by the round and the slot, so the result is a valid Ward tree and the same bits on every call, but not
necessarily the tree scipy's chain finds.  Duplicate rows merge at height 0 before anything else."""
from __future__ import annotations

import heapq

import numpy as np
import torch

from .pipeline import _need_cuda


def check_rows(N: int, what: str = "AgglomerativeClustering") -> None:
    """ValueError beyond the rows the distance matrix is built for"""
    from . import ops
    limit = ops.ward_max_rows()
    if N > limit:
        raise ValueError(f"{what}: {N} rows exceed the limit of {limit} (the float64 distance matrix takes 8 N^2 bytes, 8 GiB at the limit)")


def tree_from_log(pairs, heights, N):
    """The device's merge log (slots (i, j) in round order, heights) -> (children (N - 1, 2) int64, distances (N - 1) float64) as
    scipy's `ward` orders and numbers them.  A slot holds the node last made in it: every merge below a cluster is lower than the
    merge that consumes it, so after the sort the slot's node is the one the device merged."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)[:N - 1]
    heights = np.asarray(heights, dtype=np.float64)[:N - 1]
    order = np.argsort(heights, kind="stable")
    node = np.arange(N, dtype=np.int64)
    children = np.empty((N - 1, 2), dtype=np.int64)
    for t, at in enumerate(order):
        i, j = pairs[at]
        a, b = node[i], node[j]
        children[t] = (a, b) if a < b else (b, a)
        node[i] = N + t
    return children, heights[order]


def hc_cut(n_clusters, children, n_leaves):
    """sklearn.cluster._agglomerative._hc_cut: the n_clusters top nodes of the tree from a heap of negated ids, numbered in the heap
    list's order, and every leaf labelled with its node (pushed down the tree from the root instead of collected per node)."""
    if n_clusters > n_leaves:
        raise ValueError(f"Cannot extract more clusters than samples: {n_clusters} clusters were given for a tree with {n_leaves} leaves.")
    children = np.asarray(children, dtype=np.int64)
    nodes = [-(int(max(children[-1])) + 1)]
    for _ in range(n_clusters - 1):
        these = children[-nodes[0] - n_leaves]
        heapq.heappush(nodes, -int(these[0]))
        heapq.heappushpop(nodes, -int(these[1]))
    label = np.full(2 * n_leaves - 1, -1, dtype=np.int64)
    for i, node in enumerate(nodes):
        label[-node] = i
    for t in range(n_leaves - 2, -1, -1):                        # a node's children have smaller ids than the node
        if label[n_leaves + t] >= 0:
            label[children[t]] = label[n_leaves + t]
    return label[:n_leaves]


class AgglomerativeClustering:
    def __init__(self, n_clusters=2, *, metric="euclidean", linkage="ward", distance_threshold=None, compute_distances=False,
                 check_every=4, **refused):
        for name, value in refused.items():
            if name in ("connectivity", "memory"):
                if value is not None:
                    raise TypeError(f"AgglomerativeClustering: `{name}` is not supported (the full tree over all pairs on the device)")
            elif name == "compute_full_tree":
                if value not in ("auto", True):
                    raise TypeError("AgglomerativeClustering: `compute_full_tree` must be 'auto' or True (the full tree is always built)")
            else:
                raise TypeError(f"AgglomerativeClustering: unexpected argument `{name}`")
        if linkage != "ward":
            raise ValueError(f"AgglomerativeClustering: linkage must be 'ward', got {linkage!r}")
        if metric != "euclidean":
            raise ValueError(f"AgglomerativeClustering: metric must be 'euclidean' (ward needs it), got {metric!r}")
        if not ((n_clusters is None) ^ (distance_threshold is None)):
            raise ValueError("AgglomerativeClustering: exactly one of n_clusters and distance_threshold has to be set, "
                             "and the other needs to be None")
        if n_clusters is not None and (int(n_clusters) != n_clusters or int(n_clusters) < 1):
            raise ValueError(f"AgglomerativeClustering: n_clusters must be an integer >= 1, got {n_clusters!r}")
        if distance_threshold is not None and not float(distance_threshold) >= 0.0:
            raise ValueError(f"AgglomerativeClustering: distance_threshold must be >= 0, got {distance_threshold!r}")
        if int(check_every) < 1:
            raise ValueError("AgglomerativeClustering: check_every must be positive")
        self.n_clusters = None if n_clusters is None else int(n_clusters)
        self.metric = metric
        self.linkage = linkage
        self.distance_threshold = None if distance_threshold is None else float(distance_threshold)
        self.compute_distances = bool(compute_distances)
        self.check_every = int(check_every)
        self.labels_ = None                 # (N) int64, on the device
        self.children_ = None               # (N - 1, 2) int64 numpy
        self.distances_ = None              # (N - 1) float64 numpy, with compute_distances or a threshold
        self.n_clusters_ = None
        self.n_leaves_ = None
        self.n_connected_components_ = None
        self.n_features_in_ = None
        self.n_rounds_ = None               # rounds that merged at least one pair

    def __getstate__(self):
        d = dict(self.__dict__)
        if torch.is_tensor(d["labels_"]):
            d["labels_"] = d["labels_"].cpu()
        return d

    @torch.no_grad()
    def fit(self, x: torch.Tensor, y=None) -> "AgglomerativeClustering":
        """x: (N, E) fp32 GPU tensor, N >= 2, 1 <= E <= 512"""
        from . import ops
        _need_cuda(x, "AgglomerativeClustering.fit")
        if x.dim() != 2 or x.dtype != torch.float32:
            raise TypeError(f"AgglomerativeClustering.fit: expected a (N, E) fp32 tensor, got {tuple(x.shape)} {x.dtype}")
        N, E = x.shape
        if N < 2:
            raise ValueError(f"AgglomerativeClustering.fit: needs at least 2 rows, got {N}")
        if self.n_clusters is not None and self.n_clusters > N:
            raise ValueError(f"AgglomerativeClustering.fit: n_clusters = {self.n_clusters} exceeds the {N} rows")
        check_rows(N, "AgglomerativeClustering.fit")
        if not bool(torch.isfinite(x).all()):
            raise ValueError("AgglomerativeClustering.fit: the rows contain NaN or infinity")
        if x.stride(1) != 1 or x.stride(0) % 4 != 0 or x.data_ptr() % 16 != 0:
            x = x.contiguous()
            if x.stride(0) % 4 != 0:                             # E % 4 != 0: a row stride of whole 16-byte vectors
                wide = torch.zeros((N, (E + 3) // 4 * 4), dtype=torch.float32, device=x.device)
                wide[:, :E] = x
                x = wide[:, :E]
        D = ops.ward_distances(x)
        state = ops.ward_state(N, x.device)
        enqueued, first = 0, True
        while True:
            counters = ops.ward_rounds(D, state, init=first, rounds=self.check_every).cpu().numpy()
            first = False
            if int(counters[0]) >= N - 1:
                break
            enqueued += self.check_every
            if enqueued > N:                                     # every round with two clusters left merges at least one pair
                raise RuntimeError("AgglomerativeClustering.fit: the merges did not finish within N rounds")
        del D
        children, heights = tree_from_log(state["pairs"].cpu().numpy(), state["heights"].cpu().numpy(), N)
        self.children_ = children
        self.n_leaves_, self.n_connected_components_, self.n_features_in_ = int(N), 1, int(E)
        self.n_rounds_ = int(counters[1])
        if self.distance_threshold is not None:
            self.n_clusters_ = int(np.count_nonzero(heights >= self.distance_threshold)) + 1
        else:
            self.n_clusters_ = self.n_clusters
        self.distances_ = heights if (self.compute_distances or self.distance_threshold is not None) else None
        self.labels_ = torch.from_numpy(hc_cut(self.n_clusters_, children, N)).to(x.device)
        return self

    def fit_predict(self, x: torch.Tensor, y=None) -> torch.Tensor:
        return self.fit(x).labels_

    def cut(self, n_clusters: int) -> torch.Tensor:
        """Labels (N) int64 of the fitted tree at another n_clusters, as a fresh fit at that n_clusters gives them, without refitting
        (on the device of `labels_`)"""
        if self.children_ is None:
            raise RuntimeError("AgglomerativeClustering.cut: fit first")
        if int(n_clusters) != n_clusters or not 1 <= int(n_clusters) <= self.n_leaves_:
            raise ValueError(f"AgglomerativeClustering.cut: n_clusters must be an integer in [1, {self.n_leaves_}], got {n_clusters!r}")
        return torch.from_numpy(hc_cut(int(n_clusters), self.children_, self.n_leaves_)).to(self.labels_.device)
