"""DBSCAN over latent rows on the device, labelled as `sklearn.cluster.DBSCAN(eps, min_samples).fit(latents)` labels them: the other
branch of the reference's clustering switch (`Clustering.py:742-750`, again at `:962-969`), the one that says how many clusters the
latent space holds and which chunks belong to none.  sklearn itself is not imported.

sklearn's `dbscan_inner` is sequential, but its result is fixed by the eps-graph.  With adj(i, j) <=> |x_i - x_j| <= eps (a row is
its own neighbour): a row is core iff it has >= min_samples neighbours; a core row's root is the smallest index in its connected
component of the core rows; a component's cluster id is the rank of its root among all roots; a row that is not core takes the
smallest id among its core neighbours, or -1.  `fit` is three kinds of calls (csrc/dbscan.hip):

    ops.dbscan_neighbors   the adjacency as a bitmap (N^2 / 8 bytes) and the neighbour counts; distances are formed here, once,
                           on the exact-fp32 MFMA, and every pair near eps is decided again in float64 from differences
    ops.dbscan_propagate   rounds of min-propagation with pointer jumping until a round changes nothing; `check_every` rounds are
                           enqueued per read-back of the flags
    ops.dbscan_labels      ranks of the roots, labels, the core mask, the three counts

The same input gives the same bits.  `k_distances(x, k)` is the sorted k-distance curve `eps` is usually read from."""
from __future__ import annotations

import numpy as np
import torch

from .pipeline import _need_cuda

_REFUSED = ("sample_weight", "algorithm", "leaf_size", "p", "n_jobs")


def check_rows(N: int, what: str = "DBSCAN") -> None:
    """ValueError beyond the rows the adjacency bitmap is built for"""
    from . import ops
    limit = ops.dbscan_max_rows()
    if N > limit:
        raise ValueError(f"{what}: {N} rows exceed the limit of {limit} (the adjacency bitmap takes N^2 / 8 bytes, 2 GiB at the limit)")


@torch.no_grad()
def k_distances(x: torch.Tensor, k) -> torch.Tensor:
    """The curve one reads `eps` from: the distance from each row of x (N, E) to its k-th nearest row COUNTING ITSELF, which is how
    DBSCAN counts `min_samples` (k = 1 gives zeros), sorted ascending -> (N,) fp32 on the device.  `embedding.kneighbors` with the
    rows as their own queries (exact neighbours, the N x N distances never stored) and one sort.  k <= min(N, 127)."""
    from .embedding import kneighbors
    _need_cuda(x, "k_distances")
    dist, _ = kneighbors(x, k, queries=x)
    return dist[:, int(k) - 1].sort().values


class DBSCAN:
    def __init__(self, eps=0.5, min_samples=5, metric="euclidean", check_every=4, **refused):
        for name in refused:
            if name in _REFUSED:
                raise TypeError(f"DBSCAN: `{name}` is not supported (euclidean distances over all pairs on the device, unit weights)")
            raise TypeError(f"DBSCAN: unexpected argument `{name}`")
        if metric != "euclidean":
            raise ValueError(f"DBSCAN: metric must be 'euclidean', got {metric!r}")
        if not float(eps) > 0.0 or not np.isfinite(float(eps)):
            raise ValueError(f"DBSCAN: eps must be a positive finite number, got {eps!r}")
        if int(min_samples) != min_samples or int(min_samples) < 1:
            raise ValueError(f"DBSCAN: min_samples must be an integer >= 1, got {min_samples!r}")
        if int(check_every) < 1:
            raise ValueError("DBSCAN: check_every must be positive")
        self.eps = float(eps)
        self.min_samples = int(min_samples)
        self.metric = metric
        self.check_every = int(check_every)
        self.labels_ = None                 # (N) int64, on the device
        self.core_sample_indices_ = None    # ascending int64, on the device
        self.components_ = None             # the core rows (a gather)
        self.n_features_in_ = None
        self.n_clusters_ = None
        self.n_noise_ = None
        self.n_rounds_ = None               # propagation rounds until one changed nothing, that one included
        self._dev = {}                      # the last fit's neighbour counts and core mask; never pickled

    def __getstate__(self):
        d = dict(self.__dict__)
        d["_dev"] = {}
        for k in ("labels_", "core_sample_indices_", "components_"):
            if torch.is_tensor(d[k]):
                d[k] = d[k].cpu()
        return d

    @torch.no_grad()
    def fit(self, x: torch.Tensor, y=None, sample_weight=None) -> "DBSCAN":
        """x: (N, E) fp32 GPU tensor, 1 <= E <= 512"""
        from . import ops
        if sample_weight is not None:
            raise TypeError("DBSCAN.fit: `sample_weight` is not supported")
        _need_cuda(x, "DBSCAN.fit")
        if x.dim() != 2 or x.dtype != torch.float32:
            raise TypeError(f"DBSCAN.fit: expected a (N, E) fp32 tensor, got {tuple(x.shape)} {x.dtype}")
        N, E = x.shape
        if N < 1:
            raise ValueError("DBSCAN.fit: needs at least 1 row")
        check_rows(N, "DBSCAN.fit")
        if x.stride(1) != 1 or x.stride(0) % 4 != 0 or x.data_ptr() % 16 != 0:
            x = x.contiguous()
            if x.stride(0) % 4 != 0:                             # E % 4 != 0: a row stride of whole 16-byte vectors
                wide = torch.zeros((N, (E + 3) // 4 * 4), dtype=torch.float32, device=x.device)
                wide[:, :E] = x
                x = wide[:, :E]
        bitmap, counts = ops.dbscan_neighbors(x, self.eps)
        L = torch.empty((N,), dtype=torch.int32, device=x.device)
        tmp = torch.empty_like(L)
        rounds, first = 0, True
        while True:
            flags = ops.dbscan_propagate(bitmap, counts, self.min_samples, L, tmp, init=first, rounds=self.check_every).cpu().numpy()
            first = False
            still = np.nonzero(flags == 0)[0]
            if len(still):
                rounds += int(still[0]) + 1
                break
            rounds += len(flags)
            if rounds > N + self.check_every:
                raise RuntimeError("DBSCAN.fit: the propagation did not converge within N rounds")
        labels, core, out = ops.dbscan_labels(bitmap, L)
        n_clusters, _, n_noise = (int(v) for v in out.cpu().numpy())
        self.labels_ = labels
        self.core_sample_indices_ = torch.nonzero(core, as_tuple=False).reshape(-1)
        self.components_ = x[self.core_sample_indices_].contiguous()     # a gather: layout only
        self.n_features_in_ = int(E)
        self.n_clusters_, self.n_noise_, self.n_rounds_ = n_clusters, n_noise, rounds
        self._dev = {"counts": counts, "core": core}
        return self

    def fit_predict(self, x: torch.Tensor, y=None, sample_weight=None) -> torch.Tensor:
        return self.fit(x, sample_weight=sample_weight).labels_
