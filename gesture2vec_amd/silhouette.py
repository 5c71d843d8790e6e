"""Silhouette coefficient of a clustering of latent rows, on the device: the model-selection curve of the reference's k scan
(`Clustering.py:608-624`, `sklearn.metrics.silhouette_score(latents, labels)` per k).  Arguments and meaning follow
`sklearn.metrics.silhouette_samples` / `silhouette_score` with the Euclidean metric; sklearn itself is not imported.

The work is one call of `g2v_silhouette_samples` (csrc/silhouette.hip): rows sorted by label, Gram products on the exact-fp32 MFMA,
sqrt in the accumulator epilogue, near pairs re-evaluated from differences, float64 sums in a fixed order -- neither the N x N
distances nor an N x K table exist, and the same input gives the same bits."""
from __future__ import annotations

import numpy as np
import torch

from .pipeline import _need_cuda


def _rows_and_labels(x, labels, what):
    _need_cuda(x, what)
    if x.dim() != 2 or x.dtype != torch.float32:
        raise TypeError(f"{what}: expected a (N, E) fp32 tensor, got {tuple(x.shape)} {x.dtype}")
    if x.stride(1) != 1 or x.stride(0) % 4 != 0 or x.data_ptr() % 16 != 0:
        x = x.contiguous()
    lab = labels if torch.is_tensor(labels) else torch.from_numpy(np.ascontiguousarray(np.asarray(labels).astype(np.int64)))
    lab = lab.to(device=x.device, dtype=torch.int64).reshape(-1).contiguous()
    if lab.numel() != x.shape[0]:
        raise ValueError(f"{what}: {x.shape[0]} rows but {lab.numel()} labels")
    return x, lab


def _run(x, labels, n_clusters, what):
    from . import ops
    x, lab = _rows_and_labels(x, labels, what)
    N = x.shape[0]
    if N < 2:
        raise ValueError(f"{what}: needs at least 2 rows")
    K = int(lab.max().item()) + 1 if n_clusters is None else int(n_clusters)
    if K < 1:
        raise ValueError(f"{what}: labels must be non-negative cluster ids")
    res = ops.silhouette_samples(x, lab, K)
    counts, out = res["counts"].cpu().numpy(), res["out"].cpu().numpy()
    if counts[K] != 0:
        raise ValueError(f"{what}: {int(counts[K])} labels are outside [0, {K})")
    n_labels = int(out[1])
    if not 1 < n_labels < N:                                 # sklearn's check_number_of_labels
        raise ValueError(f"Number of labels is {n_labels}. Valid values are 2 to n_samples - 1 (inclusive)")
    return res, float(out[0]), N


@torch.no_grad()
def silhouette_samples(x: torch.Tensor, labels, n_clusters=None) -> torch.Tensor:
    """(N, E) fp32 GPU rows and N cluster ids -> (N,) float64 GPU silhouette coefficients.  `n_clusters`: ids run over
    [0, n_clusters); None infers max(labels) + 1.  ValueError unless 2 <= non-empty clusters <= N - 1."""
    return _run(x, labels, n_clusters, "silhouette_samples")[0]["s"]


@torch.no_grad()
def silhouette_score(x: torch.Tensor, labels, sample_size=None, random_state=None, n_clusters=None) -> float:
    """Mean silhouette coefficient.  `sample_size` rows are drawn as sklearn draws them:
    `numpy.random.RandomState(random_state).permutation(N)[:sample_size]`."""
    if sample_size is not None:
        x, labels = _rows_and_labels(x, labels, "silhouette_score")
        rs = random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(random_state)
        idx = torch.from_numpy(rs.permutation(x.shape[0])[:int(sample_size)].astype(np.int64)).to(x.device)
        x, labels = x[idx].contiguous(), labels[idx]         # gathers: layout only
    _, total, n = _run(x, labels, n_clusters, "silhouette_score")
    return total / n
