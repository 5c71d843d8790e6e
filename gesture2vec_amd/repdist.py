"""Pairwise-distance statistics of latent rows and the reference's representation-similarity metric, on the device
(`calculate_distances`, `Clustering.py:410-505`, which writes `Rep_distance.txt`): are chunks that follow each other in time closer in
latent space than chunks picked at random?

    pairwise_distance_stats    count, sum, sum of squares, min, max, mean, std and a histogram over ALL pairs of rows (or all pairs
                               between two sets), reduced as the pairs are formed: no distance is stored, where the reference's
                               `np.mean(pdist(latents))` holds N (N - 1) / 2 float64 values (69 GB at 131072 rows)
    lag_distances              every row's mean distance to the rows `lag` before and behind it
    representation_similarity  the reference's nine numbers for one of its two methods
    representation_report      the text of `Rep_distance.txt`

The kernels are csrc/pair_stats.hip (ops.pair_stats, ops.lag_distances): Gram tiles on the float64 MFMA with near pairs evaluated
again from differences, d^2 kept in float64, fixed-order sums, no floating-point atomics.  The same input gives the same bits on
every call and every device.  scipy is not imported.

The reference forms the neighbour distances and their means in float32 (its latents are float32); here they are float64, so the
neighbour numbers agree with the reference's to about 1e-7 relative and `avg_dist_total`, float64 on both sides, to 1e-13."""
from __future__ import annotations

import math
import random as _random

import numpy as np
import torch

KEYS = ("avg_20fs", "std_20fs", "avg_10fs", "std_10fs", "avg_dist_total", "normal_avg_20fs", "normal_std_20fs", "normal_avg_10fs",
        "normal_std_10fs")
METHODS = ("all", "random")
_LAGS = (1, 2)          # "20fs": one chunk away, "10fs": two


def _rows(x, name: str, what: str, layout: bool = True) -> torch.Tensor:
    """x as the kernels take it: (N, E) fp32 on the GPU, unit column stride, the row stride a multiple of 4, 16-byte aligned (a view
    that is not is copied; layout=False only checks)"""
    if not torch.is_tensor(x):
        raise TypeError(f"{what}: {name} must be a torch tensor, got {type(x).__name__}")
    if not x.is_cuda:
        raise TypeError(f"{what}: {name} must be a GPU tensor (the kernels have no CPU path)")
    if x.dim() != 2 or x.dtype != torch.float32:
        raise TypeError(f"{what}: {name} must be a (N, E) fp32 tensor, got {tuple(x.shape)} {x.dtype}")
    N, E = x.shape
    if N < 1 or not 1 <= E <= 512:
        raise ValueError(f"{what}: {name} needs at least one row and 1 <= E <= 512, got {tuple(x.shape)}")
    if layout and (x.stride(1) != 1 or x.stride(0) % 4 != 0 or x.stride(0) < E or x.data_ptr() % 16 != 0):
        x = x.contiguous()
        if x.stride(0) % 4 != 0 or x.data_ptr() % 16 != 0:       # E % 4 != 0: a row stride of whole 16-byte vectors
            wide = torch.zeros((N, (E + 3) // 4 * 4), dtype=torch.float32, device=x.device)
            wide[:, :E] = x
            x = wide[:, :E]
    return x


def histogram_edges(bins, range=None) -> np.ndarray:
    """The float64 edges of `bins`: an int with range=(lo, hi) gives numpy.linspace(lo, hi, bins + 1), which is what numpy.histogram
    uses; a 1-D ascending array is taken as the edges.  ValueError for anything else."""
    if isinstance(bins, (int, np.integer)) and not isinstance(bins, bool):
        if range is None:
            raise ValueError("an integer `bins` needs `range=(lo, hi)`: finding the range would take a pass of its own, and `min` / "
                             "`max` of a first call without bins give it")
        if bins < 1:
            raise ValueError(f"`bins` must be positive, got {bins}")
        lo, hi = (float(v) for v in range)
        if not (math.isfinite(lo) and math.isfinite(hi)) or not lo < hi:
            raise ValueError(f"`range` must be finite with lo < hi, got {range!r}")
        return np.linspace(lo, hi, int(bins) + 1, dtype=np.float64)
    if range is not None:
        raise ValueError("`range` goes with an integer `bins`, not with an array of edges")
    if torch.is_tensor(bins):
        bins = bins.detach().cpu().numpy()
    edges = np.asarray(bins, dtype=np.float64)
    if edges.ndim != 1 or edges.size < 2:
        raise ValueError(f"`bins` must be an int or a 1-D array of at least 2 edges, got shape {edges.shape}")
    if not np.isfinite(edges).all() or not (np.diff(edges) > 0).all():
        raise ValueError("the edges in `bins` must be finite and strictly ascending")
    return edges


@torch.no_grad()
def pairwise_distance_stats(x, y=None, *, bins=None, range=None) -> dict:
    """Statistics of the Euclidean distances over the pairs i < j of the rows of x (N, E) fp32, or with y (M, E) over all N M pairs:
    count, nonfinite (ints), sum, sum_sq (of the squared distances themselves), min, max, mean, std (population, as np.std of the
    distances: sqrt(max(0, sum_sq / count - mean^2))) as floats; with `bins` also hist (int64, on the device) and edges (numpy), counted
    as numpy.histogram counts them.  Without a pair: sums 0, min inf, max -inf, mean and std NaN.  A NaN distance is counted in
    nonfinite and in no bin, makes the sums NaN and is passed over by min and max."""
    from . import ops
    what = "pairwise_distance_stats"
    _rows(x, "x", what, layout=False)
    if y is not None:
        _rows(y, "y", what, layout=False)
        if y.shape[1] != x.shape[1] or y.device != x.device:
            raise ValueError(f"{what}: y must be (M, {x.shape[1]}) on the device of x, got {tuple(y.shape)} on {y.device}")
    for name, t in (("x", x), ("y", y)):
        if t is not None and t.shape[0] > ops.pair_stats_max_rows():
            raise ValueError(f"{what}: {name} has {t.shape[0]} rows, more than {ops.pair_stats_max_rows()}")
    edges = None
    if bins is not None:
        edges = histogram_edges(bins, range)
        if edges.size - 1 > ops.pair_stats_max_bins():
            raise ValueError(f"{what}: {edges.size - 1} bins exceed the limit of {ops.pair_stats_max_bins()}")
    elif range is not None:
        raise ValueError(f"{what}: `range` without `bins`")
    x = _rows(x, "x", what)                                      # (every refusal above comes before the first launch)
    y = None if y is None else _rows(y, "y", what)
    out, counts, hist = ops.pair_stats(x, y, None if edges is None else torch.from_numpy(edges).to(x.device))
    s, sq, lo, hi = (float(v) for v in out.cpu().numpy())
    count, bad = (int(v) for v in counts.cpu().numpy())
    mean = s / count if count else float("nan")
    var = sq / count - mean * mean if count else float("nan")
    std = var if math.isnan(var) else math.sqrt(max(0.0, var))   # (max(0.0, nan) is 0.0: a NaN is passed on by hand)
    res = {"count": count, "sum": s, "sum_sq": sq, "min": lo, "max": hi, "nonfinite": bad, "mean": mean, "std": std}
    if edges is not None:
        res["hist"], res["edges"] = hist, edges
    return res


@torch.no_grad()
def lag_distances(x, lags=_LAGS, clip_ids=None) -> torch.Tensor:
    """(n_lags, N) float64 on the device: out[l][i] = (|x_{i - lag} - x_i| + |x_{i + lag} - x_i|) / 2, NaN where a neighbour is past
    either end or, with clip_ids (N integers), belongs to another clip than row i.  Without clip_ids all rows are one sequence, which
    is the reference's reading."""
    from . import ops
    x = _rows(x, "x", "lag_distances")
    lags = [lags] if isinstance(lags, (int, np.integer)) else list(lags)
    if not 1 <= len(lags) <= 8:
        raise ValueError(f"lag_distances: needs 1 to 8 lags, got {len(lags)}")
    for v in lags:
        if isinstance(v, bool) or int(v) != v or not 1 <= int(v) < 2 ** 31:
            raise ValueError(f"lag_distances: every lag must be an integer >= 1, got {v!r}")
    if clip_ids is not None:
        clip_ids = torch.as_tensor(clip_ids)
        if clip_ids.dim() != 1 or clip_ids.shape[0] != x.shape[0] or clip_ids.dtype.is_floating_point or clip_ids.dtype == torch.bool:
            raise ValueError(f"lag_distances: clip_ids must be ({x.shape[0]},) integers, got {tuple(clip_ids.shape)} {clip_ids.dtype}")
        clip_ids = clip_ids.to(device=x.device, dtype=torch.int64).contiguous()
    return ops.lag_distances(x, [int(v) for v in lags], clip_ids)


def similarity_rows(N: int, method: str = "all", n_random: int = 1000, seed=None, margin: int = 2):
    """The rows representation_similarity uses: range(margin, N - margin), or for "random" random.Random(seed).sample of it, which
    after random.seed(seed) is the reference's own sample"""
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, got {method!r}")
    if isinstance(margin, bool) or int(margin) != margin or int(margin) < max(_LAGS):
        raise ValueError(f"margin must be an integer >= {max(_LAGS)} (the longest lag), got {margin!r}")
    rows = range(int(margin), int(N) - int(margin))
    if len(rows) < 1:
        raise ValueError(f"{N} rows leave none between the margins of {margin}")
    if method == "all":
        return rows
    if isinstance(n_random, bool) or int(n_random) != n_random or int(n_random) < 1:
        raise ValueError(f"n_random must be a positive integer, got {n_random!r}")
    if int(n_random) > len(rows):
        raise ValueError(f"n_random = {n_random} exceeds the {len(rows)} rows between the margins")
    return _random.Random(seed).sample(rows, int(n_random))


def _similarity(lagd: torch.Tensor, avg_total: float, rows, drop_nan: bool) -> dict:
    if isinstance(rows, range):
        v = lagd[:, rows.start:rows.stop]
    else:
        v = lagd.index_select(1, torch.tensor(rows, dtype=torch.int64).to(lagd.device))
    vals = []
    for l in (0, 1):
        r = v[l]
        if drop_nan:
            r = r[~torch.isnan(r)]
        if r.numel() == 0:
            vals += [float("nan")] * 4
            continue
        n = r / avg_total
        vals += [r.mean(), r.std(unbiased=False), n.mean(), n.std(unbiased=False)]
    vals = [float(t) for t in torch.stack([torch.as_tensor(t, dtype=torch.float64, device=lagd.device) for t in vals]).cpu()]
    a20, s20, na20, ns20, a10, s10, na10, ns10 = vals
    return {"avg_20fs": a20, "std_20fs": s20, "avg_10fs": a10, "std_10fs": s10, "avg_dist_total": avg_total,
            "normal_avg_20fs": na20, "normal_std_20fs": ns20, "normal_avg_10fs": na10, "normal_std_10fs": ns10}


@torch.no_grad()
def representation_similarity(latents, *, method="all", n_random=1000, seed=None, margin=2, clip_ids=None) -> dict:
    """The reference's representation-similarity numbers of latents (N, E) fp32 for one `method`, keyed as it prints them: avg_20fs,
    std_20fs (the distance to the rows one chunk away, mean and population std over the rows used), avg_10fs, std_10fs (two chunks
    away), avg_dist_total (the mean distance over ALL pairs of ALL rows) and normal_* (the neighbour distances divided by
    avg_dist_total, then mean and std).  With clip_ids a row whose neighbour lies in another clip is left out.  Only the index
    sample and the final scalars touch the host."""
    _rows(latents, "latents", "representation_similarity", layout=False)
    rows = similarity_rows(latents.shape[0], method, n_random, seed, margin)   # (refusals come before any launch)
    x = _rows(latents, "latents", "representation_similarity")
    lagd = lag_distances(x, _LAGS, clip_ids)
    return _similarity(lagd, pairwise_distance_stats(x)["mean"], rows, clip_ids is not None)


@torch.no_grad()
def representation_report(latents, seed=None) -> str:
    """The text the reference writes to Rep_distance.txt: both methods under its headings and in its line layout, floats as str()
    prints them.  seed: of the "random" method's sample."""
    _rows(latents, "latents", "representation_report", layout=False)
    plan = [(m, similarity_rows(latents.shape[0], m, 1000, seed, 2)) for m in METHODS]
    x = _rows(latents, "latents", "representation_report")
    lagd = lag_distances(x, _LAGS)
    avg = pairwise_distance_stats(x)["mean"]
    text = "=====Representation similarity at the embedding space.=====\n\n"
    for method, rows in plan:
        r = _similarity(lagd, avg, rows, False)
        text += "\n\n==========================\nMethod: {}\n".format(method)
        text += ("Representation Similarity metric\n" + "avg_20fs={} -- std_20fs={}\navg_10fs={} -- std_10fs={}\n".format(
            r["avg_20fs"], r["std_20fs"], r["avg_10fs"], r["std_10fs"]))
        text += ("\nStandardized:\n" + "average distance total: " + str(r["avg_dist_total"]) + "\nstandardized distances\n" +
                 "normal_avg_20fs={} -- normal_std_20fs={}\nnormal_avg_10fs={} -- normal_std_10fs={}\n".format(
                     r["normal_avg_20fs"], r["normal_std_20fs"], r["normal_avg_10fs"], r["normal_std_10fs"]))
        text += "\n\n"
    return text


def parse_report(text: str) -> dict:
    """{method: {key: float}} out of the text of a Rep_distance.txt, the reference's or representation_report's"""
    res, cur = {}, None
    for line in text.splitlines():
        line = line.strip()
        if line.startswith("Method: "):
            cur = res.setdefault(line[len("Method: "):], {})
        elif cur is not None and line.startswith("average distance total: "):
            cur["avg_dist_total"] = float(line[len("average distance total: "):])
        elif cur is not None and "=" in line and not line.startswith("="):
            for part in line.split(" -- "):
                k, v = part.split("=")
                cur[k.strip()] = float(v)
    return res
