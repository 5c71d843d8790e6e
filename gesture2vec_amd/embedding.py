"""2-D maps of latent rows and codebooks, on the device: the reference's `PCA(50)` + `TSNE(n_components=2, perplexity=30)` pictures of
the codebook (`train_autoencoder_VQVAE.py:450-505`, `train_DAE.py:516-526`, `inference_Autoencoder.py:269-277`) and of all chunk
latents coloured by code (`Clustering.py:1046-1056`, `:1411-1417`).  Arguments, attributes and the optimisation schedule follow
`sklearn.decomposition.PCA` and `sklearn.manifold.TSNE(method="exact")` (sklearn 1.7); sklearn itself is not imported.

* `PCA`: the float64 covariance comes from `metrics.LatentMoments` (g2v_moments_accumulate: one pass over the rows), a host
  `numpy.linalg.eigh` of the E x E matrix gives the components, `transform` is one g2v_linear_fwd with bias -mean C^T.
* `TSNE`: g2v_tsne_affinities builds the dense joint P once (csrc/tsne.hip), every iteration is g2v_tsne_gradient (one pass over P)
  + g2v_tsne_update; the host reads the KL divergence and the gradient norm back every 50 iterations, where sklearn checks its two
  stop rules.  Only `n_components == 2` and the exact method exist; N <= `ops.tsne_max_rows()` rows.
* `TSNE.transform` places new rows into the fitted map, as the reference's `make_unity_scatter(latents, labels, file, pca, MyTSNE)`
  does with `MyTSNE.transform(pca.transform(latents))` (`Clustering.py:1318-1350`): openTSNE's structure and `transform` defaults,
  stated exactly in DESIGN 3.5e (csrc/tsne_place.hip: exact neighbours among the fitted rows, their conditionals, a median start,
  then a per-row descent against the fixed map in one launch).  Every row is placed on its own, so a set of any size can be placed
  against an exactly fitted sample.  `LatentMap` is the reference's `(pca, MyTSNE)` pair as one picklable object.
* `trustworthiness`, `continuity`, `map_quality`, `placement_quality`, `LatentMap.quality`: how far a map can be believed, by
  sklearn's `trustworthiness` both ways round, at any number of rows (csrc/map_quality.hip ranks the neighbours of one space
  among all rows of the other without forming a distance matrix); `kneighbors` is the exact neighbour search they share.

Out of scope: numerical parity with openTSNE, Barnes-Hut / FFT approximations, 3-D maps, plots."""
from __future__ import annotations

import numpy as np
import torch

from .pipeline import _need_cuda

_N_ITER_CHECK = 50
_EXPLORATION_MAX_ITER = 250


def _rows(x, what):
    _need_cuda(x, what)
    if x.dim() != 2 or x.dtype != torch.float32:
        raise TypeError(f"{what}: expected a (N, E) fp32 tensor, got {tuple(x.shape)} {x.dtype}")
    return x if x.stride(1) == 1 else x.contiguous()


def _pitch4(x):
    """the rows on a 16-byte aligned pitch of a multiple of 4 floats (a view of a zero-filled copy where they are not): layout only"""
    if x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0:
        return x
    wide = torch.zeros((x.shape[0], (x.shape[1] + 3) & ~3), dtype=torch.float32, device=x.device)
    wide[:, :x.shape[1]] = x
    return wide[:, :x.shape[1]]


def _rng(random_state):
    return random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(random_state)


class PCA:
    """`fit` / `transform` / `fit_transform` over (N, E) fp32 GPU rows; `mean_`, `components_` (k, E), `explained_variance_`,
    `explained_variance_ratio_` as float64 numpy, each component signed so that its largest-magnitude entry is positive (sklearn's
    svd_flip on V).  A streamed set takes one `update` per batch and then `fit()`.  As the reference does inside its `try`, data
    with fewer than `n_components` rows or columns is passed through unchanged (`components_` stays None).  Pickles without device
    state."""

    def __init__(self, n_components=50):
        if int(n_components) < 1:
            raise ValueError("PCA: n_components must be positive")
        self.n_components = int(n_components)
        self.mean_ = self.components_ = self.explained_variance_ = self.explained_variance_ratio_ = None
        self.n_samples_ = 0
        self._mom = None
        self._dev = {}                 # device -> (weights (k, E), bias (k,)); never pickled

    def __getstate__(self):
        state = dict(self.__dict__)
        state["_mom"], state["_dev"] = None, {}
        return state

    def update(self, rows: torch.Tensor) -> "PCA":
        from .metrics import LatentMoments
        rows = _rows(rows, "PCA.update")
        if self._mom is None:
            self._mom = LatentMoments(rows.shape[1], rows.device)
        self._mom.update(rows)
        return self

    def fit(self, x: torch.Tensor = None) -> "PCA":
        if x is not None:
            self._mom = None
            self.update(x)
        if self._mom is None:
            raise ValueError("PCA.fit: no rows (pass x, or call update first)")
        self._dev = {}
        n, E = self._mom.n, self._mom.E
        self.n_samples_ = n
        self.mean_ = self.components_ = self.explained_variance_ = self.explained_variance_ratio_ = None
        if min(n, E) < self.n_components:
            return self
        _, mean, cov = self._mom.finalize()
        lam, v = np.linalg.eigh(0.5 * (cov + cov.T))
        lam, v = np.clip(lam[::-1], 0.0, None), v[:, ::-1]
        comp = v[:, :self.n_components].T.copy()
        comp *= np.sign(comp[np.arange(comp.shape[0]), np.abs(comp).argmax(axis=1)])[:, None]
        self.mean_, self.components_ = mean, comp
        self.explained_variance_ = lam[:self.n_components].copy()
        self.explained_variance_ratio_ = self.explained_variance_ / lam.sum()
        return self

    def _project(self, x, scale=1.0):
        """x C^T scale - mean C^T scale as one dense layer; output rows padded to a multiple of 4 floats (a view is returned)"""
        from . import ops
        k = self.components_.shape[0]
        key = (str(x.device), float(scale))
        if key not in self._dev:
            w = self.components_ * scale
            self._dev = {key: (torch.from_numpy(w.astype(np.float32)).to(x.device).contiguous(),
                               torch.from_numpy((-(w @ self.mean_)).astype(np.float32)).to(x.device).contiguous())}
        w, b = self._dev[key]
        ldy = (k + 3) & ~3
        out = torch.zeros((x.shape[0], ldy), dtype=torch.float32, device=x.device)
        ops.linear_fwd(x, w, b, M=x.shape[0], ldx=int(x.stride(0)), out=out, ldy=ldy)
        return out[:, :k]

    def transform(self, x: torch.Tensor) -> torch.Tensor:
        x = _rows(x, "PCA.transform")
        if self.n_samples_ == 0:
            raise ValueError("PCA.transform: not fitted")
        if self.components_ is None:
            return x
        if x.shape[1] != self.components_.shape[1]:
            raise ValueError(f"PCA.transform: rows must have {self.components_.shape[1]} columns, got {x.shape[1]}")
        return self._project(x)

    def fit_transform(self, x: torch.Tensor) -> torch.Tensor:
        return self.fit(x).transform(x)


class TSNE:
    """Exact t-SNE of (N, d) fp32 GPU rows into the plane with sklearn's schedule: 250 exploration iterations at momentum 0.5 with
    `early_exaggeration`, then momentum 0.8; velocity and gains start afresh in each phase; `learning_rate="auto"` is
    max(N / early_exaggeration / 4, 50); the two stop rules (no progress of the KL divergence for `n_iter_without_progress`
    iterations, gradient norm <= `min_grad_norm`) are looked at every 50 iterations.  `init`: "pca" (the first two principal
    scores, scaled to a standard deviation of 1e-4 in column 0), "random" (1e-4 * RandomState(random_state).standard_normal((N, 2)))
    or an (N, 2) array.  After `fit`: `embedding_` (N, 2) fp32 on the device, `kl_divergence_`, `n_iter_`, `learning_rate_`, and
    `fit_rows_`, the rows it was given (on the device; `transform` measures new rows against them)."""

    def __init__(self, n_components=2, perplexity=30.0, early_exaggeration=12.0, learning_rate="auto", max_iter=1000,
                 n_iter_without_progress=300, min_grad_norm=1e-7, init="pca", random_state=None, method="exact"):
        if int(n_components) != 2:
            raise ValueError(f"TSNE: only n_components == 2 is built (got {n_components})")
        if method != "exact":
            raise ValueError(f"TSNE: only method == 'exact' is built (got {method!r})")
        if not float(perplexity) > 0.0:
            raise ValueError("TSNE: perplexity must be positive")
        if not float(early_exaggeration) >= 1.0:
            raise ValueError("TSNE: early_exaggeration must be at least 1")
        if not (learning_rate == "auto" or (not isinstance(learning_rate, str) and float(learning_rate) > 0.0)):
            raise ValueError("TSNE: learning_rate must be 'auto' or a positive number")
        if int(max_iter) < _EXPLORATION_MAX_ITER:
            raise ValueError(f"TSNE: max_iter must be at least {_EXPLORATION_MAX_ITER}")
        if isinstance(init, str) and init not in ("pca", "random"):
            raise ValueError(f"TSNE: init must be 'pca', 'random' or an (N, 2) array (got {init!r})")
        self.n_components = 2
        self.perplexity = float(perplexity)
        self.early_exaggeration = float(early_exaggeration)
        self.learning_rate = learning_rate
        self.max_iter = int(max_iter)
        self.n_iter_without_progress = int(n_iter_without_progress)
        self.min_grad_norm = float(min_grad_norm)
        self.init = init
        self.random_state = random_state
        self.method = method
        self.embedding_ = self.kl_divergence_ = self.n_iter_ = self.learning_rate_ = None
        self.fit_rows_ = self.transform_kl_ = None

    def __getstate__(self):
        state = dict(self.__dict__)
        for name in ("embedding_", "fit_rows_", "transform_kl_"):
            if torch.is_tensor(state.get(name)):
                state[name] = state[name].cpu()
        return state

    def _initial(self, x, N):
        if isinstance(self.init, str) and self.init == "pca":
            if x.shape[1] < 2:
                raise ValueError("TSNE: init='pca' needs rows of at least 2 columns")
            pca = PCA(2).fit(x)
            std0 = float(np.sqrt(pca.explained_variance_[0] * (N - 1) / N))     # np.std of the first score
            if not std0 > 0.0:
                raise ValueError("TSNE: init='pca' on rows without variance")
            return pca._project(x, 1e-4 / std0).contiguous()
        if isinstance(self.init, str):
            y = 1e-4 * _rng(self.random_state).standard_normal(size=(N, 2))
        else:
            y = np.asarray(self.init.detach().cpu() if torch.is_tensor(self.init) else self.init)
            if y.shape != (N, 2):
                raise ValueError(f"TSNE: init must be ({N}, 2), got {y.shape}")
        return torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)).to(x.device)

    def _descent(self, P, y, it, max_iter, n_iter_without_progress, momentum, exaggeration, bufs):
        """sklearn's _gradient_descent: -> (last KL read, last iteration)"""
        from . import ops
        grad, out, gnorm2 = bufs
        velocity, gains = torch.zeros_like(y), torch.ones_like(y)
        error = best_error = np.finfo(float).max
        best_iter = i = it
        for i in range(it, max_iter):
            check = (i + 1) % _N_ITER_CHECK == 0
            want_kl = check or i == max_iter - 1
            ops.tsne_gradient(P, y, exaggeration, want_kl, grad=grad, out=out)
            ops.tsne_update(y, velocity, gains, grad, momentum, self.learning_rate_, gnorm2 if check else None)
            if want_kl:
                error = float(out[0].item())
            if check:
                if error < best_error:
                    best_error, best_iter = error, i
                elif i - best_iter > n_iter_without_progress:
                    break
                if float(np.sqrt(gnorm2.item())) <= self.min_grad_norm:
                    break
        return error, i

    @torch.no_grad()
    def fit(self, x: torch.Tensor, y=None) -> "TSNE":
        from . import ops
        x = _rows(x, "TSNE.fit")
        N = x.shape[0]
        if self.perplexity >= N:
            raise ValueError(f"perplexity ({self.perplexity}) must be less than n_samples ({N})")
        if N > ops.tsne_max_rows():
            raise ValueError(f"TSNE: {N} rows; the exact method holds the dense N x N joint and is built for at most "
                             f"{ops.tsne_max_rows()} rows: map a sub-sample (latent_map(..., sample_size=M))")
        if x.stride(0) % 4 != 0:                                   # rows on a 16-byte pitch: layout only
            wide = torch.zeros((N, (x.shape[1] + 3) & ~3), dtype=torch.float32, device=x.device)
            wide[:, :x.shape[1]] = x
            x = wide[:, :x.shape[1]]
        self.learning_rate_ = (max(N / self.early_exaggeration / 4.0, 50.0) if isinstance(self.learning_rate, str)
                               else float(self.learning_rate))
        emb = self._initial(x, N)
        P = ops.tsne_affinities(x, self.perplexity)
        bufs = (torch.empty_like(emb), torch.empty((3,), dtype=torch.float64, device=x.device),
                torch.empty((1,), dtype=torch.float64, device=x.device))
        kl, it = self._descent(P, emb, 0, _EXPLORATION_MAX_ITER, _EXPLORATION_MAX_ITER, 0.5, self.early_exaggeration, bufs)
        if it < _EXPLORATION_MAX_ITER or self.max_iter - _EXPLORATION_MAX_ITER > 0:
            kl, it = self._descent(P, emb, it + 1, self.max_iter, self.n_iter_without_progress, 0.8, 1.0, bufs)
        self.embedding_, self.kl_divergence_, self.n_iter_ = emb, kl, it
        self.fit_rows_, self.transform_kl_ = x, None
        return self

    def fit_transform(self, x: torch.Tensor, y=None) -> torch.Tensor:
        return self.fit(x).embedding_

    @torch.no_grad()
    def transform(self, x: torch.Tensor, perplexity=5, initialization="median", k=25, learning_rate=0.1, exaggeration=1.5,
                  n_iter=250, momentum=0.8, max_grad_norm=0.25, batch_rows=262144) -> torch.Tensor:
        """Places the rows of x (M, d) into the fitted map -> (M, 2) fp32 on the device; `embedding_` does not move and the rows do
        not interact, so each row's result is the same bits whatever else is in x (openTSNE's `transform` defaults).
        The `max(k_aff, k)` nearest fitted rows are found exactly, `k_aff = min(N - 1, floor(3 perplexity))` of them carry the
        conditionals; `initialization`: "median" of the map over the `k` nearest, "weighted" by the conditionals, or an (M, 2)
        array.  `transform_kl_` receives the per-row KL divergence (float64, on the device).  `batch_rows` bounds the rows per
        kernel call (memory only)."""
        from . import ops
        if self.embedding_ is None or self.fit_rows_ is None:
            raise ValueError("TSNE.transform: not fitted")
        N, d = self.fit_rows_.shape
        if not torch.is_tensor(x) or x.dim() != 2 or x.shape[1] != d:
            raise ValueError(f"TSNE.transform: rows must have {d} columns, got {tuple(getattr(x, 'shape', ()))}")
        M, k = x.shape[0], int(k)
        k_aff = min(N - 1, int(3.0 * float(perplexity)))
        if not 0.0 < float(perplexity) < k_aff:
            raise ValueError(f"TSNE.transform: perplexity ({perplexity}) must be positive and less than the number of neighbours "
                             f"that carry the conditionals, k_aff = min(N - 1, floor(3 perplexity)) = {k_aff}")
        if not 1 <= k <= min(N, 128):
            raise ValueError(f"TSNE.transform: k ({k}) must be in [1, min(N, 128) = {min(N, 128)}]")
        if k_aff > 128:
            raise ValueError(f"TSNE.transform: k_aff = {k_aff} neighbours; the kernels keep at most 128 (perplexity < 43)")
        y0 = None
        if isinstance(initialization, str):
            if initialization not in ("median", "weighted"):
                raise ValueError(f"TSNE.transform: initialization must be 'median', 'weighted' or an (M, 2) array "
                                 f"(got {initialization!r})")
        else:
            y0 = initialization.detach() if torch.is_tensor(initialization) else torch.from_numpy(np.asarray(initialization))
            if tuple(y0.shape) != (M, 2):
                raise ValueError(f"TSNE.transform: initialization must be ({M}, 2), got {tuple(y0.shape)}")
        if int(n_iter) < 0 or int(batch_rows) < 1:
            raise ValueError("TSNE.transform: n_iter must not be negative and batch_rows must be positive")
        x = _rows(x, "TSNE.transform")
        dev = x.device
        if self.fit_rows_.device != dev or self.embedding_.device != dev:      # (an unpickled object holds host tensors)
            self.fit_rows_, self.embedding_ = self.fit_rows_.to(dev), self.embedding_.to(dev)
        ref, emb = _pitch4(self.fit_rows_), self.embedding_.contiguous()
        if y0 is not None:
            y0 = y0.to(device=dev, dtype=torch.float32)
        out = torch.empty((M, 2), dtype=torch.float32, device=dev)
        kl = torch.empty((M,), dtype=torch.float64, device=dev)
        kk = max(k_aff, k)
        for s in range(0, M, int(batch_rows)):
            z = _pitch4(x[s:s + int(batch_rows)])
            idx, d2 = ops.tsne_place_neighbors(ref, z, kk)
            p = ops.tsne_place_conditionals(d2, k_aff, perplexity)
            if y0 is not None:
                y = y0[s:s + int(batch_rows)].contiguous().clone()
            else:
                y = ops.tsne_place_init(emb, idx, p, initialization, k if initialization == "median" else k_aff)
            res = ops.tsne_place_descent(emb, idx, p, y, None, None, n_iter, exaggeration, momentum, learning_rate, max_grad_norm,
                                         want=("kl",))
            out[s:s + z.shape[0]] = y
            kl[s:s + z.shape[0]] = res["kl"]
        self.transform_kl_ = kl
        return out


class LatentMap:
    """The reference's `(pca, MyTSNE)` pair as one object: `fit(latents)` runs `PCA(n_pca)` and `TSNE(random_state=random_state,
    **tsne_kw)` on the rows, or on `sample_size` rows drawn exactly as `latent_map` draws them, and sets `coords_` (the fitted map)
    and `rows_` (the fitted rows' indices, int64); `transform(latents, **place_kw)` places further rows (`TSNE.transform` of their
    PCA scores); `fit_all` maps a whole set of any size: the sample exactly, every other row placed against it.  Pickles without
    device state."""

    def __init__(self, n_pca=50, sample_size=None, random_state=None, **tsne_kw):
        self.n_pca, self.sample_size, self.random_state = int(n_pca), sample_size, random_state
        self.pca = PCA(n_pca)
        self.tsne = TSNE(**tsne_kw)
        self.coords_ = self.rows_ = None

    def __getstate__(self):
        state = dict(self.__dict__)
        for name in ("coords_", "rows_"):
            if torch.is_tensor(state[name]):
                state[name] = state[name].cpu()
        return state

    @torch.no_grad()
    def fit(self, latents: torch.Tensor) -> "LatentMap":
        latents = _rows(latents, "LatentMap.fit")
        N = latents.shape[0]
        rs = _rng(self.random_state)
        if self.sample_size is not None:
            idx = torch.from_numpy(rs.permutation(N)[:int(self.sample_size)].astype(np.int64)).to(latents.device)
            latents = latents[idx].contiguous()                    # a gather: layout only
        else:
            idx = torch.arange(N, dtype=torch.int64, device=latents.device)
        self.tsne.random_state = rs
        self.coords_ = self.tsne.fit_transform(self.pca.fit_transform(latents))
        self.tsne.random_state = self.random_state                 # (a RandomState that has been drawn from is not kept)
        self.rows_ = idx
        return self

    @torch.no_grad()
    def transform(self, latents: torch.Tensor, **place_kw) -> torch.Tensor:
        if self.coords_ is None:
            raise ValueError("LatentMap.transform: not fitted")
        return self.tsne.transform(self.pca.transform(_rows(latents, "LatentMap.transform")), **place_kw)

    @torch.no_grad()
    def fit_all(self, latents: torch.Tensor, **place_kw):
        """-> (coords (N, 2) fp32, fitted (N,) bool), in input row order: the fitted rows carry `coords_`, the others are placed"""
        latents = _rows(latents, "LatentMap.fit_all")
        self.fit(latents)
        N = latents.shape[0]
        fitted = torch.zeros((N,), dtype=torch.bool, device=latents.device)
        fitted[self.rows_] = True
        coords = torch.empty((N, 2), dtype=torch.float32, device=latents.device)
        coords[self.rows_] = self.coords_
        rest = (~fitted).nonzero().flatten()
        if rest.numel():
            coords[rest] = self.transform(latents[rest].contiguous(), **place_kw)
        return coords, fitted


    @torch.no_grad()
    def quality(self, latents: torch.Tensor, coords: torch.Tensor, sample_idx=None, **kw) -> dict:
        """How faithful is the map `coords` (N, 2) of `latents` (N, E), as `fit_all` returns it?  -> {"fitted": `map_quality` of the
        rows `sample_idx` (default `rows_`, the rows the map was fitted on), "placed": `placement_quality` of every other row
        against them, or None where there is none}, each with `rows`: the rows of `latents` its penalties belong to, in their
        order.  The high-dimensional space is the one the map was made from: the PCA scores.  `kw`: n_neighbors."""
        if self.coords_ is None:
            raise ValueError("LatentMap.quality: not fitted")
        latents, coords = _rows(latents, "LatentMap.quality"), _rows(coords, "LatentMap.quality")
        N = latents.shape[0]
        if tuple(coords.shape) != (N, 2):
            raise ValueError(f"LatentMap.quality: coords must be ({N}, 2), got {tuple(coords.shape)}")
        idx = self.rows_ if sample_idx is None else torch.as_tensor(sample_idx, dtype=torch.int64)
        idx = idx.to(latents.device)
        scores = self.pca.transform(latents)
        placed = torch.ones((N,), dtype=torch.bool, device=latents.device)
        placed[idx] = False
        rest = placed.nonzero().flatten()
        # (the rows the map was fitted on are kept: the very bits its neighbours were taken from)
        xs = self.tsne.fit_rows_.to(latents.device) if sample_idx is None else scores[idx].contiguous()
        ys = coords[idx].contiguous()
        out = {"fitted": dict(map_quality(xs, ys, **kw), rows=idx), "placed": None}
        if rest.numel():
            out["placed"] = dict(placement_quality(xs, ys, scores[rest].contiguous(), coords[rest].contiguous(), **kw), rows=rest)
        return out


# ---- how faithful a map is: trustworthiness and continuity (csrc/map_quality.hip) ---------------------------------------------------
# sklearn.manifold.trustworthiness (sklearn 1.7, Euclidean) without its two N x N float64 matrices and their argsorts: the k nearest
# other rows in one space (ops.tsne_place_neighbors, exact, never storing the distances) are ranked among all rows of the other
# space (ops.neighbor_ranks).  With r_X(i, j) the rank of j among the rows other than i by ascending X-distance to i (nearest: 1,
# ties to the lower index) and N_k^Y(i) the k nearest other rows of i in the map:
#   p_T(i) = sum_{j in N_k^Y(i)} max(0, r_X(i, j) - k)        trustworthiness = 1 - 2 / (N k (2 N - 3 k - 1)) sum_i p_T(i)
# continuity is the same with X and Y swapped.  The penalties are integers and are summed as int64 on the device.
_MAX_K = 127


def _check_k(what, n_neighbors, N, half=True):
    k = int(n_neighbors)
    if k != n_neighbors or k < 1:
        raise ValueError(f"{what}: n_neighbors must be a positive integer, got {n_neighbors!r}")
    if half and k >= N / 2:
        raise ValueError(f"{what}: n_neighbors ({k}) should be less than n_samples / 2 ({N / 2})")
    if k > _MAX_K:
        raise ValueError(f"{what}: n_neighbors ({k}) exceeds {_MAX_K}, the most the kernels rank per row")
    return k


def _pair(X, Y, what):
    if not torch.is_tensor(X) or not torch.is_tensor(Y) or X.dim() != 2 or Y.dim() != 2 or X.shape[0] != Y.shape[0]:
        raise ValueError(f"{what}: X (N, d) and Y (N, c) must be tensors with the same number of rows")
    return X.shape[0]


def _score(total, rows, N, k):
    """sklearn's closing expression, in float64, from the integer sum of the penalties"""
    return 1.0 - float(total) * (2.0 / (rows * k * (2.0 * N - 3.0 * k - 1.0)))


@torch.no_grad()
def kneighbors(x: torch.Tensor, k, queries=None, return_distance=True):
    """The k nearest rows of x (N, d) under ascending (d^2, index), exactly (ops.tsne_place_neighbors: the distances are selected
    from as they are formed and never stored) -> (distances (M, k) fp32, indices (M, k) int32) on the device, or the indices alone.
    `queries` (M, d): the neighbours of those rows among x.  Without it every row of x is asked for its k nearest OTHER rows: k + 1
    are found and the row itself is taken out; where it is not among them (more than k bitwise duplicates with lower indices
    precede it) the last entry is.  Distances are the square roots of the correctly rounded d^2.  k <= 127."""
    from . import ops
    x = _rows(x, "kneighbors")
    N, k = x.shape[0], int(k)
    own = queries is None
    if not 1 <= k <= min(N - 1 if own else N, _MAX_K):
        raise ValueError(f"kneighbors: k ({k}) must be in [1, min({'N - 1' if own else 'N'}, {_MAX_K})] (N = {N})")
    ref = _pitch4(x)
    if own:
        idx, d2 = ops.tsne_place_neighbors(ref, ref, k + 1)
        me = torch.arange(N, dtype=torch.int32, device=x.device)[:, None]
        hit = idx == me
        drop = torch.where(hit.any(dim=1), hit.to(torch.int8).argmax(dim=1), torch.full_like(hit[:, 0], k, dtype=torch.int64))
        keep = torch.arange(k + 1, device=x.device)[None, :] != drop[:, None]
        idx, d2 = idx[keep].view(N, k), d2[keep].view(N, k)
    else:
        q = _rows(queries, "kneighbors")
        if q.shape[1] != x.shape[1]:
            raise ValueError(f"kneighbors: x has {x.shape[1]} columns and queries {q.shape[1]}")
        idx, d2 = ops.tsne_place_neighbors(ref, _pitch4(q), k)
    return (d2.sqrt(), idx) if return_distance else idx


def _penalties(rank_space, pick_space, k):
    """-> (penalty (N,) int64, redecided (1,) int64): neighbours picked in one space, ranked in the other, over the same rows"""
    from . import ops
    idx = kneighbors(pick_space, k, return_distance=False)
    rows = _pitch4(rank_space)
    me = torch.arange(rows.shape[0], dtype=torch.int64, device=rows.device)
    rank, redo = ops.neighbor_ranks(rows, rows, idx, me)
    return (rank.to(torch.int64) - k).clamp_(min=0).sum(dim=1), redo


def _placed_penalties(rank_ref, rank_new, pick_ref, pick_new, k):
    """the same for new rows against a fitted set: picked among pick_ref, ranked among rank_ref, no row left out"""
    from . import ops
    idx = kneighbors(pick_ref, k, queries=pick_new, return_distance=False)
    rank, redo = ops.neighbor_ranks(_pitch4(rank_ref), _pitch4(rank_new), idx, None)
    return (rank.to(torch.int64) - k).clamp_(min=0).sum(dim=1), redo


def _quality(pen_t, redo_t, pen_c, redo_c, rows, N, k):
    sums = torch.stack([pen_t.sum(), pen_c.sum(), (redo_t + redo_c)[0]]).cpu().numpy()       # the one read-back
    return {"trustworthiness": _score(int(sums[0]), rows, N, k), "continuity": _score(int(sums[1]), rows, N, k),
            "penalty_t": pen_t, "penalty_c": pen_c, "n_neighbors": k, "redecided": int(sums[2])}


@torch.no_grad()
def map_quality(X: torch.Tensor, Y: torch.Tensor, n_neighbors=5, sample_size=None, random_state=None) -> dict:
    """Both scores of the map Y (N, c) of the rows X (N, d), fp32 on the device -> {"trustworthiness", "continuity" (floats),
    "penalty_t", "penalty_c" ((N,) int64 on the device: each row's share, so the badly mapped rows can be found), "n_neighbors",
    "redecided" (the pairs the kernel decided again in float64)}.  `sample_size` / `random_state` score the sub-map of the rows
    `RandomState(random_state).permutation(N)[:sample_size]`, as `silhouette_score` draws them."""
    N = _pair(X, Y, "map_quality")
    if sample_size is not None:
        N = min(N, int(sample_size))
    k = _check_k("map_quality", n_neighbors, N)
    X, Y = _rows(X, "map_quality"), _rows(Y, "map_quality")
    if sample_size is not None:
        idx = torch.from_numpy(_rng(random_state).permutation(X.shape[0])[:int(sample_size)].astype(np.int64)).to(X.device)
        X, Y = X[idx].contiguous(), Y[idx].contiguous()            # a gather: layout only
    pen_t, redo_t = _penalties(X, Y, k)
    pen_c, redo_c = _penalties(Y, X, k)
    return _quality(pen_t, redo_t, pen_c, redo_c, N, N, k)


@torch.no_grad()
def trustworthiness(X: torch.Tensor, Y: torch.Tensor, *, n_neighbors=5, metric="euclidean") -> float:
    """`sklearn.manifold.trustworthiness(X, X_embedded, n_neighbors=5, metric="euclidean")` for fp32 rows on the device: to what
    extent the map's neighbourhoods are neighbourhoods of X."""
    if metric != "euclidean":
        raise ValueError(f"trustworthiness: metric must be 'euclidean', got {metric!r}")
    N = _pair(X, Y, "trustworthiness")
    k = _check_k("trustworthiness", n_neighbors, N)
    pen, _ = _penalties(_rows(X, "trustworthiness"), _rows(Y, "trustworthiness"), k)
    return _score(int(pen.sum().item()), N, N, k)


@torch.no_grad()
def continuity(X: torch.Tensor, Y: torch.Tensor, *, n_neighbors=5) -> float:
    """Trustworthiness the other way round: to what extent the neighbourhoods of X stay neighbourhoods in the map."""
    N = _pair(X, Y, "continuity")
    k = _check_k("continuity", n_neighbors, N)
    pen, _ = _penalties(_rows(Y, "continuity"), _rows(X, "continuity"), k)
    return _score(int(pen.sum().item()), N, N, k)


@torch.no_grad()
def placement_quality(X_ref: torch.Tensor, Y_ref: torch.Tensor, Z: torch.Tensor, y: torch.Tensor, n_neighbors=5) -> dict:
    """The same two scores for M rows Z (M, d) placed at y (M, c) against a fitted set X_ref (N, d) with the map Y_ref (N, c)
    (`TSNE.transform`): every neighbour and every rank is among the N fitted rows, none is left out, and the sums are normalised by
    M k (2 N - 3 k - 1) / 2.  Trustworthiness: the map-neighbours of y among Y_ref, ranked by distance from Z among X_ref;
    continuity the other way round.  -> the dict of `map_quality`, the penalties (M,)."""
    N, M = _pair(X_ref, Y_ref, "placement_quality"), _pair(Z, y, "placement_quality")
    k = _check_k("placement_quality", n_neighbors, N)
    X_ref, Y_ref, Z, y = (_rows(t, "placement_quality") for t in (X_ref, Y_ref, Z, y))
    if Z.shape[1] != X_ref.shape[1] or y.shape[1] != Y_ref.shape[1]:
        raise ValueError("placement_quality: Z must have the columns of X_ref and y those of Y_ref")
    pen_t, redo_t = _placed_penalties(X_ref, Z, Y_ref, y, k)
    pen_c, redo_c = _placed_penalties(Y_ref, y, X_ref, Z, k)
    return _quality(pen_t, redo_t, pen_c, redo_c, M, N, k)


@torch.no_grad()
def latent_map(latents: torch.Tensor, n_pca=50, sample_size=None, random_state=None, **tsne_kw):
    """(N, E) fp32 GPU latent rows -> (coords (M, 2) fp32, row indices (M,) int64), both on the device: `PCA(n_pca)` (skipped for
    fewer than n_pca rows or columns, as in the reference) and then `TSNE(random_state=random_state, **tsne_kw)`.  `sample_size`
    rows are drawn as `silhouette_score` draws them: `numpy.random.RandomState(random_state).permutation(N)[:sample_size]`."""
    latents = _rows(latents, "latent_map")
    N = latents.shape[0]
    rs = _rng(random_state)
    if sample_size is not None:
        idx = torch.from_numpy(rs.permutation(N)[:int(sample_size)].astype(np.int64)).to(latents.device)
        latents = latents[idx].contiguous()                        # a gather: layout only
    else:
        idx = torch.arange(N, dtype=torch.int64, device=latents.device)
    rows = PCA(n_pca).fit_transform(latents)
    return TSNE(random_state=rs, **tsne_kw).fit_transform(rows), idx


@torch.no_grad()
def codebook_map(net, n_pca=50, **tsne_kw) -> torch.Tensor:
    """The (K, 2) map of the quantiser's codebook, `net.vq_layer._embedding.weight`."""
    if not getattr(net, "vq", True) or getattr(net, "vq_layer", None) is None:
        raise ValueError("codebook_map: this autoencoder has no quantiser (autoencoder_vq == 'False'), so there is no codebook")
    return latent_map(net.vq_layer._embedding.weight.detach().float(), n_pca=n_pca, **tsne_kw)[0]
