"""DTW k-means over chunk sequences on the device: the reference's `TimeSeriesKMeans(n_clusters=40, metric="dtw", max_iter=5,
max_iter_barycenter=5, random_state=0)` of tslearn over `latent_linear`, the `(n_poses, F)` frame latents of every chunk
(`Clustering.py:629-669`), so that two executions of one gesture at different speeds land in one cluster.

tslearn is not imported and is no dependency: **parity with tslearn is claimed from its definition only**, not from a recorded run
of it.  The algorithm is stated in include/g2v.h (the DTW block) and tested against a float64 restatement (tests/_dtw_ref.py).

    dtw_cdist(x, y)     (N, M) float64 DTW distances between GPU series (ops.dtw_cdist, csrc/dtw.hip)
    TimeSeriesKMeans    fit / fit_predict / predict / predict_device / from_centers

The loop, which is tslearn's as read from its source.  Centres start as the init rows.  For `it` in `range(max_iter)`:
    assign    labels = argmin over the centres of dtw^2, inertia = the mean of the minimal dtw^2 (ops.dtw_cdist)
    an empty cluster raises (array init) or redraws the init rows (`init="random"`, at most 10 draws per init)
    update    up to `max_iter_barycenter` DBA steps per cluster from its current centre (ops.dtw_dba_accumulate + ops.dtw_dba_update):
              every path cell (i, j) of a member adds the member's row j to the sum of centre row i; the centre becomes sums / counts;
              a cluster stops when its mean dtw^2 to its members moved by less than `barycenter_tol`, or rose.  The rule is decided
              on the device per cluster, so all steps are enqueued without a read-back
    stop after the update if |old_inertia - inertia| < tol
`n_iter_ = it + 1`; `labels_` and `inertia_` are those of the last assignment, that is, of the centres before the last update;
`predict` uses the final centres.  Everything is float64 on the device: path decisions have margins down to 4e-7 relative on the
test inputs, which fp32 would flip.

`init="random"` draws `RandomState(seed).permutation(N)[:K]` as `KMeans` here does, which is not tslearn's draw.  Refused by name:
`metric="euclidean"` (that is `KMeans` on the flattened rows) and `"softdtw"` (that is `SoftDTWKMeans` below), `init="k-means++"`
(tslearn's seeding under DTW), `metric_params` (a Sakoe-Chiba band), `dtw_inertia`, sample weights, and series of unequal length
within one array.

Soft-DTW (Cuturi & Blondel 2017; the reference's `TimeSeriesKMeans(n_clusters=40, metric="softdtw", max_iter=5,
max_iter_barycenter=5, metric_params={"gamma": 0.5}, random_state=0)`, `Clustering.py:670-691`), stated in the soft-DTW block of
include/g2v.h and tested against tests/_softdtw_ref.py, again from tslearn's definition only:

    soft_dtw_cdist(x, y, gamma)        (N, M) float64 soft-DTW values (ops.softdtw_cdist, csrc/softdtw.hip)
    soft_dtw_alignment(x_row, z, gamma) the soft alignment matrix E (S, T) and the value (ops.softdtw_alignment)
    softdtw_barycenter(X, gamma, ...)  scipy's L-BFGS-B on the host, value and gradient from the device (ops.softdtw_grad)
    SoftDTWKMeans                      the surface of TimeSeriesKMeans; the reference's call with only the class name changed

Its loop is the one above with soft-DTW values in the assignment (inertia = their mean over the rows' best centres, which can be
negative) and, as update, `softdtw_barycenter(members, gamma, max_iter=max_iter_barycenter, init=the current centre)` per cluster,
one cluster after another.  Refused by name there: bands in `metric_params`, `init="k-means++"`, sample weights, unequal lengths."""
from __future__ import annotations

import numpy as np
import torch

from .kmeans import _code_perplexity
from .pipeline import _need_cuda

MAX_REDRAWS = 10           # draws of the init rows per init before an empty cluster raises


class EmptyClusterError(ValueError):
    pass


def _series(x, what, device=None):
    """-> contiguous (N, T, F) fp32 GPU tensor; a list of arrays of unequal length is refused by name"""
    if isinstance(x, (list, tuple)):
        shapes = {tuple(np.shape(r)) for r in x}
        if len(shapes) > 1:
            raise NotImplementedError(f"{what}: series of unequal length within one array are not supported (got shapes {sorted(shapes)})")
        x = np.asarray(x, dtype=np.float32)
    if not torch.is_tensor(x):
        a = np.asarray(x)
        if a.dtype == object:
            raise NotImplementedError(f"{what}: series of unequal length within one array are not supported")
        if device is None:
            raise TypeError(f"{what}: expected a GPU tensor, got {type(x).__name__}")
        x = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)
    elif device is not None and not x.is_cuda:
        x = x.to(device)
    _need_cuda(x, what)
    if x.dim() != 3 or x.dtype != torch.float32:
        raise TypeError(f"{what}: expected a (N, T, F) fp32 tensor, got {tuple(x.shape)} {x.dtype}")
    return x.contiguous()


@torch.no_grad()
def dtw_cdist(x: torch.Tensor, y: torch.Tensor = None, squared: bool = False) -> torch.Tensor:
    """DTW distances between GPU series x (N, T, F) fp32 and y (M, S, F) fp32 or float64 (None: x against itself) -> (N, M)
    float64 on the device: sqrt of the minimal accumulated squared difference over all warping paths, or that minimum itself with
    squared=True.  tslearn's `cdist_dtw` by definition (no run of it stands behind this)."""
    from . import ops
    x = _series(x, "dtw_cdist")
    if y is None:
        y = x
    _need_cuda(y, "dtw_cdist")
    if y.dim() != 3 or y.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"dtw_cdist: y must be a (M, S, F) fp32 or float64 tensor, got {tuple(y.shape)} {y.dtype}")
    return ops.dtw_cdist(x, y.to(torch.float64).contiguous(), squared=squared)[0]


class _SeriesKMeans:
    """What the two time-series k-means classes share: the state, from_centers, pickling, the fit loop with its redraws, predict.
    A subclass supplies `_assign(x, centers) -> (labels, best)` and `_barycenters(x, labels, members, centers)` (in place)."""

    def _start(self, n_clusters, max_iter, tol, n_init, max_iter_barycenter, random_state, init):
        name = type(self).__name__
        if isinstance(init, str):
            if init == "k-means++":
                raise NotImplementedError(f"{name}: init='k-means++' (tslearn's seeding under DTW) is not supported; "
                                          "use 'random' or a (K, S, F) array")
            if init != "random":
                raise ValueError(f"{name}: unknown init {init!r}")
        if int(n_clusters) < 1 or int(max_iter) < 1 or int(n_init) < 1 or int(max_iter_barycenter) < 1:
            raise ValueError(f"{name}: n_clusters, max_iter, n_init and max_iter_barycenter must be positive")
        self.n_clusters = int(n_clusters)
        self.max_iter = int(max_iter)
        self.tol = float(tol)
        self.n_init = int(n_init)
        self.max_iter_barycenter = int(max_iter_barycenter)
        self.random_state = random_state
        self.init = init
        self.cluster_centers_ = None       # (K, S, F) float64 numpy
        self.labels_ = None                # (N) int32 numpy
        self.inertia_ = None
        self.n_iter_ = None
        self.init_rows_ = None             # rows the last `init="random"` chose
        self._dev = {}                     # device -> centres; never pickled

    # ---- construction / pickling ------------------------------------------------------------------------------------------------
    @classmethod
    def from_centers(cls, centers, **keywords):
        """A fitted model around given (K, S, F) centres"""
        c = np.ascontiguousarray(np.asarray(centers.detach().cpu() if torch.is_tensor(centers) else centers, dtype=np.float64))
        if c.ndim != 3 or c.shape[0] < 1:
            raise ValueError(f"from_centers: expected a (K, S, F) array, got shape {c.shape}")
        km = cls(n_clusters=c.shape[0], **keywords)
        km.cluster_centers_ = c
        return km

    def __getstate__(self):
        d = dict(self.__dict__)
        d["_dev"] = {}
        if not isinstance(d["init"], str):
            d["init"] = np.asarray(d["init"].detach().cpu() if torch.is_tensor(d["init"]) else d["init"])
        return d

    # ---- fit ----------------------------------------------------------------------------------------------------------------------
    def _init_centers(self, x, rs):
        N, T, F = x.shape
        K = self.n_clusters
        if isinstance(self.init, str):
            self.init_rows_ = [int(i) for i in rs.permutation(N)[:K]]
            return x[torch.tensor(self.init_rows_, dtype=torch.int64, device=x.device)].to(torch.float64).contiguous()
        c = self.init.detach() if torch.is_tensor(self.init) else torch.from_numpy(np.asarray(self.init, dtype=np.float64))
        if c.dim() != 3 or c.shape[0] != K or c.shape[2] != F:
            raise ValueError(f"{type(self).__name__}: init must have shape ({K}, S, {F}), got {tuple(c.shape)}")
        return c.to(device=x.device, dtype=torch.float64).contiguous().clone()

    def _fit_one(self, x, centers):
        K = self.n_clusters
        old = float("inf")
        for it in range(self.max_iter):
            labels, best = self._assign(x, centers)
            members = torch.bincount(labels, minlength=K)
            inertia = float(best.cpu().numpy().mean())
            empty = np.flatnonzero(members.cpu().numpy() == 0)
            if empty.size:
                raise EmptyClusterError(f"{type(self).__name__}: cluster {int(empty[0])} is empty after the assignment of iteration {it}"
                                        f" ({empty.size} of {K} clusters are)")
            self._barycenters(x, labels, members, centers)
            if abs(old - inertia) < self.tol:
                break
            old = inertia
        return centers, labels, inertia, it + 1

    @torch.no_grad()
    def fit(self, X, y=None, sample_weight=None):
        """X: (N, T, F) fp32 GPU tensor, 1 <= T <= ops.dtw_max_len(), 1 <= F <= 512"""
        if sample_weight is not None:
            raise NotImplementedError(f"{type(self).__name__}.fit: sample weights are not supported")
        x = _series(X, f"{type(self).__name__}.fit")
        N = x.shape[0]
        K = self.n_clusters
        if K > N:
            raise ValueError(f"{type(self).__name__}: n_clusters = {K} exceeds the {N} series")
        if not bool(torch.isfinite(x).all()):
            raise ValueError(f"{type(self).__name__}.fit: the series contain NaN or infinity")
        rs = self.random_state if isinstance(self.random_state, np.random.RandomState) else np.random.RandomState(self.random_state)
        random_init = isinstance(self.init, str)
        best = None
        for _ in range(self.n_init if random_init else 1):
            for draw in range(MAX_REDRAWS):
                try:
                    run = self._fit_one(x, self._init_centers(x, rs))
                    break
                except EmptyClusterError:
                    if not random_init or draw == MAX_REDRAWS - 1:
                        raise
            rows = self.init_rows_
            if best is None or run[2] < best[0][2]:
                best = (run, rows)
        (centers, labels, inertia, n_iter, *extra), self.init_rows_ = best
        self._keep(*extra)
        self.cluster_centers_ = centers.cpu().numpy()
        self.labels_ = labels.cpu().numpy().astype(np.int32)
        self.inertia_, self.n_iter_ = inertia, n_iter
        self._dev = {str(x.device): centers}
        return self

    def _keep(self):
        """what a subclass's _fit_one returned beyond (centres, labels, inertia, n_iter), of the run that was kept"""

    def fit_predict(self, X, y=None) -> np.ndarray:
        return self.fit(X).labels_

    # ---- predict ------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def predict_device(self, X: torch.Tensor) -> torch.Tensor:
        """(N, T, F) fp32 GPU series of any length T <= ops.dtw_max_len() -> (N,) int64 GPU ids: the argmin of the class's distance
        over the final centres, lowest index on ties"""
        if self.cluster_centers_ is None:
            raise RuntimeError(f"{type(self).__name__}: not fitted")
        x = _series(X, f"{type(self).__name__}.predict_device")
        if x.shape[2] != self.cluster_centers_.shape[2]:
            raise ValueError(f"{type(self).__name__}.predict_device: series have {x.shape[2]} columns, the centres {self.cluster_centers_.shape[2]}")
        key = str(x.device)
        if key not in self._dev:
            self._dev[key] = torch.from_numpy(self.cluster_centers_).to(x.device)
        if x.shape[0] == 0:
            return torch.empty((0,), dtype=torch.int64, device=x.device)
        return self._assign(x, self._dev[key])[0]

    def predict(self, X, device="cuda:0") -> np.ndarray:
        """numpy or torch series -> numpy int32 ids (tslearn's `predict`); the work is done on `device`"""
        return self.predict_device(_series(X, f"{type(self).__name__}.predict", device)).cpu().numpy().astype(np.int32)

    def code_perplexity(self) -> float:
        """exp(entropy) of the fitted labels' histogram"""
        return _code_perplexity(np.bincount(self.labels_, minlength=self.n_clusters))


class TimeSeriesKMeans(_SeriesKMeans):
    def __init__(self, n_clusters=3, max_iter=50, tol=1e-6, n_init=1, metric="dtw", max_iter_barycenter=100, barycenter_tol=1e-5,
                 random_state=None, init="random", **refused):
        for name, value in refused.items():
            if name == "metric_params":
                if value is not None:
                    raise NotImplementedError("TimeSeriesKMeans: `metric_params` (a Sakoe-Chiba or Itakura band) is not supported")
            elif name == "dtw_inertia":
                if value:
                    raise NotImplementedError("TimeSeriesKMeans: `dtw_inertia` is not supported (inertia_ is the DTW inertia already)")
            elif name in ("verbose", "n_jobs"):
                pass
            else:
                raise TypeError(f"TimeSeriesKMeans: unexpected argument `{name}`")
        if metric in ("euclidean", "softdtw"):
            raise NotImplementedError(f"TimeSeriesKMeans: metric={metric!r} is not supported, only 'dtw'" +
                                      (" (Euclidean time-series k-means is KMeans on the flattened rows)" if metric == "euclidean"
                                       else " (soft-DTW k-means is SoftDTWKMeans, which takes metric='softdtw' and the same keywords)"))
        if metric != "dtw":
            raise ValueError(f"TimeSeriesKMeans: unknown metric {metric!r}")
        self._start(n_clusters, max_iter, tol, n_init, max_iter_barycenter, random_state, init)
        self.metric = metric
        self.barycenter_tol = float(barycenter_tol)

    def _assign(self, x, centers):
        from . import ops
        return ops.dtw_cdist(x, centers, want_out=False, want_labels=True)[1:]

    def _barycenters(self, x, labels, members, centers):
        """up to max_iter_barycenter DBA steps per cluster, in place on centers, all enqueued at once"""
        from . import ops
        state, _, live = ops.dtw_dba_state(self.n_clusters, x.device)
        acc = None
        for _ in range(self.max_iter_barycenter):
            acc = ops.dtw_dba_accumulate(x, labels, centers, live, out=acc)
            ops.dtw_dba_update(acc, members, state, centers, self.barycenter_tol)


# ---- soft-DTW ------------------------------------------------------------------------------------------------------------------------
def _gamma(gamma, what):
    g = float(gamma)
    if not np.isfinite(g) or g <= 0.0:
        raise ValueError(f"{what}: gamma must be finite and > 0, got {gamma!r}")
    return g


@torch.no_grad()
def soft_dtw_cdist(x: torch.Tensor, y: torch.Tensor = None, gamma: float = 1.0) -> torch.Tensor:
    """Soft-DTW values between GPU series x (N, T, F) fp32 and y (M, S, F) fp32 or float64 (None: x against itself) -> (N, M)
    float64 on the device.  gamma == 0 is `dtw_cdist(squared=True)`, as in tslearn.  tslearn's `cdist_soft_dtw` by definition (no
    run of it stands behind this)."""
    from . import ops
    if float(gamma) == 0.0:
        return dtw_cdist(x, y, squared=True)
    g = _gamma(gamma, "soft_dtw_cdist")
    x = _series(x, "soft_dtw_cdist")
    if y is None:
        y = x
    _need_cuda(y, "soft_dtw_cdist")
    if y.dim() != 3 or y.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"soft_dtw_cdist: y must be a (M, S, F) fp32 or float64 tensor, got {tuple(y.shape)} {y.dtype}")
    return ops.softdtw_cdist(x, y.to(torch.float64).contiguous(), g)[0]


@torch.no_grad()
def soft_dtw_alignment(x_row: torch.Tensor, z: torch.Tensor, gamma: float = 1.0):
    """The soft alignment of one GPU series x_row (T, F) fp32 with z (S, F) fp32 or float64 -> (E (S, T) float64, value): E[i][j]
    is the weight of matching row i of z with row j of x_row, value = sdtw_gamma(z, x_row), both on the device.  x_row (R, T, F)
    gives E (R, S, T) and value (R).  tslearn's `soft_dtw_alignment` by definition."""
    from . import ops
    g = _gamma(gamma, "soft_dtw_alignment")
    _need_cuda(x_row, "soft_dtw_alignment")
    _need_cuda(z, "soft_dtw_alignment")
    one = x_row.dim() == 2
    x = _series(x_row[None] if one else x_row, "soft_dtw_alignment")
    if z.dim() != 2 or z.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"soft_dtw_alignment: z must be a (S, F) fp32 or float64 tensor, got {tuple(z.shape)} {z.dtype}")
    E, value = ops.softdtw_alignment(x, z.to(torch.float64).contiguous(), g)
    return (E[0], value[0]) if one else (E, value)


def _descend(x, rows, weights, start, gamma, max_iter, tol):
    """scipy's L-BFGS-B from `start` (S, F) float64 numpy over the member rows x[rows], value and gradient from the device, one
    launch set and one copy to the host per function evaluation -> (centre (S, F) float64 numpy, function evaluations)"""
    from scipy.optimize import minimize
    from . import ops
    S, F = start.shape
    if max_iter == 0:
        return start.copy(), 0
    z = torch.empty((S, F), dtype=torch.float64, device=x.device)
    out = torch.empty((1 + S * F,), dtype=torch.float64, device=x.device)

    def f(flat):
        z.copy_(torch.from_numpy(flat.reshape(S, F)))
        ops.softdtw_grad(x, rows, z, gamma, weights, out=out)
        host = out.cpu().numpy()
        return float(host[0]), host[1:].copy()

    res = minimize(f, start.ravel(), method="L-BFGS-B", jac=True, tol=tol, options=dict(maxiter=int(max_iter), disp=False))
    return res.x.reshape(S, F), int(res.nfev)


@torch.no_grad()
def softdtw_barycenter(X, gamma=1.0, weights=None, max_iter=50, tol=1e-3, init=None, return_nfev=False, device="cuda:0"):
    """The soft-DTW barycentre of the series X (R, T, F) (a GPU tensor, or numpy: moved to `device`) -> (S, F) float64 numpy, and
    with return_nfev=True the pair (barycentre, function evaluations): scipy's L-BFGS-B on the host over value and gradient from
    the device (ops.softdtw_grad).  weights (R) default to ones and are not normalised; init (S, F) defaults to the weighted
    Euclidean mean.  tslearn's `softdtw_barycenter` by definition."""
    g = _gamma(gamma, "softdtw_barycenter")
    x = _series(X, "softdtw_barycenter", None if torch.is_tensor(X) and X.is_cuda else device)
    R, T, F = x.shape
    if R < 1:
        raise ValueError("softdtw_barycenter: needs at least one series")
    if int(max_iter) < 0:
        raise ValueError("softdtw_barycenter: max_iter must not be negative")
    w = None
    if weights is not None:
        w = torch.as_tensor(np.asarray(weights.detach().cpu() if torch.is_tensor(weights) else weights, dtype=np.float64)).to(x.device)
        if tuple(w.shape) != (R,):
            raise ValueError(f"softdtw_barycenter: weights must be ({R},), got {tuple(w.shape)}")
    if init is None:
        xd = x.to(torch.float64)
        start = (xd.mean(dim=0) if w is None else (xd * w[:, None, None]).sum(dim=0) / w.sum()).cpu().numpy()
    else:
        start = np.array(init.detach().cpu() if torch.is_tensor(init) else init, dtype=np.float64)
        if start.ndim != 2 or start.shape[1] != F:
            raise ValueError(f"softdtw_barycenter: init must be (S, {F}), got {start.shape}")
    rows = torch.arange(R, dtype=torch.int64, device=x.device)
    z, nfev = _descend(x, rows, w, np.ascontiguousarray(start), g, int(max_iter), float(tol))
    return (z, nfev) if return_nfev else z


class SoftDTWKMeans(_SeriesKMeans):
    """tslearn's `TimeSeriesKMeans(metric="softdtw", metric_params={"gamma": g})` on the device, with the surface of
    `TimeSeriesKMeans` here; the loop is the soft-DTW block of include/g2v.h.  `gamma=` and `metric_params={"gamma": g}` name the
    same thing (the latter wins when both are given, tslearn's default is 1).  `nfev_`: per iteration, the function evaluations of
    every cluster's barycentre.  The clusters are optimised one after another, one ops.softdtw_grad launch set and one read-back
    per function evaluation."""

    def __init__(self, n_clusters=3, max_iter=50, tol=1e-6, n_init=1, metric="softdtw", max_iter_barycenter=100, gamma=1.0,
                 metric_params=None, random_state=None, init="random", barycenter_tol=1e-3, **refused):
        for name, value in refused.items():
            if name == "dtw_inertia":
                if value:
                    raise NotImplementedError("SoftDTWKMeans: `dtw_inertia` is not supported (inertia_ is the mean soft-DTW value)")
            elif name in ("verbose", "n_jobs"):
                pass
            else:
                raise TypeError(f"SoftDTWKMeans: unexpected argument `{name}`")
        if metric != "softdtw":
            raise ValueError(f"SoftDTWKMeans: metric={metric!r}; this class is metric='softdtw' only (TimeSeriesKMeans is 'dtw')")
        if metric_params is not None:
            other = sorted(set(metric_params) - {"gamma"})
            if other:
                raise NotImplementedError(f"SoftDTWKMeans: `metric_params` other than gamma are not supported (bands: {other})")
            gamma = metric_params.get("gamma", gamma)
        self._start(n_clusters, max_iter, tol, n_init, max_iter_barycenter, random_state, init)
        self.metric = metric
        self.gamma = _gamma(gamma, "SoftDTWKMeans")
        self.barycenter_tol = float(barycenter_tol)      # the tol of scipy's minimize (tslearn's softdtw_barycenter default)
        self.nfev_ = None

    def _assign(self, x, centers):
        from . import ops
        return ops.softdtw_cdist(x, centers, self.gamma, want_out=False, want_labels=True)[1:]

    def _fit_one(self, x, centers):
        self._nfev = []
        run = super()._fit_one(x, centers)
        return run + (self._nfev,)

    def _keep(self, nfev):
        self.nfev_ = nfev
        del self._nfev

    def _barycenters(self, x, labels, members, centers):
        """every cluster in turn: L-BFGS-B from its current centre over its member rows, in place on centers"""
        nfev = np.zeros(self.n_clusters, dtype=np.int64)
        for k in range(self.n_clusters):
            rows = torch.nonzero(labels == k).flatten()           # ascending row ids
            z, nfev[k] = _descend(x, rows, None, centers[k].cpu().numpy(), self.gamma, self.max_iter_barycenter, self.barycenter_tol)
            centers[k].copy_(torch.from_numpy(z))
        self._nfev.append(nfev)
