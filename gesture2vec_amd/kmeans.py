"""k-means codes for the latents of a quantiser-free autoencoder (`autoencoder_vq: False`), fitted and applied on the device.

The reference fits `sklearn.cluster.KMeans(n_clusters=300, max_iter=2500, random_state=0)` on the `(N, L*H)` chunk latents
(`Clustering.py:705-725`), pickles it to `<ckpt dir>/clusters/kmeans_model.pk` and calls `kmeanmodel.predict(latents)` wherever the
VQ-VAE path calls its quantiser (`lmdb_data_loader.py:1097-1103, 1287-1292`, `inference_text2embedding.py:169-219`).  `KMeans` here has
the same constructor arguments, attributes and `predict`, so those call sites work on it; sklearn itself is not imported.

One Lloyd iteration = the exact fp32 argmin of the quantiser kernels (`ops.vq_assign`, lowest index on ties; the centres are padded
to a multiple of 16 with rows whose squared norm is +inf, which never win) + `g2v_kmeans_update` (counts, float64 sums, centres,
inertia, shift, changed labels, sklearn's empty-cluster relocation in a fixed order) + `g2v_kmeans_commit`.  Convergence is decided on
the device in a small state block; once it is set every k-means kernel and the commit are no-ops, so `check_every=m` enqueues m
iterations per read-back and gives bitwise the result of m = 1 (the assignment kernels are not gated: up to m - 1 assignments past
convergence are computed and dropped, so keep m small where the assignment dominates).  Seeding is sklearn's greedy k-means++ with the uniform draws of
`numpy.random.RandomState(seed)` in sklearn's order (`g2v_kmeans_pp_step`; bit-parity of the picks with sklearn is not a goal),
`init="random"` (`RandomState(seed).permutation(N)[:K]`), or a given (K, E) array."""
from __future__ import annotations

import math

import numpy as np
import torch

from .pipeline import _need_cuda

_PAD = 16
PP_MAX_TRIALS = 8          # candidates per g2v_kmeans_pp_step


def _code_perplexity(counts) -> float:
    p = np.asarray(counts, dtype=np.float64)
    p = p / p.sum()
    return float(np.exp(-np.sum(p * np.log(p + 1e-10))))


class KMeans:
    def __init__(self, n_clusters=300, init="k-means++", n_init=1, max_iter=2500, tol=1e-4, random_state=0, check_every=1):
        if int(n_clusters) < 1 or int(n_init) < 1 or int(max_iter) < 1 or int(check_every) < 1:
            raise ValueError("KMeans: n_clusters, n_init, max_iter and check_every must be positive")
        self.n_clusters = int(n_clusters)
        self.init = init
        self.n_init = int(n_init)
        self.max_iter = int(max_iter)
        self.tol = float(tol)
        self.random_state = random_state
        self.check_every = int(check_every)
        self.cluster_centers_ = None
        self.labels_ = None
        self.inertia_ = None
        self.n_iter_ = None
        self.init_rows_ = None         # rows the last seeding chose (k-means++ / random)
        self._dev = {}                 # device -> (padded centres, their squared norms); never pickled

    # ---- construction / pickling ------------------------------------------------------------------------------------------------
    @classmethod
    def from_centers(cls, centers) -> "KMeans":
        """A fitted model around given centres, e.g. an sklearn pickle's `cluster_centers_`."""
        c = np.ascontiguousarray(np.asarray(centers.detach().cpu() if torch.is_tensor(centers) else centers, dtype=np.float32))
        if c.ndim != 2 or c.shape[0] < 1:
            raise ValueError(f"from_centers: expected a (K, E) array, got shape {c.shape}")
        km = cls(n_clusters=c.shape[0])
        km.cluster_centers_ = c
        return km

    def __getstate__(self):
        d = dict(self.__dict__)
        d["_dev"] = {}
        if not isinstance(d["init"], str):
            d["init"] = np.asarray(d["init"].detach().cpu() if torch.is_tensor(d["init"]) else d["init"])
        return d

    # ---- device helpers -----------------------------------------------------------------------------------------------------------
    def _padded(self, K, E, dev):
        Kp = (K + _PAD - 1) // _PAD * _PAD
        cen = torch.zeros((Kp, E), dtype=torch.float32, device=dev)
        sq = torch.full((Kp,), float("inf"), dtype=torch.float32, device=dev)     # the padding rows: never the argmin
        return cen, sq

    @staticmethod
    def _assign(x, cen, sq, K):
        from . import ops
        ops.vq_code_sqnorm(cen[:K], out=sq)                  # (writes the first K entries)
        return ops.vq_assign(x, None, cen, sq, want_quantized=False)[0]

    def _check_rows(self, x, what):
        _need_cuda(x, what)
        if x.dim() != 2 or x.dtype != torch.float32:
            raise TypeError(f"{what}: expected a (N, E) fp32 tensor, got {tuple(x.shape)} {x.dtype}")
        return x.contiguous()

    # ---- seeding ------------------------------------------------------------------------------------------------------------------
    def _kmeans_pp(self, x, rs):
        """Greedy k-means++ (sklearn `_kmeans_plusplus`): (K,E) device centres and the chosen rows, consuming `rs` in sklearn's
        order: one `random_sample()` for the first centre, `uniform(size=2 + int(log K))` per further centre (8 at the most)."""
        from . import ops
        N, E = x.shape
        K = self.n_clusters
        dev = x.device
        nblk = ops.kmeans_pp_blocks(N)
        trials = min(2 + int(math.log(K)), PP_MAX_TRIALS)
        centers = torch.empty((K, E), dtype=torch.float32, device=dev)
        closest = torch.full((N,), float("inf"), dtype=torch.float64, device=dev)
        out = torch.zeros((nblk + 11,), dtype=torch.float64, device=dev)
        first = min(int(rs.random_sample() * N), N - 1)
        ops.kmeans_pp_step(x, closest, [first], None, out, centers[0])
        rows = []
        for c in range(1, K + 1):
            h = out.cpu().numpy()                            # block sums of closest[], the row just chosen, the current potential
            rows.append(int(h[nblk + 9]))
            if c == K:
                break
            cum = np.cumsum(h[:nblk])
            vals = rs.uniform(size=trials) * h[nblk + 10]
            blk = np.minimum(np.searchsorted(cum, vals), nblk - 1)
            resid = vals - np.where(blk > 0, cum[np.maximum(blk - 1, 0)], 0.0)
            ops.kmeans_pp_step(x, closest, blk.tolist(), resid.tolist(), out, centers[c])
        return centers, rows

    def _init_centers(self, x, rs):
        N, E = x.shape
        K = self.n_clusters
        if isinstance(self.init, str):
            if K > N:
                raise ValueError(f"KMeans: n_clusters = {K} exceeds the {N} rows")
            if self.init == "k-means++":
                centers, self.init_rows_ = self._kmeans_pp(x, rs)
                return centers
            if self.init == "random":
                self.init_rows_ = [int(i) for i in rs.permutation(N)[:K]]
                return x[torch.tensor(self.init_rows_, dtype=torch.int64, device=x.device)].contiguous()     # a gather: layout only
            raise ValueError(f"KMeans: unknown init {self.init!r}")
        c = self.init.detach() if torch.is_tensor(self.init) else torch.from_numpy(np.asarray(self.init, dtype=np.float32))
        if tuple(c.shape) != (K, E):
            raise ValueError(f"KMeans: init must have shape ({K}, {E}), got {tuple(c.shape)}")
        return c.to(device=x.device, dtype=torch.float32).contiguous()

    # ---- fit ----------------------------------------------------------------------------------------------------------------------
    def _lloyd(self, x, init_centers):
        from . import ops
        N, E = x.shape
        K = self.n_clusters
        dev = x.device
        cen, sq = self._padded(K, E, dev)
        cen[:K].copy_(init_centers)
        state = torch.zeros((8,), dtype=torch.float64, device=dev)
        ops.kmeans_tolerance(x, self.tol, out=state[7:8])
        labels = torch.full((N,), -1, dtype=torch.int64, device=dev)
        buf, it = None, 0
        st = None
        while it < self.max_iter:
            m = min(self.check_every, self.max_iter - it)
            for _ in range(m):
                idx = self._assign(x, cen, sq, K)
                buf = ops.kmeans_update(x, idx, cen[:K], labels, relocate=True, state=state, out=buf)
                ops.kmeans_commit(state, buf["centers_new"], cen[:K], idx, labels)
            it += m
            st = state.cpu().numpy()
            if st[0] != 0.0:
                break
        n_iter = int(st[1])
        strict = st[0] != 0.0 and st[2] == 0.0
        if not strict:                                       # stopped by tol or max_iter: labels of the final centres, as sklearn
            labels = self._assign(x, cen, sq, K)
        fin = ops.kmeans_update(x, labels, cen[:K], None, relocate=False)
        inertia = float(fin["stats"][0].item())
        return cen, sq, labels, inertia, n_iter

    @torch.no_grad()
    def fit(self, latents: torch.Tensor) -> "KMeans":
        x = self._check_rows(latents, "KMeans.fit")
        rs = self.random_state if isinstance(self.random_state, np.random.RandomState) else np.random.RandomState(self.random_state)
        n_init = 1 if not isinstance(self.init, str) else self.n_init
        best = None
        for _ in range(n_init):
            run = self._lloyd(x, self._init_centers(x, rs))
            if best is None or run[3] < best[3]:
                best = run
        cen, sq, labels, inertia, n_iter = best
        K = self.n_clusters
        self.cluster_centers_ = cen[:K].cpu().numpy()
        self.labels_ = labels.cpu().numpy().astype(np.int32)
        self.inertia_, self.n_iter_ = inertia, n_iter
        self._dev = {str(x.device): (cen, sq)}
        return self

    # ---- predict ------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def predict_device(self, latents: torch.Tensor) -> torch.Tensor:
        """(N, E) fp32 GPU rows -> (N,) int64 GPU ids: the fp32 argmin over the centres, lowest index on ties."""
        if self.cluster_centers_ is None:
            raise RuntimeError("KMeans: not fitted")
        x = self._check_rows(latents, "KMeans.predict_device")
        K, E = self.cluster_centers_.shape
        if x.shape[1] != E:
            raise ValueError(f"KMeans.predict_device: rows have {x.shape[1]} columns, the centres {E}")
        key = str(x.device)
        if key not in self._dev:
            cen, sq = self._padded(K, E, x.device)
            cen[:K].copy_(torch.from_numpy(self.cluster_centers_))
            self._dev[key] = (cen, sq)
        cen, sq = self._dev[key]
        if x.shape[0] == 0:
            return torch.empty((0,), dtype=torch.int64, device=x.device)
        return self._assign(x, cen, sq, K)

    def predict(self, x, device="cuda:0") -> np.ndarray:
        """numpy or torch rows -> numpy int32 ids (sklearn's `kmeanmodel.predict`); the work is done on `device`."""
        t = x.detach() if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32)))
        if not t.is_cuda:
            t = t.to(device)
        return self.predict_device(t.float().reshape(-1, t.shape[-1])).cpu().numpy().astype(np.int32)

    def fit_predict(self, latents) -> np.ndarray:
        return self.fit(latents).labels_

    def code_perplexity(self) -> float:
        """exp(entropy) of the fitted labels' histogram (the usage figure the VQ-VAE path reports for its codebook)."""
        return _code_perplexity(np.bincount(self.labels_, minlength=self.n_clusters))

    def silhouette(self, x, sample_size=None, random_state=None) -> float:
        """Mean silhouette coefficient of the fitted labels over the rows `x` they were fitted on (silhouette.silhouette_score)."""
        from .silhouette import silhouette_score
        return silhouette_score(x, self.labels_, sample_size, random_state, self.n_clusters)
