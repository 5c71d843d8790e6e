"""Evaluation metrics of a generated gesture set against the ground truth: the table columns the reference computes in
`scripts/Clustering.py::Metrics_analysis` (`:1353-1628`), with the statistics gathered on the device.

* Frechet distance between the chunk latents of the two sets (`frechet_distance` `:1376-1385`, `calculate_frechet_distance`
  `:1252-1315`): mean and covariance come from `LatentMoments` (g2v_moments_accumulate: one pass over the latents, fp32 MFMA on
  the upper triangle, float64 accumulators that are additive over batches and ranks), the distance itself is host float64.
* Hellinger distance (`hellinger` `:1635-1646`), code-usage perplexity (`:1539-1540`) and Wasserstein distance (`:1387-1394`) between
  the two code histograms (g2v_code_histogram: exact integer counts).

The reference does all of it on the host with numpy / scipy / sklearn on latents pulled off the device chunk by chunk; nothing here
needs scipy or sklearn.  For an autoencoder without a quantiser the code ids come from a fitted `gesture2vec_amd.kmeans.KMeans`
(`kmeans=`), as the reference takes them from its pickled k-means model.  Out of scope: BLEU over code sequences (`:1560-1609`, host
string work on `torchtext`) and the plots (the PCA + t-SNE maps are `gesture2vec_amd.embedding`)."""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np
import torch

from .pipeline import _need_cuda, chunk_latents

_SHIFT_ROWS = 256


class LatentMoments:
    """Running first and second moments of (N, E) fp32 latent rows about a fixed `shift`:
    S1 = sum (x - shift), S2 = sum (x - shift)(x - shift)^T (stored full and symmetric), n rows -- float64 on `device`.

    The sums are additive for one shift: a streamed set takes one `update` per batch, a data-parallel run one SUM all-reduce of
    `[S1 | S2]` and of the count (`all_reduce`), two accumulators `merge`.  `update` needs the GPU; everything else works on any
    device (states can be built, merged and finalized on the host)."""

    def __init__(self, E: int, device="cuda:0", shift=None):
        self.E = int(E)
        self.device = torch.device(device)
        self._acc = torch.zeros(self.E + self.E * self.E, dtype=torch.float64, device=self.device)     # [S1 | S2]
        self._n = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.shift = None if shift is None else self._as_shift(shift)

    def _as_shift(self, shift) -> torch.Tensor:
        t = torch.as_tensor(np.asarray(shift.detach().cpu() if torch.is_tensor(shift) else shift, dtype=np.float32))
        if t.shape != (self.E,):
            raise ValueError(f"shift must have shape ({self.E},), got {tuple(t.shape)}")
        return t.to(self.device).contiguous()

    @property
    def s1(self) -> torch.Tensor:
        return self._acc[:self.E]

    @property
    def s2(self) -> torch.Tensor:
        return self._acc[self.E:].view(self.E, self.E)

    @property
    def n(self) -> int:
        return int(self._n.item())

    @torch.no_grad()
    def update(self, rows: torch.Tensor) -> "LatentMoments":
        """Add the rows of a (N, E) fp32 GPU tensor (row stride >= E allowed).  The first call fixes `shift`, when none was given,
        to the mean of its first <= 256 rows (any value near the data keeps the covariance's cancellation small)."""
        from . import ops
        _need_cuda(rows, "LatentMoments.update")
        if self.device.type != "cuda":
            raise RuntimeError("LatentMoments.update runs on the MI355X kernels only (no CPU fallback)")
        if rows.dim() != 2 or rows.shape[1] != self.E:
            raise ValueError(f"rows must be (N, {self.E}), got {tuple(rows.shape)}")
        if rows.shape[0] == 0:
            return self
        if rows.dtype != torch.float32 or rows.stride(1) != 1:
            rows = rows.float().contiguous()
        if self.shift is None:
            head = rows[:_SHIFT_ROWS]
            tmp = torch.zeros_like(self._acc)
            ops.moments_accumulate(head, torch.zeros(self.E, dtype=torch.float32, device=self.device), tmp[:self.E],
                                   tmp[self.E:].view(self.E, self.E))
            self.shift = self._as_shift(tmp[:self.E].cpu().numpy() / head.shape[0])
        ops.moments_accumulate(rows, self.shift, self.s1, self.s2)
        self._n += rows.shape[0]
        return self

    def _same_shift(self, shift) -> bool:
        if self.shift is None or shift is None:
            return self.shift is None and shift is None
        return bool(np.array_equal(self.shift.cpu().numpy(), np.asarray(shift, dtype=np.float32)))

    def merge(self, other: "LatentMoments") -> "LatentMoments":
        if other.E != self.E:
            raise ValueError(f"merge: widths differ ({self.E} vs {other.E})")
        if not self._same_shift(None if other.shift is None else other.shift.cpu().numpy()):
            raise ValueError("merge: the two accumulators were built about different shifts; their sums do not add")
        self._acc += other._acc.to(self.device)
        self._n += other._n.to(self.device)
        return self

    def state(self) -> dict:
        return {"E": self.E, "n": np.int64(self.n), "shift": None if self.shift is None else self.shift.cpu().numpy().copy(),
                "s1": self.s1.cpu().numpy().copy(), "s2": self.s2.cpu().numpy().copy()}

    def load_state(self, state: dict) -> "LatentMoments":
        if int(state["E"]) != self.E:
            raise ValueError(f"load_state: width {int(state['E'])} does not match {self.E}")
        s1 = np.asarray(state["s1"], dtype=np.float64).reshape(self.E)
        s2 = np.asarray(state["s2"], dtype=np.float64).reshape(self.E, self.E)
        self._acc.copy_(torch.from_numpy(np.concatenate([s1, s2.reshape(-1)])))
        self._n.fill_(int(state["n"]))
        self.shift = None if state.get("shift") is None else self._as_shift(state["shift"])
        return self

    def all_reduce(self, reduce_fn: Callable[[torch.Tensor], torch.Tensor]) -> "LatentMoments":
        """reduce_fn: an in-place SUM all-reduce of a tensor (e.g. `dp.GradStatsAllReduce()`); called on [S1 | S2] (float64) and
        on the row count (int64).  Every rank must have used the same shift."""
        reduce_fn(self._acc)
        reduce_fn(self._n)
        return self

    def finalize(self):
        """(n, mean, cov) as float64 numpy: mean = shift + S1 / n, cov = (S2 - S1 S1^T / n) / (n - 1) (np.cov(rowvar=False))."""
        n = self.n
        if n < 2:
            raise ValueError(f"finalize: a covariance needs at least 2 rows, got {n}")
        s1, s2 = self.s1.cpu().numpy(), self.s2.cpu().numpy()
        shift = np.zeros(self.E) if self.shift is None else self.shift.cpu().numpy().astype(np.float64)
        return n, shift + s1 / n, (s2 - np.outer(s1, s1) / n) / (n - 1)


def _psd_sqrt(sigma: np.ndarray) -> np.ndarray:
    lam, v = np.linalg.eigh(sigma)
    return (v * np.sqrt(np.clip(lam, 0.0, None))) @ v.T


def frechet_distance(mu1, sigma1, mu2, sigma2) -> float:
    """|mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^(1/2) in float64.  tr (S1 S2)^(1/2) = sum_i sqrt(lambda_i(S1^(1/2) S2 S1^(1/2))):
    two symmetric eigendecompositions instead of the reference's `scipy.linalg.sqrtm` of the unsymmetric product.

    Parity with the reference (`calculate_frechet_distance`) is claimed for n > E rows in BOTH sets only: with n <= E a covariance
    is singular, `sqrtm` goes complex there and the reference keeps the real part of that (or falls back to its eps-regularised
    product), which is not the quantity above."""
    mu1, mu2 = np.atleast_1d(np.asarray(mu1, np.float64)), np.atleast_1d(np.asarray(mu2, np.float64))
    s1, s2 = np.atleast_2d(np.asarray(sigma1, np.float64)), np.atleast_2d(np.asarray(sigma2, np.float64))
    if mu1.shape != mu2.shape or s1.shape != s2.shape or s1.shape != (mu1.size, mu1.size):
        raise ValueError("frechet_distance: mean / covariance shapes do not match")
    s1, s2 = 0.5 * (s1 + s1.T), 0.5 * (s2 + s2.T)
    r = _psd_sqrt(s1)
    m = r @ s2 @ r
    lam = np.linalg.eigvalsh(0.5 * (m + m.T))
    diff = mu1 - mu2
    return float(diff @ diff + np.trace(s1) + np.trace(s2) - 2.0 * np.sqrt(np.clip(lam, 0.0, None)).sum())


def code_histogram(idx: torch.Tensor, K: int) -> np.ndarray:
    """(K,) int64 counts of the code ids of a GPU int64 tensor; an id outside [0, K) raises."""
    from . import ops
    _need_cuda(idx, "code_histogram")
    counts = ops.code_histogram(idx.reshape(-1).contiguous(), K).cpu().numpy()
    if counts[K]:
        raise ValueError(f"code_histogram: {int(counts[K])} ids outside [0, {K})")
    return counts[:K]


def _pdf(h) -> np.ndarray:
    h = np.asarray(h, dtype=np.float64)
    return h / h.sum()


def hellinger(h1, h2) -> float:
    return float(np.sqrt(1.0 - np.sum(np.sqrt(_pdf(h1) * _pdf(h2)))))


def histogram_perplexity(h) -> float:
    p = _pdf(h)
    return float(np.exp(-np.sum(p * np.log(p + 1e-10))))


def wasserstein(h1, h2) -> float:
    """sum_k |CDF1(k) - CDF2(k)| over unit-spaced bins: what `scipy.stats.wasserstein_distance(range(K), range(K), p, q)` evaluates."""
    return float(np.abs(np.cumsum(_pdf(h1)) - np.cumsum(_pdf(h2)))[:-1].sum())


@torch.no_grad()
def _scan(net, chunks: torch.Tensor, dae, batch_rows: int, K: Optional[int], kmeans=None):
    from . import ops
    mom, counts = None, None
    for a in range(0, chunks.shape[0], batch_rows):
        x = chunks[a:a + batch_rows]
        if dae is not None and dae.encoder is not None:
            B, T, D = x.shape
            x = dae.encode(x.reshape(B * T, D).contiguous()).view(B, T, -1)
        lat = chunk_latents(net, x)
        if mom is None:
            mom = LatentMoments(lat.shape[1], lat.device)
        mom.update(lat)
        if K is not None:
            counts = ops.code_histogram(kmeans.predict_device(lat) if kmeans is not None else net.vq_layer.assign(lat), K, counts)
    if K is not None:
        counts = counts.cpu().numpy()
        if counts[K]:
            raise ValueError(f"gesture_metrics: {int(counts[K])} code ids outside [0, {K})")
        counts = counts[:K]
    return mom, counts


@torch.no_grad()
def gesture_metrics(net, real_chunks: torch.Tensor, generated_chunks: torch.Tensor, dae=None, batch_rows: int = 65536,
                    kmeans=None) -> dict:
    """Both (N, T, D) chunk sets -> [dae.encode per frame ->] chunk_latents -> moments (+ vq_layer.assign -> histogram), streamed in
    batches of `batch_rows` chunks.  A net without a quantiser gives the Frechet distance and None for the code metrics, unless a
    fitted `kmeans` (gesture2vec_amd.kmeans.KMeans) is given: its ids then fill the histogram columns."""
    _need_cuda(real_chunks, "gesture_metrics")
    _need_cuda(generated_chunks, "gesture_metrics")
    if real_chunks.shape[0] == 0 or generated_chunks.shape[0] == 0:
        raise ValueError("gesture_metrics: an empty chunk set")
    if getattr(net, "vq", True):
        K, kmeans = int(net.vq_layer._num_embeddings), None
    else:
        K = None if kmeans is None else int(kmeans.n_clusters)
    m_r, h_r = _scan(net, real_chunks, dae, int(batch_rows), K, kmeans)
    m_g, h_g = _scan(net, generated_chunks, dae, int(batch_rows), K, kmeans)
    n_r, mu_r, cov_r = m_r.finalize()
    n_g, mu_g, cov_g = m_g.finalize()
    out = {"frechet": frechet_distance(mu_r, cov_r, mu_g, cov_g), "hellinger": None, "perplexity_real": None,
           "perplexity_generated": None, "wasserstein": None, "n_real": n_r, "n_generated": n_g}
    if K is not None:
        out.update(hellinger=hellinger(h_r, h_g), perplexity_real=histogram_perplexity(h_r),
                   perplexity_generated=histogram_perplexity(h_g), wasserstein=wasserstein(h_r, h_g))
    return out
