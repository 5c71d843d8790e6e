"""Evaluation metrics of a generated gesture set against the ground truth: the table columns the reference computes in
`scripts/Clustering.py::Metrics_analysis` (`:1353-1628`), with the statistics gathered on the device.

* Frechet distance between the chunk latents of the two sets (`frechet_distance` `:1376-1385`, `calculate_frechet_distance`
  `:1252-1315`): mean and covariance come from `LatentMoments` (g2v_moments_accumulate: one pass over the latents, fp32 MFMA on
  the upper triangle, float64 accumulators that are additive over batches and ranks), the distance itself is host float64.
* Hellinger distance (`hellinger` `:1635-1646`), code-usage perplexity (`:1539-1540`) and Wasserstein distance (`:1387-1394`) between
  the two code histograms (g2v_code_histogram: exact integer counts).

The reference does all of it on the host with numpy / scipy / sklearn on latents pulled off the device chunk by chunk; nothing here
needs scipy or sklearn.  For an autoencoder without a quantiser the code ids come from a fitted `gesture2vec_amd.kmeans.KMeans`
(`kmeans=`), as the reference takes them from its pickled k-means model.
* BLEU of each test case's code sequence against the ground truth's sequence of the same test case (`:1560-1609`:
  `torchtext.data.metrics.bleu_score(max_n=4, weights=[.25] * 4)`, one sentence and one reference per call): `code_bleu` -- the clipped
  n-gram counts over the integer ids come from g2v_ngram_clipped_counts, `bleu_from_counts` turns them into scores in float64 where
  the ids are.  torchtext forms the score in float32 and is not installed where this was written: parity with it is claimed from its
  definition, to float32 rounding, not from a recorded run.

* `energy_distance`: a second two-sample distance between the latents, beside the Frechet distance (not a reference column, and
  not part of `gesture_metrics`).

Out of scope: the plots (the PCA + t-SNE maps are `gesture2vec_amd.embedding`)."""
from __future__ import annotations

from typing import Callable, Optional, Sequence

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


def energy_distance(x: torch.Tensor, y: torch.Tensor) -> float:
    """The energy distance 2 E|x - y| - E|x - x'| - E|y - y'| between two sets of rows (n, E) and (m, E), fp32 on the GPU: a
    two-sample distance between the latents of real and generated chunks that, unlike the Frechet distance, assumes no Gaussians.
    0 for equal sets, symmetric.  The expectations are over ordered pairs (x' and y' independent copies, the n zero distances of a
    row to itself included): E|x - x'| = 2 sum_{i<j} |x_i - x_j| / n^2.  Three passes of repdist.pairwise_distance_stats; no
    distance is stored."""
    from .repdist import pairwise_distance_stats
    xy = pairwise_distance_stats(x, y)
    xx, yy = pairwise_distance_stats(x), pairwise_distance_stats(y)
    n, m = int(x.shape[0]), int(y.shape[0])
    return 2.0 * xy["mean"] - 2.0 * xx["sum"] / (float(n) * n) - 2.0 * yy["sum"] / (float(m) * m)


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


BLEU_MAX_LEN, BLEU_MAX_K = 4096, 65536                     # g2v_ngram_clipped_counts: longest sequence, largest codebook


def bleu_from_counts(clipped: torch.Tensor, cand_len: torch.Tensor, ref_len: torch.Tensor, weights=None, corpus: bool = False):
    """torchtext's `bleu_score` formula on clipped n-gram counts: clipped (B, max_n) integers, cand_len / ref_len (B,) -> (B,) float64
    scores on the inputs' device (any device; pure torch).  Per pair, with total_n = max(cand_len - n + 1, 0):
        0 if any clipped_n == 0, else exp(min(1 - ref_len / cand_len, 0)) * exp(sum_n w_n log(clipped_n / total_n)).
    weights: max_n numbers, default 1 / max_n each.  corpus=True: counts, totals and lengths are summed over the pairs first and ONE
    0-d score is returned (torchtext's corpus of several sentences with one reference each)."""
    if clipped.dim() != 2 or cand_len.shape != (clipped.shape[0],) or ref_len.shape != (clipped.shape[0],):
        raise ValueError(f"bleu_from_counts: clipped must be (B, max_n) and the lengths (B,), got {tuple(clipped.shape)}, "
                         f"{tuple(cand_len.shape)}, {tuple(ref_len.shape)}")
    max_n = clipped.shape[1]
    w = torch.full((max_n,), 1.0 / max_n, dtype=torch.float64) if weights is None else torch.as_tensor(weights, dtype=torch.float64)
    if w.shape != (max_n,):
        raise ValueError(f"bleu_from_counts: {max_n} orders need {max_n} weights, got {tuple(w.shape)}")
    w = w.to(clipped.device)
    clipped, lc, lr = clipped.to(torch.int64), cand_len.to(torch.int64), ref_len.to(torch.int64)
    n = torch.arange(1, max_n + 1, dtype=torch.int64, device=clipped.device)
    total = (lc[:, None] - n[None, :] + 1).clamp_min(0)
    if corpus:
        clipped, total, lc, lr = clipped.sum(0, keepdim=True), total.sum(0, keepdim=True), lc.sum(0, keepdim=True), lr.sum(0, keepdim=True)
    zero = (clipped <= 0).any(dim=1)                       # (clipped_n <= total_n: a zero total is a zero count)
    one = torch.ones((), dtype=torch.float64, device=clipped.device)
    pn = torch.where(zero[:, None], one, clipped.to(torch.float64) / total.clamp_min(1).to(torch.float64))
    bp = torch.exp((1.0 - lr.to(torch.float64) / lc.clamp_min(1).to(torch.float64)).clamp_max(0.0))
    score = torch.where(zero, torch.zeros_like(bp), bp * torch.exp((w[None, :] * torch.log(pn)).sum(dim=1)))
    return score[0] if corpus else score


def _flat_sequences(seqs, lengths, what: str):
    """-> (flat int64 ids, start (B,), len (B,), longest possible length, B); every tensor stays on the device"""
    if torch.is_tensor(seqs):
        if seqs.dim() != 2 or seqs.dtype != torch.int64:
            raise ValueError(f"code_bleu: {what} must be a (B, L) int64 tensor or a list of 1-D int64 tensors")
        _need_cuda(seqs, "code_bleu")
        B, L = seqs.shape
        if L > BLEU_MAX_LEN:
            raise ValueError(f"code_bleu: {what} rows hold {L} ids, the kernel takes at most {BLEU_MAX_LEN} per sequence")
        if B and L and (seqs.stride(1) != 1 or seqs.stride(0) < L):
            seqs = seqs.contiguous()
        stride = seqs.stride(0) if B and L else max(L, 1)
        flat = torch.as_strided(seqs, ((B - 1) * stride + L,), (1,)) if B and L else seqs.reshape(-1)
        start = torch.arange(B, dtype=torch.int64, device=seqs.device) * stride
        if lengths is None:
            lens = torch.full((B,), L, dtype=torch.int64, device=seqs.device)
        else:
            lens = torch.as_tensor(lengths).to(device=seqs.device, dtype=torch.int64).contiguous()
            if lens.shape != (B,):
                raise ValueError(f"code_bleu: {what} has {B} rows and {tuple(lens.shape)} lengths")
        return flat, start, lens, L, B
    seqs = list(seqs)
    if lengths is not None:
        raise ValueError(f"code_bleu: lengths go with a padded (B, L) tensor; a list of {what} carries its own")
    for t in seqs:
        if not torch.is_tensor(t) or t.dim() != 1 or t.dtype != torch.int64:
            raise ValueError(f"code_bleu: {what} must be a (B, L) int64 tensor or a list of 1-D int64 tensors")
        _need_cuda(t, "code_bleu")
    sizes = [int(t.numel()) for t in seqs]                  # (shapes: host knowledge, nothing is read back)
    if sizes and max(sizes) > BLEU_MAX_LEN:
        raise ValueError(f"code_bleu: a sequence of {what} holds {max(sizes)} ids, the kernel takes at most {BLEU_MAX_LEN}")
    dev = seqs[0].device if seqs else torch.device("cuda:0")
    flat = torch.cat(seqs) if seqs else torch.zeros((0,), dtype=torch.int64, device=dev)
    lens_h = np.asarray(sizes, dtype=np.int64)
    start_h = np.concatenate([[0], np.cumsum(lens_h)[:-1]]).astype(np.int64) if sizes else lens_h
    return flat, torch.from_numpy(start_h).to(dev), torch.from_numpy(lens_h).to(dev), max(sizes, default=0), len(sizes)


@torch.no_grad()
def code_bleu(candidates, references, *, cand_lengths=None, ref_lengths=None, K: int, max_n: int = 4, weights=None) -> torch.Tensor:
    """BLEU of B candidate code sequences, each against ITS reference sequence -> (B,) float64 scores on the GPU: torchtext's
    `bleu_score([cand], [[ref]], max_n, weights)` per pair, as `Metrics_analysis` calls it per test case.  ONE reference per candidate
    is supported (all the reference program uses); several references per candidate are not.

    candidates / references: each a (B, L) int64 GPU tensor of ids in [0, K) (rows may be strided; `cand_lengths` / `ref_lengths`,
    tensors or sequences of B numbers, give shorter rows -- what lies past a length is not read), or a list of B 1-D int64 GPU
    tensors.  The padded route reads nothing back; the scores stay on the device.  After the launch ONE number comes back: the count
    of pairs with an id outside [0, K) or a length outside [0, L]; a non-zero count raises ValueError."""
    from . import ops
    if not 1 <= int(K) <= BLEU_MAX_K:
        raise ValueError(f"code_bleu: K = {K} outside [1, {BLEU_MAX_K}] (an n-gram is packed from 16-bit ids)")
    if not 1 <= int(max_n) <= 4:
        raise ValueError(f"code_bleu: max_n = {max_n} outside [1, 4]")
    c, cs, cl, c_max, Bc = _flat_sequences(candidates, cand_lengths, "candidates")
    r, rs, rl, r_max, Br = _flat_sequences(references, ref_lengths, "references")
    if Bc != Br:
        raise ValueError(f"code_bleu: {Bc} candidates against {Br} references: one reference per candidate")
    if c.device != r.device:
        raise ValueError("code_bleu: candidates and references are on different devices")
    if Bc == 0:
        return torch.zeros((0,), dtype=torch.float64, device=c.device)
    clipped, bad = ops.ngram_clipped_counts(c, cs, cl, r, rs, rl, int(K), int(max_n), max(c_max, r_max))
    n_bad = int(bad.item())
    if n_bad:
        raise ValueError(f"code_bleu: {n_bad} of {Bc} pairs hold a code id outside [0, {K}) or a length outside its row")
    return bleu_from_counts(clipped, cl, rl, weights)


def _clip_counts(clips, n_chunks: int, what: str) -> list:
    counts = [int(v) for v in np.asarray(clips).reshape(-1)]
    if any(v < 0 for v in counts) or sum(counts) != n_chunks:
        raise ValueError(f"gesture_metrics: {what} must be non-negative chunk counts that sum to the set's {n_chunks} chunks, "
                         f"got a sum of {sum(counts)}")
    return counts


@torch.no_grad()
def _scan(net, chunks: torch.Tensor, dae, batch_rows: int, K: Optional[int], kmeans=None, keep_ids: bool = False):
    from . import ops
    mom, counts, kept = None, None, []
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
            ids = kmeans.predict_device(lat) if kmeans is not None else net.vq_layer.assign(lat)
            counts = ops.code_histogram(ids, K, counts)
            if keep_ids:
                kept.append(ids)
    if K is not None:
        counts = counts.cpu().numpy()
        if counts[K]:
            raise ValueError(f"gesture_metrics: {int(counts[K])} code ids outside [0, {K})")
        counts = counts[:K]
    if keep_ids:
        return mom, counts, torch.cat(kept)
    return mom, counts


@torch.no_grad()
def set_latents(net, chunks: torch.Tensor, dae=None, batch_rows: int = 65536) -> torch.Tensor:
    """The latent rows `gesture_metrics` scans, kept: (N, T, D) chunks -> [dae.encode per frame ->] chunk_latents -> (N, E) fp32"""
    _need_cuda(chunks, "set_latents")
    rows = []
    for a in range(0, chunks.shape[0], int(batch_rows)):
        x = chunks[a:a + int(batch_rows)]
        if dae is not None and dae.encoder is not None:
            B, T, D = x.shape
            x = dae.encode(x.reshape(B * T, D).contiguous()).view(B, T, -1)
        rows.append(chunk_latents(net, x))
    return torch.cat(rows)


@torch.no_grad()
def gesture_metrics(net, real_chunks: torch.Tensor, generated_chunks: torch.Tensor, dae=None, batch_rows: int = 65536,
                    kmeans=None, real_clips: Optional[Sequence[int]] = None, generated_clips: Optional[Sequence[int]] = None) -> dict:
    """Both (N, T, D) chunk sets -> [dae.encode per frame ->] chunk_latents -> moments (+ vq_layer.assign -> histogram), streamed in
    batches of `batch_rows` chunks.  A net without a quantiser gives the Frechet distance and None for the code metrics, unless a
    fitted `kmeans` (gesture2vec_amd.kmeans.KMeans) is given: its ids then fill the histogram columns.

    real_clips / generated_clips (both or neither; equally many): the number of consecutive chunks of each clip (test case) of the
    set, summing to its N.  The code ids of the scan are then kept, and clip i of the generated set is scored against clip i of the
    real set with `code_bleu`; the result gains `bleu` (mean over the clips), `bleu_var` (np.var: what the reference prints behind
    `+-`), `bleu_sum` and `bleu_scores` (float64 numpy, per clip).  Needs code ids: a quantiser or `kmeans=`."""
    _need_cuda(real_chunks, "gesture_metrics")
    _need_cuda(generated_chunks, "gesture_metrics")
    if real_chunks.shape[0] == 0 or generated_chunks.shape[0] == 0:
        raise ValueError("gesture_metrics: an empty chunk set")
    if (real_clips is None) != (generated_clips is None):
        raise ValueError("gesture_metrics: real_clips and generated_clips go together (clip i is scored against clip i)")
    clips = real_clips is not None
    if clips:
        real_clips = _clip_counts(real_clips, real_chunks.shape[0], "real_clips")
        generated_clips = _clip_counts(generated_clips, generated_chunks.shape[0], "generated_clips")
        if len(real_clips) != len(generated_clips) or not real_clips:
            raise ValueError(f"gesture_metrics: {len(real_clips)} real clips against {len(generated_clips)} generated ones")
    if getattr(net, "vq", True):
        K, kmeans = int(net.vq_layer._num_embeddings), None
    else:
        K = None if kmeans is None else int(kmeans.n_clusters)
    if clips and K is None:
        raise ValueError("gesture_metrics: BLEU is scored over code ids: a net without a quantiser needs a fitted kmeans=")
    m_r, h_r, *ids_r = _scan(net, real_chunks, dae, int(batch_rows), K, kmeans, keep_ids=clips)
    m_g, h_g, *ids_g = _scan(net, generated_chunks, dae, int(batch_rows), K, kmeans, keep_ids=clips)
    n_r, mu_r, cov_r = m_r.finalize()
    n_g, mu_g, cov_g = m_g.finalize()
    out = {"frechet": frechet_distance(mu_r, cov_r, mu_g, cov_g), "hellinger": None, "perplexity_real": None,
           "perplexity_generated": None, "wasserstein": None, "n_real": n_r, "n_generated": n_g}
    if K is not None:
        out.update(hellinger=hellinger(h_r, h_g), perplexity_real=histogram_perplexity(h_r),
                   perplexity_generated=histogram_perplexity(h_g), wasserstein=wasserstein(h_r, h_g))
    if clips:
        scores = code_bleu(list(torch.split(ids_g[0], generated_clips)), list(torch.split(ids_r[0], real_clips)), K=K)
        scores = scores.cpu().numpy()
        out.update(bleu=float(np.mean(scores)), bleu_var=float(np.var(scores)), bleu_sum=float(np.sum(scores)), bleu_scores=scores)
    return out
