#!/usr/bin/env python3
"""Fits the k-means model a quantiser-free chunk autoencoder (`autoencoder_vq: False`) needs downstream, on the MI355X kernels
(gesture2vec_amd/kmeans.py): the reference's `Clustering.py:705-725`.

    python cluster_latents.py --checkpoint autoencoder_checkpoint.bin --chunks x.npy [--n_clusters 300] [--scan-k 50:400:50]
                              [--silhouette-rows M | --no-silhouette]
    python cluster_latents.py --checkpoint autoencoder_checkpoint.bin --chunks x.npy --algorithm dbscan --eps 0.5 --min-samples 5
                              [--k-distances K]
    python cluster_latents.py --checkpoint autoencoder_checkpoint.bin --chunks x.npy --algorithm ward [--n_clusters 300 |
                              --distance-threshold T] [--scan-k 50:400:50]
    python cluster_latents.py --checkpoint autoencoder_checkpoint.bin --chunks x.npy --algorithm dtw --n_clusters 40 --max_iter 5
                              --max-iter-barycenter 5
    python cluster_latents.py --checkpoint autoencoder_checkpoint.bin --chunks x.npy --algorithm softdtw --gamma 0.5 --n_clusters 40
                              --max_iter 5 --max-iter-barycenter 5

`--chunks` holds (N, T, D) pose chunks in the autoencoder's input space.  Their latents (`chunk_latents`) are clustered with
`KMeans(n_clusters, max_iter=2500, random_state=0)` and the model is pickled to `<checkpoint dir>/clusters/kmeans_model.pk`, where the
reference's data loader and inference script look for it; `n_iter`, inertia, the code-usage perplexity and the silhouette coefficient
of the fitted labels are printed.
`--scan-k a:b:step` prints the two curves of `Clustering.py:586-624` (`init="random", n_init=10, max_iter=300` per k), inertia and
silhouette coefficient (gesture2vec_amd/silhouette.py, on the device), instead of writing a model, and returns `(k, inertia,
silhouette)` triples.  The silhouette is taken over all latents up to 65 536 rows and over `--silhouette-rows M` rows sampled as
sklearn's `sample_size` (seeded with `--seed`) beyond that or when M is given; `--no-silhouette` leaves it out (None in the triples).
`--algorithm dbscan` is the other branch of the reference's switch (`Clustering.py:742-750, 962-972`): `DBSCAN(eps, min_samples)` on
the device (gesture2vec_amd/dbscan.py), the reference's two printed lines, and `labels` and the `core` mask in an `.npz` at `--out`
(default `<checkpoint dir>/clusters/dbscan_labels.npz`).  `--k-distances K` adds the curve one reads `eps` from, as `k_distances`:
every row's distance to its K-th nearest row counting itself (K = the `min_samples` one has in mind), sorted ascending
(`dbscan.k_distances`); its quartiles are printed.
`--algorithm ward` is the third (`Clustering.py:751-755`): `AgglomerativeClustering(linkage="ward", n_clusters)` on the device
(gesture2vec_amd/agglomerative.py), cut at `--n_clusters` or, instead, at `--distance-threshold`; `labels`, `children` and the merge
`heights` go to an `.npz` at `--out` (default `<checkpoint dir>/clusters/ward_labels.npz`).  With `--scan-k a:b:step` the tree is
fitted once and the silhouette coefficient of `cut(k)` is printed per k; `(k, silhouette)` pairs are returned and nothing is written.
`--algorithm dtw` clusters the `--chunks` sequences themselves under dynamic time warping, with no encoder pass: the reference's
`TimeSeriesKMeans(n_clusters=40, metric="dtw", max_iter=5, max_iter_barycenter=5, random_state=0)` (`Clustering.py:629-669`; its
own call is `--n_clusters 40 --max_iter 5 --max-iter-barycenter 5`) on the device (gesture2vec_amd/timeseries.py), with
`--n_clusters`, `--max_iter`, `--n_init`, `--seed` and `--max-iter-barycenter`.  `--checkpoint` only names the default output directory
then.  `n_iter`, inertia and the usage perplexity are printed and the model is pickled to `<checkpoint dir>/clusters/dtw_kmeans_model.pk`
or `--out`.
`--algorithm softdtw` is the same under soft-DTW: the reference's `TimeSeriesKMeans(n_clusters=40, metric="softdtw", max_iter=5,
max_iter_barycenter=5, metric_params={"gamma": 0.5}, random_state=0)` (`Clustering.py:670-691`) as `SoftDTWKMeans` with `--gamma`;
the model is pickled to `<checkpoint dir>/clusters/softdtw_kmeans_model.pk` or `--out`.
`--rep-distance [--rep-seed S]` also writes the reference's `Rep_distance.txt` (`calculate_distances`, `Clustering.py:410-505`, whose call
at `:580` is commented out because `pdist` cannot hold the pairs at scale) next to the model or labels file, and prints it: the
representation-similarity numbers of the latents, both methods (gesture2vec_amd/repdist.py; at least 1004 latents, the reference
samples 1000 of them).  It needs the latents, so it does not go with `--algorithm dtw|softdtw`."""
from __future__ import annotations

import argparse
import os
import pickle
import sys

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
for _p in (_HERE, _ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from utils.train_utils import load_checkpoint_and_model  # noqa: E402
from gesture2vec_amd.agglomerative import AgglomerativeClustering  # noqa: E402
from gesture2vec_amd.dbscan import DBSCAN, k_distances  # noqa: E402
from gesture2vec_amd.kmeans import KMeans  # noqa: E402
from gesture2vec_amd.pipeline import chunk_latents  # noqa: E402
from gesture2vec_amd.repdist import representation_report  # noqa: E402
from gesture2vec_amd.timeseries import SoftDTWKMeans, TimeSeriesKMeans  # noqa: E402


SILHOUETTE_ROWS = 65536        # latents beyond this many are sampled for the silhouette coefficient


@torch.no_grad()
def latents_of(net, chunks: torch.Tensor, batch_rows: int) -> torch.Tensor:
    return torch.cat([chunk_latents(net, chunks[a:a + batch_rows]) for a in range(0, chunks.shape[0], batch_rows)])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--checkpoint", required=True, help="chunk autoencoder checkpoint (train_autoencoder_VQVAE.py)")
    ap.add_argument("--chunks", required=True, help=".npy of (N, T, D) pose chunks")
    ap.add_argument("--n_clusters", type=int, default=300)
    ap.add_argument("--max_iter", type=int, default=2500)
    ap.add_argument("--n_init", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--check_every", type=int, default=4, help="Lloyd iterations enqueued per convergence read-back")
    ap.add_argument("--scan-k", dest="scan_k", default=None, help="a:b:step -- print the inertia per k instead of writing a model")
    ap.add_argument("--silhouette-rows", dest="silhouette_rows", type=int, default=None,
                    help="rows the silhouette is sampled over (default: all rows up to 65536, that many sampled beyond)")
    ap.add_argument("--no-silhouette", dest="silhouette", action="store_false", help="do not compute silhouette coefficients")
    ap.add_argument("--out", default=None, help="model path (default: <checkpoint dir>/clusters/kmeans_model.pk; dbscan: the .npz of labels, dbscan_labels.npz there; ward: ward_labels.npz there; dtw: dtw_kmeans_model.pk there; softdtw: softdtw_kmeans_model.pk there)")
    ap.add_argument("--algorithm", choices=("kmeans", "dbscan", "ward", "dtw", "softdtw"), default="kmeans",
                    help="the branch of the reference's clustering switch: {kmeans,dbscan} as before, or ward = "
                         "AgglomerativeClustering(linkage='ward') cut at --n_clusters or --distance-threshold; "
                         "{kmeans,dbscan,ward} cluster the chunks' latents, dtw = TimeSeriesKMeans(metric='dtw') and softdtw = "
                         "SoftDTWKMeans(gamma) the chunk sequences themselves")
    ap.add_argument("--max-iter-barycenter", dest="max_iter_barycenter", type=int, default=5,
                    help="dtw: barycentre averaging steps per cluster and iteration; softdtw: L-BFGS-B iterations per barycentre")
    ap.add_argument("--gamma", type=float, default=0.5, help="softdtw: the temperature of the soft minimum")
    ap.add_argument("--distance-threshold", dest="distance_threshold", type=float, default=None,
                    help="ward: cut the tree below this merge height instead of at --n_clusters")
    ap.add_argument("--eps", type=float, default=0.5, help="dbscan: the neighbourhood radius")
    ap.add_argument("--min-samples", dest="min_samples", type=int, default=5, help="dbscan: neighbours (itself included) of a core row")
    ap.add_argument("--k-distances", dest="k_distances", type=int, default=None, metavar="K",
                    help="dbscan: also write every row's distance to its K-th nearest row (itself included), sorted: the curve eps is read from")
    ap.add_argument("--rep-distance", dest="rep_distance", action="store_true",
                    help="also write and print Rep_distance.txt, the reference's representation-similarity numbers of the latents")
    ap.add_argument("--rep-seed", dest="rep_seed", type=int, default=None, help="--rep-distance: seed of the 1000 sampled rows")
    ap.add_argument("--batch_rows", type=int, default=65536)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    if a.rep_distance and a.algorithm in ("dtw", "softdtw"):
        ap.error("--rep-distance measures the latents: --algorithm dtw and softdtw have none")
    if a.rep_seed is not None and not a.rep_distance:
        ap.error("--rep-seed goes with --rep-distance")
    if a.k_distances is not None and a.algorithm != "dbscan":
        ap.error("--k-distances goes with --algorithm dbscan")
    dev = torch.device(a.device)
    if a.algorithm in ("dtw", "softdtw"):                        # the sequences themselves: no encoder pass, the checkpoint is not read
        chunks = torch.from_numpy(np.load(a.chunks).astype(np.float32, copy=False)).to(dev)
        print(f"sequences: {tuple(chunks.shape)}")
        common = dict(n_clusters=a.n_clusters, max_iter=a.max_iter, n_init=a.n_init, random_state=a.seed,
                      max_iter_barycenter=a.max_iter_barycenter)
        ts = (TimeSeriesKMeans(**common) if a.algorithm == "dtw" else SoftDTWKMeans(gamma=a.gamma, **common)).fit(chunks)
        out = a.out or os.path.join(os.path.dirname(os.path.abspath(a.checkpoint)), "clusters", a.algorithm + "_kmeans_model.pk")
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "wb") as f:
            pickle.dump(ts, f)
        print(f"n_iter: {ts.n_iter_}")
        print(f"inertia: {ts.inertia_!r}")
        print(f"code-usage perplexity: {ts.code_perplexity()!r} of {ts.n_clusters}")
        print(f"wrote {out}")
        return ts
    _, net, _, _, _ = load_checkpoint_and_model(a.checkpoint, dev, "autoencoder_vq")
    net.eval()
    chunks = torch.from_numpy(np.load(a.chunks).astype(np.float32, copy=False)).to(dev)
    lat = latents_of(net, chunks, a.batch_rows)
    print(f"latents: {tuple(lat.shape)}")
    if a.rep_distance:
        rep_dir = os.path.dirname(os.path.abspath(a.out)) if a.out else os.path.join(os.path.dirname(os.path.abspath(a.checkpoint)), "clusters")
        os.makedirs(rep_dir, exist_ok=True)
        text = representation_report(lat, seed=a.rep_seed)
        print(text)
        with open(os.path.join(rep_dir, "Rep_distance.txt"), "w") as f:
            f.write(text)
        print(f"wrote {os.path.join(rep_dir, 'Rep_distance.txt')}")

    if a.algorithm == "dbscan":
        db = DBSCAN(eps=a.eps, min_samples=a.min_samples).fit(lat)
        print("Estimated number of clusters: %d" % db.n_clusters_)
        print("Estimated number of noise points: %d" % db.n_noise_)
        out = a.out or os.path.join(os.path.dirname(os.path.abspath(a.checkpoint)), "clusters", "dbscan_labels.npz")
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        core = np.zeros(lat.shape[0], dtype=bool)
        core[db.core_sample_indices_.cpu().numpy()] = True
        arrays = {"labels": db.labels_.cpu().numpy(), "core": core}
        if a.k_distances is not None:
            arrays["k_distances"] = k_distances(lat, a.k_distances).cpu().numpy()
            print(f"{a.k_distances}-distances: quartiles " + ", ".join(repr(float(v)) for v in
                                                                   np.quantile(arrays["k_distances"], (0.25, 0.5, 0.75))))
        with open(out, "wb") as f:                               # (a file object: numpy appends no suffix of its own)
            np.savez(f, **arrays)
        print(f"wrote {out}")
        return db

    if a.algorithm == "ward":
        from gesture2vec_amd.silhouette import silhouette_score
        if a.scan_k:                                             # one tree answers every k: the fit's own cut is the first of them
            lo, hi, step = (int(v) for v in a.scan_k.split(":"))
            a.n_clusters, a.distance_threshold = lo, None
        by_k = a.distance_threshold is None
        ac = AgglomerativeClustering(n_clusters=a.n_clusters if by_k else None, distance_threshold=a.distance_threshold,
                                     compute_distances=True, check_every=a.check_every).fit(lat)
        print(f"rounds: {ac.n_rounds_}")
        if a.scan_k:
            curve = []
            for k in range(lo, hi, step):
                sil = silhouette_score(lat, ac.cut(k)) if a.silhouette else None
                curve.append((k, sil))
                print(f"k = {k}" + (f": silhouette {sil!r}" if a.silhouette else ""))
            return curve
        print("Number of clusters: %d" % ac.n_clusters_)
        out = a.out or os.path.join(os.path.dirname(os.path.abspath(a.checkpoint)), "clusters", "ward_labels.npz")
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "wb") as f:
            np.savez(f, labels=ac.labels_.cpu().numpy(), children=ac.children_, heights=ac.distances_)
        print(f"wrote {out}")
        return ac

    def silhouette_of(km):
        if not a.silhouette:
            return None
        rows = a.silhouette_rows if a.silhouette_rows is not None else (SILHOUETTE_ROWS if lat.shape[0] > SILHOUETTE_ROWS else None)
        if rows is not None and rows >= lat.shape[0]:
            rows = None
        return km.silhouette(lat, sample_size=rows, random_state=a.seed)

    if a.scan_k:
        lo, hi, step = (int(v) for v in a.scan_k.split(":"))
        curve = []
        for k in range(lo, hi, step):
            km = KMeans(n_clusters=k, init="random", n_init=10, max_iter=300, random_state=a.seed, check_every=a.check_every).fit(lat)
            sil = silhouette_of(km)
            curve.append((k, km.inertia_, sil))
            print(f"k = {k}: inertia {km.inertia_!r}" + (f", silhouette {sil!r}" if a.silhouette else ""))
        return curve
    km = KMeans(n_clusters=a.n_clusters, n_init=a.n_init, max_iter=a.max_iter, random_state=a.seed, check_every=a.check_every).fit(lat)
    out = a.out or os.path.join(os.path.dirname(os.path.abspath(a.checkpoint)), "clusters", "kmeans_model.pk")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "wb") as f:
        pickle.dump(km, f)
    print(f"n_iter: {km.n_iter_}")
    print(f"inertia: {km.inertia_!r}")
    print(f"code-usage perplexity: {km.code_perplexity()!r} of {km.n_clusters}")
    if a.silhouette:
        print(f"silhouette: {silhouette_of(km)!r}")
    print(f"wrote {out}")
    return km


if __name__ == "__main__":
    main()
