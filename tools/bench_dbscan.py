#!/usr/bin/env python
"""Times DBSCAN.fit (gesture2vec_amd/dbscan.py) on blob latents of width E = 400, split into the neighbour pass
(g2v_dbscan_neighbors), all propagation rounds with their read-backs (g2v_dbscan_propagate) and the labelling (g2v_dbscan_labels),
against the two routes a user has without the neighbour kernel, alternating in one process:
  cdist  : chunked `torch.cdist(x[a:b], x) <= eps` on the device, row sums, the bits packed into the same bitmap, then the same
           propagation and labelling kernels
  sklearn: `sklearn.cluster.DBSCAN(eps, min_samples, n_jobs=16).fit` on the host on the same rows, the read-back of the rows included
           (--sklearn-rows; timed once per N, and scaled by (N / n)^2 from the largest n that was run where N itself was not)
One JSON line per N: medians of device-synchronised host-clock times, whether each route's labels equal the kernel route's, and the
neighbour pass as a fraction of the exact-fp32 MFMA peak: the 2 (64 W)^2 E16 FLOP of the executed tiles over 157.3 TF/s.

    python tools/bench_dbscan.py --out profiles/dbscan.jsonl [--rows 4096,32768,65536] [--sklearn-rows 4096,16384]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gesture2vec_amd import ops  # noqa: E402
from gesture2vec_amd.dbscan import DBSCAN  # noqa: E402

PEAK_F32_MFMA = 157.3e12
DEV = "cuda:0"
E, EPS, MIN_SAMPLES = 400, 7.3, 5


def blob_latents(N, seed=0):
    """N / 256 blobs of spread 0.25 around centres of unit entries (pairs inside a blob are 7.07 +- 0.18 apart, 90 % of them within
    eps = 7.3; blobs are 28 apart) and one row in twenty on its own"""
    g = torch.Generator(device=DEV).manual_seed(seed + N)
    K = max(2, N // 256)
    centres = torch.randn(K, E, generator=g, device=DEV)
    which = torch.randint(0, K, (N,), generator=g, device=DEV)
    x = centres[which] + 0.25 * torch.randn(N, E, generator=g, device=DEV)
    alone = torch.rand(N, generator=g, device=DEV) < 0.05
    x[alone] = torch.randn(int(alone.sum().item()), E, generator=g, device=DEV)
    return x.contiguous()


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def propagate(bitmap, counts, check_every=4):
    N = bitmap.shape[0]
    L = torch.empty((N,), dtype=torch.int32, device=DEV)
    tmp = torch.empty_like(L)
    rounds, first = 0, True
    while True:
        flags = ops.dbscan_propagate(bitmap, counts, MIN_SAMPLES, L, tmp, init=first, rounds=check_every).cpu().numpy()
        first = False
        still = np.nonzero(flags == 0)[0]
        if len(still):
            return L, rounds + int(still[0]) + 1
        rounds += len(flags)


def cdist_bitmap(x, chunk=4096):
    N = x.shape[0]
    W = (N + 63) // 64
    bitmap = torch.empty((N, W), dtype=torch.int64, device=DEV)
    counts = torch.empty((N,), dtype=torch.int64, device=DEV)
    weights = torch.ones(64, dtype=torch.int64, device=DEV) << torch.arange(64, dtype=torch.int64, device=DEV)
    for a in range(0, N, chunk):
        adj = torch.cdist(x[a:a + chunk], x) <= EPS
        counts[a:a + chunk] = adj.sum(1)
        if N % 64:
            adj = torch.nn.functional.pad(adj, (0, 64 * W - N))
        bitmap[a:a + chunk] = (adj.view(-1, W, 64).to(torch.int64) * weights).sum(-1)
    return bitmap, counts


def bench(N, reps, sk_times):
    x = blob_latents(N)
    W = (N + 63) // 64
    for _ in range(2):                                                       # warm-up of every kernel at the shape
        bitmap, counts = ops.dbscan_neighbors(x, EPS)
        L, rounds = propagate(bitmap, counts)
        labels, core, out = ops.dbscan_labels(bitmap, L)
        cdist_bitmap(x)
    t = {k: [] for k in ("neighbors", "propagate", "labels", "fit", "cdist_adjacency", "cdist_fit")}
    for _ in range(reps):                                                    # alternating
        ms, (bitmap, counts) = clock(lambda: ops.dbscan_neighbors(x, EPS))
        t["neighbors"].append(ms)
        ms, (L, rounds) = clock(lambda: propagate(bitmap, counts))
        t["propagate"].append(ms)
        ms, (labels, core, out) = clock(lambda: ops.dbscan_labels(bitmap, L))
        t["labels"].append(ms)
        ms, db = clock(lambda: DBSCAN(EPS, MIN_SAMPLES).fit(x))
        t["fit"].append(ms)
        del bitmap
        ms, (bm2, cnt2) = clock(lambda: cdist_bitmap(x))
        t["cdist_adjacency"].append(ms)
        ms2, (L2, _) = clock(lambda: propagate(bm2, cnt2))
        ms3, (labels2, _, _) = clock(lambda: ops.dbscan_labels(bm2, L2))
        t["cdist_fit"].append(ms + ms2 + ms3)
        del bm2
    n_clusters, n_core, n_noise = (int(v) for v in out.cpu().numpy())
    rec = {"N": N, "E": E, "eps": EPS, "min_samples": MIN_SAMPLES, "reps": reps, "clusters": n_clusters, "core": n_core, "noise": n_noise,
           "rounds": rounds, "bitmap_MiB": N * W * 8 / 2 ** 20, "fit_labels_equal_parts": bool(torch.equal(db.labels_, labels)),
           "cdist_labels_equal": bool(torch.equal(labels2, labels))}
    for k, v in t.items():
        rec[f"{k}_ms_median"] = statistics.median(v)
        rec[f"{k}_ms_min"] = min(v)
    flop = 2.0 * (64 * W) ** 2 * ((E + 15) // 16 * 16)
    rec["neighbors_frac_mfma_f32_peak"] = flop / PEAK_F32_MFMA / (rec["neighbors_ms_median"] * 1e-3)
    rec["cdist_fit_over_fit"] = rec["cdist_fit_ms_median"] / rec["fit_ms_median"]
    if N in sk_times["rows"] or any(isinstance(k, int) for k in sk_times):
        from sklearn.cluster import DBSCAN as SK
        if N in sk_times["rows"]:
            t0 = time.perf_counter()
            sk = SK(eps=EPS, min_samples=MIN_SAMPLES, n_jobs=16).fit(x.cpu().numpy())
            sk_times[N] = (time.perf_counter() - t0) * 1e3
            rec["sklearn_ms"] = sk_times[N]
            rec["sklearn_labels_equal"] = bool(np.array_equal(sk.labels_, labels.cpu().numpy()))
        else:
            n = max(k for k in sk_times if isinstance(k, int))
            rec["sklearn_ms_scaled_from"] = n
            rec["sklearn_ms"] = sk_times[n] * (N / n) ** 2
        rec["sklearn_over_fit"] = rec["sklearn_ms"] / rec["fit_ms_median"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="4096,32768,65536")
    ap.add_argument("--sklearn-rows", dest="sklearn_rows", default="4096,16384", help="rows sklearn is run at; '' leaves it out")
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: there is nothing to time on a CPU"
    sk_rows = [int(v) for v in filter(None, a.sklearn_rows.split(","))]
    rows = sorted(set(int(v) for v in filter(None, a.rows.split(","))) | set(sk_rows))
    sk_times = {"rows": sk_rows}
    recs = []
    for N in rows:
        recs.append(bench(N, a.reps if N <= 32768 else max(3, a.reps // 2), sk_times))
        print(json.dumps(recs[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
