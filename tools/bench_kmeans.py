#!/usr/bin/env python
"""Times the pieces of one Lloyd iteration at E = 400, alternating in one process (events around each call, medians):
  assign  : ops.vq_code_sqnorm + ops.vq_assign on the centres padded to a multiple of 16 (the exact fp32 argmin)
  update  : ops.kmeans_update (g2v_kmeans_update: inverted index, float64 chunk sums, centres, inertia, shift, state)
  stats   : the update the library had before -- ops.vq_stats (one-hot fp32 MFMA product on the padded K) and a divide
for N in {4096, 65536, 2^20} x K in {300, 512}.  One JSON line per shape; `update_frac_hbm_peak` = 4 N E bytes over 8 TB/s over
the update's time (its split into index build, chunk sums and the rest comes from a `rocprofv3 --kernel-trace --stats` run of
--only-new: the kernels are separate launches).  --fit also times a whole KMeans.fit at 2^17 x 400, K = 300 (k-means++ seeding, then Lloyd to convergence).

    python tools/bench_kmeans.py --out profiles/kmeans_lloyd.jsonl [--fit] [--only-new]"""
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
from gesture2vec_amd.kmeans import KMeans  # noqa: E402

PEAK_HBM = 8.0e12
DEV = "cuda:0"


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def mixture(N, E, K, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    cen = torch.randn(max(K // 3, 4), E, generator=g, device=DEV) * 0.3
    pick = torch.randint(0, cen.shape[0], (N,), generator=g, device=DEV)
    return torch.tanh(cen[pick] + 0.4 * torch.randn(N, E, generator=g, device=DEV)).contiguous()


def bench_shape(N, E, K, reps, only_new):
    x = mixture(N, E, K, N + K)
    km = KMeans(n_clusters=K)
    cen, sq = km._padded(K, E, DEV)
    cen[:K].copy_(x[torch.randperm(N, device=DEV)[:K]])
    Kp = cen.shape[0]
    labels = km._assign(x, cen, sq, K)
    prev = labels.clone()
    buf = ops.kmeans_update(x, labels, cen[:K], prev)
    routes = {"update": lambda: ops.kmeans_update(x, labels, cen[:K], prev, out=buf)}
    if not only_new:
        routes["assign"] = lambda: km._assign(x, cen, sq, K)
        routes["stats"] = lambda: _stats_route(labels, x, Kp)
    for fn in routes.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in routes}
    for _ in range(reps):
        for k, fn in routes.items():                                      # alternating
            times[k].append(timed(fn))
    rec = {"N": N, "E": E, "K": K, "K_padded": Kp, "reps": reps, "bytes_x": 4.0 * N * E}
    for k, v in times.items():
        rec[f"{k}_ms_median"] = statistics.median(v)
        rec[f"{k}_ms_min"] = min(v)
    rec["update_frac_hbm_peak"] = rec["bytes_x"] / PEAK_HBM / (rec["update_ms_median"] * 1e-3)
    if not only_new:
        rec["update_over_stats"] = rec["update_ms_median"] / rec["stats_ms_median"]
    return rec


def _stats_route(labels, x, Kp):
    st = ops.vq_stats(labels, x, Kp)                                       # [counts (Kp) | sums (Kp, E)] fp32
    return st[Kp:].view(Kp, -1) / st[:Kp].clamp_min(1.0)[:, None]


def bench_fit(N, E, K):
    x = mixture(N, E, K, 11)
    KMeans(n_clusters=K, max_iter=2, check_every=2).fit(x[:8192])          # warm-up of every kernel
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    km = KMeans(n_clusters=K, random_state=0, check_every=4)
    centers, _ = km._kmeans_pp(x, np.random.RandomState(0))
    torch.cuda.synchronize()
    t_seed = time.perf_counter() - t0
    t0 = time.perf_counter()
    km = KMeans(n_clusters=K, init=centers, check_every=4).fit(x)
    torch.cuda.synchronize()
    t_lloyd = time.perf_counter() - t0
    return {"fit_N": N, "E": E, "K": K, "seeding_s": t_seed, "lloyd_s": t_lloyd, "n_iter": km.n_iter_, "inertia": km.inertia_,
            "lloyd_ms_per_iter": 1e3 * t_lloyd / km.n_iter_, "perplexity": km.code_perplexity()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--fit", action="store_true")
    ap.add_argument("--only-new", action="store_true", help="the update alone (for a rocprofv3 --kernel-trace --stats run)")
    ap.add_argument("--shapes", default="4096x300,65536x300,1048576x300,4096x512,65536x512,1048576x512", help="NxK list")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: there is nothing to time on a CPU"
    recs = []
    for s in a.shapes.split(","):
        N, K = (int(v) for v in s.split("x"))
        recs.append(bench_shape(N, 400, K, 30 if N >= 2 ** 20 else 100, a.only_new))
        print(json.dumps(recs[-1]), flush=True)
    if a.fit:
        recs.append(bench_fit(2 ** 17, 400, 300))
        print(json.dumps(recs[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
