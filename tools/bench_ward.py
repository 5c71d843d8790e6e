#!/usr/bin/env python
"""Times Ward clustering on the device (gesture2vec_amd/agglomerative.py) on blob latents of width E = 400, alternating in one
process:
  distances: g2v_ward_distances (float64 Gram tiles on v_mfma_f64_16x16x4_f64, the upper triangle computed and mirrored) against
             `torch.cdist` on float64 copies of the same rows (the copies are made outside the timed region)
  fit      : AgglomerativeClustering(n_clusters).fit, split into the distance pass, all rounds with their read-backs and the host's
             tree bookkeeping (sort, relabelling, cut), with the rounds per fit
  scipy    : `scipy.cluster.hierarchy.ward` on the host on the same rows, the read-back of the rows included (--scipy-rows: sizes the
             host finishes; timed once per N), and whether its merges equal the device's
One JSON line per N: medians of device-synchronised host-clock times.  The distance pass is also given in TFLOP/s of the executed
tiles, 2 * 64^2 * E16 per tile on or above the diagonal.

    python tools/bench_ward.py --out profiles/ward.jsonl [--rows 2048,8192,32768] [--scipy-rows 2048,8192]"""
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
from gesture2vec_amd.agglomerative import AgglomerativeClustering, hc_cut, tree_from_log  # noqa: E402

DEV = "cuda:0"
E, K = 400, 300


def blob_latents(N, seed=0):
    """N / 64 (>= 2) blobs of unit spread around centres drawn 3 wide"""
    g = torch.Generator(device=DEV).manual_seed(seed + N)
    k = max(2, N // 64)
    centres = 3.0 * torch.randn(k, E, generator=g, device=DEV)
    which = torch.randint(0, k, (N,), generator=g, device=DEV)
    return (centres[which] + torch.randn(N, E, generator=g, device=DEV)).contiguous()


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def run_rounds(D, check_every=4):
    N = D.shape[0]
    state = ops.ward_state(N, DEV)
    first = True
    while True:
        c = ops.ward_rounds(D, state, init=first, rounds=check_every).cpu().numpy()
        first = False
        if c[0] >= N - 1:
            return state, int(c[1])


def host_tree(state, N, k):
    children, heights = tree_from_log(state["pairs"].cpu().numpy(), state["heights"].cpu().numpy(), N)
    return children, heights, hc_cut(k, children, N)


def bench(N, reps, scipy_rows):
    x = blob_latents(N)
    k = min(K, N)
    x64 = x.double()
    for _ in range(2):                                                       # warm-up of every kernel at the shape
        D = ops.ward_distances(x)
        run_rounds(D)
        del D
        ref = torch.cdist(x64, x64)
    t = {name: [] for name in ("distances", "cdist_f64", "rounds", "host_tree", "fit")}
    for _ in range(reps):                                                    # alternating
        ms, D = clock(lambda: ops.ward_distances(x))
        t["distances"].append(ms)
        ms, ref = clock(lambda: torch.cdist(x64, x64))
        t["cdist_f64"].append(ms)
        ms, (state, rounds) = clock(lambda: run_rounds(D))
        t["rounds"].append(ms)
        del D
        ms, (children, heights, labels) = clock(lambda: host_tree(state, N, k))
        t["host_tree"].append(ms)
        ms, ac = clock(lambda: AgglomerativeClustering(k, compute_distances=True).fit(x))
        t["fit"].append(ms)
    D = ops.ward_distances(x)
    off = ~torch.eye(N, dtype=torch.bool, device=DEV)
    rel = float(((D - ref).abs() / D)[off & (D > 0)].max().item())
    del D, ref
    rec = {"N": N, "E": E, "n_clusters": k, "reps": reps, "rounds": rounds, "matrix_MiB": N * N * 8 / 2 ** 20,
           "fit_equals_parts": bool(np.array_equal(ac.children_, children) and np.array_equal(ac.labels_.cpu().numpy(), labels)),
           "cdist_max_rel_diff": rel}
    for name, v in t.items():
        rec[f"{name}_ms_median"] = statistics.median(v)
        rec[f"{name}_ms_min"] = min(v)
    W = (N + 63) // 64
    flop = 2.0 * 64 * 64 * ((E + 15) // 16 * 16) * (W * (W + 1) // 2)
    rec["distances_tflops"] = flop / (rec["distances_ms_median"] * 1e-3) / 1e12
    rec["cdist_over_distances"] = rec["cdist_f64_ms_median"] / rec["distances_ms_median"]
    if N in scipy_rows:
        from scipy.cluster.hierarchy import ward
        t0 = time.perf_counter()
        Z = ward(x.cpu().numpy())
        rec["scipy_ms"] = (time.perf_counter() - t0) * 1e3
        rec["scipy_children_equal"] = bool(np.array_equal(Z[:, :2].astype(np.int64), children))
        rec["scipy_heights_max_rel_diff"] = float(np.max(np.abs(Z[:, 2] - heights) / Z[:, 2]))
        rec["scipy_over_fit"] = rec["scipy_ms"] / rec["fit_ms_median"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="2048,8192,32768")
    ap.add_argument("--scipy-rows", dest="scipy_rows", default="2048,8192", help="rows scipy is run at; '' leaves it out")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: there is nothing to time on a CPU"
    scipy_rows = [int(v) for v in filter(None, a.scipy_rows.split(","))]
    rows = sorted(set(int(v) for v in filter(None, a.rows.split(","))) | set(scipy_rows))
    recs = []
    for N in rows:
        recs.append(bench(N, a.reps if N <= 8192 else max(2, a.reps // 2), scipy_rows))
        print(json.dumps(recs[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
