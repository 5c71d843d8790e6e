#!/usr/bin/env python
"""Times DTW k-means on the device (gesture2vec_amd/timeseries.py, csrc/dtw.hip) on planted sequences, one JSON line per shape:
  assign   : one assignment pass, ops.dtw_cdist(labels and best only) of N series against K centres
  dba_step : one barycentre step, ops.dtw_dba_accumulate + ops.dtw_dba_update, with the labels of that assignment
  fit      : TimeSeriesKMeans(K, max_iter=5, max_iter_barycenter=5).fit from init rows (the reference's call), with --fit
  host     : the float64 numpy restatement (tests/_dtw_ref.py, up to 16 host threads) of the assignment pass at --host-rows series
             of the same shape, and that time scaled to N series: an EXTRAPOLATION, labelled as such
Medians of device-synchronised host-clock times.  The shapes: 65 536 chunks of 34 poses x 135 columns against 40 centres (the
reference's call) and 65 536 x 10 x 45 (GENEA); no predecessor exists to compare with.

    python tools/bench_dtw.py --out profiles/dtw_kmeans.jsonl [--shapes 65536x34x135x40,65536x10x45x40] [--fit]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gesture2vec_amd import ops  # noqa: E402
from gesture2vec_amd.timeseries import TimeSeriesKMeans  # noqa: E402

DEV = "cuda:0"


def planted(N, T, F, K, seed=0):
    """K prototypes = tanh of a random walk; a row = a prototype read at sorted random times plus noise 0.15 (on the device)"""
    g = torch.Generator(device=DEV).manual_seed(seed + N + T)
    protos = torch.tanh(torch.cumsum(0.35 * torch.randn(K, 2 * T, F, generator=g, device=DEV), dim=1))
    which = torch.randint(0, K, (N,), generator=g, device=DEV)
    idx = torch.sort(torch.randint(0, 2 * T, (N, T), generator=g, device=DEV), dim=1).values
    idx[:, 0], idx[:, -1] = 0, 2 * T - 1
    x = protos[which[:, None], idx] + 0.15 * torch.randn(N, T, F, generator=g, device=DEV)
    return x.float().contiguous(), which


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def bench(N, T, F, K, reps, host_rows, fit):
    x, which = planted(N, T, F, K)
    centers = x[torch.randperm(N, device=DEV)[:K]].double().contiguous()
    assign = lambda: ops.dtw_cdist(x, centers, want_out=False, want_labels=True)     # noqa: E731
    _, labels, best = assign()
    members = torch.bincount(labels, minlength=K)

    def dba_step():
        c = centers.clone()
        state, _, live = ops.dtw_dba_state(K, DEV)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        acc = ops.dtw_dba_accumulate(x, labels, c, live)
        ops.dtw_dba_update(acc, members, state, c, 1e-5)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    dba_step()
    t = {"assign": [], "dba_step": []}
    for _ in range(reps):                                                    # alternating
        t["assign"].append(clock(assign)[0])
        t["dba_step"].append(dba_step())
    rec = {"N": N, "T": T, "F": F, "K": K, "reps": reps, "empty_clusters": int((members == 0).sum().item()),
           "largest_cluster": int(members.max().item()), "inertia": float(best.mean().item())}
    for name, v in t.items():
        rec[f"{name}_ms_median"] = statistics.median(v)
        rec[f"{name}_ms_min"] = min(v)
    cells = float(N) * K * T * T
    rec["assign_cost_gflops"] = 3.0 * cells * F / (rec["assign_ms_median"] * 1e-3) / 1e9      # a subtraction and a fused multiply-add
    if fit:
        first = torch.stack([torch.nonzero(which == k)[0, 0] for k in range(K)])      # one row of every prototype: no empty cluster
        init = x[first].double().cpu().numpy()
        ms, km = clock(lambda: TimeSeriesKMeans(K, max_iter=5, max_iter_barycenter=5, init=init).fit(x))
        rec["fit_ms"], rec["fit_n_iter"] = ms, km.n_iter_
    if host_rows:
        import _dtw_ref as DR
        n = min(host_rows, N)
        xs, cs = x[:n].cpu().numpy(), centers.cpu().numpy()
        t0 = time.perf_counter()
        want = DR.cdist2(xs, cs)
        ms = (time.perf_counter() - t0) * 1e3
        got = ops.dtw_cdist(x[:n].contiguous(), centers, squared=True)[0].cpu().numpy()
        rec["host_rows"], rec["host_ms_measured"] = n, ms
        rec["host_ms_extrapolated_to_N"] = ms * N / n
        rec["host_over_assign_extrapolated"] = rec["host_ms_extrapolated_to_N"] / rec["assign_ms_median"]
        rec["host_max_rel_diff"] = float(np.max(np.abs(got - want) / np.where(want > 0, want, 1.0)))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="65536x34x135x40,65536x10x45x40", help="NxTxFxK, comma separated")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-rows", dest="host_rows", type=int, default=256, help="series the host restatement is timed at; 0 leaves it out")
    ap.add_argument("--fit", action="store_true", help="also time a whole fit (max_iter = max_iter_barycenter = 5)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: there is nothing to time on a CPU"
    recs = []
    for shape in filter(None, a.shapes.split(",")):
        N, T, F, K = (int(v) for v in shape.split("x"))
        recs.append(bench(N, T, F, K, a.reps, a.host_rows, a.fit))
        print(json.dumps(recs[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
