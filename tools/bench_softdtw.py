#!/usr/bin/env python
"""Times soft-DTW on the device (gesture2vec_amd/timeseries.py, csrc/softdtw.hip) on planted sequences, one JSON line per shape:
  assign     : one assignment pass, ops.softdtw_cdist(labels and best only) of N series against K centres, and beside it
  dtw_assign : ops.dtw_cdist at the same shape (the parent's pass)
  grad       : one ops.softdtw_grad evaluation (value and gradient of one centre) over a cluster of N / K member rows, read back
               to the host as the optimiser reads it
  fit        : SoftDTWKMeans(K, max_iter=5, max_iter_barycenter=5, gamma).fit from init rows (the reference's call), with --fit:
               wall time, function evaluations, and the share of the wall time the device is NOT busy, estimated as
               1 - (assignments x assign + evaluations x the device-only time of a grad launch set of N / K rows) / wall
  host       : the float64 numpy restatement (tests/_softdtw_ref.py) of the assignment pass at --host-rows series of the same shape,
               and that time scaled to N series: an EXTRAPOLATION, labelled as such
Medians of device-synchronised host-clock times.

    python tools/bench_softdtw.py --out profiles/softdtw_kmeans.jsonl [--shapes 65536x34x135x40] [--gamma 0.5] [--fit]"""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_dtw import clock, planted  # noqa: E402
from gesture2vec_amd import ops  # noqa: E402
from gesture2vec_amd.timeseries import SoftDTWKMeans  # noqa: E402

DEV = "cuda:0"


def bench(N, T, F, K, gamma, reps, host_rows, fit):
    x, which = planted(N, T, F, K)
    centers = x[torch.randperm(N, device=DEV)[:K]].double().contiguous()
    assign = lambda: ops.softdtw_cdist(x, centers, gamma, want_out=False, want_labels=True)      # noqa: E731
    dtw_assign = lambda: ops.dtw_cdist(x, centers, want_out=False, want_labels=True)             # noqa: E731
    rows = torch.arange(0, N, K, dtype=torch.int64, device=DEV)                                  # N / K member rows
    out = torch.empty((1 + T * F,), dtype=torch.float64, device=DEV)
    z = centers[0].contiguous()
    grad_dev = lambda: ops.softdtw_grad(x, rows, z, gamma, out=out)                              # noqa: E731
    grad = lambda: (ops.softdtw_grad(x, rows, z, gamma, out=out), out.cpu())                     # noqa: E731
    _, labels, best = assign()
    dtw_assign(), grad()
    t = {"assign": [], "dtw_assign": [], "grad": [], "grad_device": []}
    for _ in range(reps):                                                    # alternating
        t["assign"].append(clock(assign)[0])
        t["dtw_assign"].append(clock(dtw_assign)[0])
        t["grad"].append(clock(grad)[0])
        t["grad_device"].append(clock(grad_dev)[0])
    rec = {"N": N, "T": T, "F": F, "K": K, "gamma": gamma, "reps": reps, "grad_rows": int(rows.numel()),
           "inertia": float(best.mean().item())}
    for name, v in t.items():
        rec[f"{name}_ms_median"] = statistics.median(v)
        rec[f"{name}_ms_min"] = min(v)
    rec["assign_over_dtw_assign"] = rec["assign_ms_median"] / rec["dtw_assign_ms_median"]
    if fit:
        first = torch.stack([torch.nonzero(which == k)[0, 0] for k in range(K)])      # one row of every prototype: no empty cluster
        init = x[first].double().cpu().numpy()
        ms, km = clock(lambda: SoftDTWKMeans(K, max_iter=5, max_iter_barycenter=5, gamma=gamma, init=init).fit(x))
        nfev = int(sum(int(e.sum()) for e in km.nfev_))
        busy = km.n_iter_ * rec["assign_ms_median"] + nfev * rec["grad_device_ms_median"]
        rec.update(fit_ms=ms, fit_n_iter=km.n_iter_, fit_nfev=nfev, fit_device_busy_ms_estimate=busy,
                   fit_device_idle_share_estimate=max(0.0, 1.0 - busy / ms))
    if host_rows:
        import _softdtw_ref as SR
        n = min(host_rows, N)
        xs, cs = x[:n].cpu().numpy(), centers.cpu().numpy()
        t0 = time.perf_counter()
        want, maxR = SR.cdist(xs, cs, gamma)
        ms = (time.perf_counter() - t0) * 1e3
        got = ops.softdtw_cdist(x[:n].contiguous(), centers, gamma)[0].cpu().numpy()
        rec["host_rows"], rec["host_ms_measured"] = n, ms
        rec["host_ms_extrapolated_to_N"] = ms * N / n
        rec["host_over_assign_extrapolated"] = rec["host_ms_extrapolated_to_N"] / rec["assign_ms_median"]
        rec["host_max_diff_in_bars"] = float(np.max(np.abs(got - want) / SR.tol_R(T, T, maxR, gamma)))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="65536x34x135x40", help="NxTxFxK, comma separated")
    ap.add_argument("--gamma", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-rows", dest="host_rows", type=int, default=256, help="series the host restatement is timed at; 0 leaves it out")
    ap.add_argument("--fit", action="store_true", help="also time a whole fit (max_iter = max_iter_barycenter = 5)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: there is nothing to time on a CPU"
    recs = []
    for shape in filter(None, a.shapes.split(",")):
        N, T, F, K = (int(v) for v in shape.split("x"))
        recs.append(bench(N, T, F, K, a.gamma, a.reps, a.host_rows, a.fit))
        print(json.dumps(recs[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
