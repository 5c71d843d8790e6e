#!/usr/bin/env python
"""Times the pairwise-distance statistics (gesture2vec_amd/repdist.py, csrc/pair_stats.hip) on blob latents of width E = 400:
  pair_stats : one g2v_pair_stats call without bins (both norm launches, the pair pass, the fold) and one with 64 bins
  lag        : g2v_lag_distances with lags (1, 2)
  report     : representation_report, everything the reference's calculate_distances computes, read-backs included
against the routes a user has without the kernel, alternating in one process:
  cdist      : `torch.cdist(x64[a:b], x64)` over row blocks on float64 copies of the rows (made outside the timed region), the
               upper triangle summed on the device: what one would write to get np.mean(pdist(x)) without storing the pairs
  pdist      : `scipy.spatial.distance.pdist(x).mean()` on the host (--pdist-rows, where scipy is installed and the N (N - 1) / 2
               float64 values fit; timed once per N, the read-back of the rows included); skipped by name otherwise
One JSON line per N: medians of device-event times, the relative difference of the means, and the pair_stats call in TFLOP/s of the
executed tiles (2 * 64^2 * E16 per tile on or above the diagonal, as tools/bench_ward.py counts them) and as a fraction of the float64
matrix peak of the MI355X's data sheet, 78.6 TFLOP/s.  The split of the call into its kernels comes from a run of
`rocprofv3 --kernel-trace --stats -- python tools/bench_pair_stats.py --only-new --rows N`.

    python tools/bench_pair_stats.py --out profiles/pair_stats.jsonl [--rows 4096,32768,131072] [--pdist-rows 4096,16384]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gesture2vec_amd import ops, repdist  # noqa: E402

PEAK_F64_MFMA = 78.6e12
DEV = "cuda:0"
E = 400


def blob_latents(N, seed=0):
    """N / 64 (>= 2) blobs of unit spread around centres drawn 3 wide (the rows of tools/bench_ward.py)"""
    g = torch.Generator(device=DEV).manual_seed(seed + N)
    k = max(2, N // 64)
    centres = 3.0 * torch.randn(k, E, generator=g, device=DEV)
    which = torch.randint(0, k, (N,), generator=g, device=DEV)
    return (centres[which] + torch.randn(N, E, generator=g, device=DEV)).contiguous()


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def cdist_mean(x64, block):
    """sum_{i<j} |x_i - x_j| / pairs without holding more than `block` rows of the matrix"""
    N = x64.shape[0]
    total = torch.zeros((), dtype=torch.float64, device=DEV)
    for a in range(0, N, block):
        d = torch.cdist(x64[a:a + block], x64)
        total += d.triu(diagonal=a + 1).sum()
    return total / (N * (N - 1) / 2)


def bench(N, reps, pdist_rows):
    x = blob_latents(N)
    x64 = x.double()
    block = max(256, min(N, (1 << 29) // N))                                 # at most 4 GiB of float64 distances at a time
    edges = torch.linspace(0.0, 120.0, 65, dtype=torch.float64, device=DEV)
    for _ in range(2):                                                       # warm-up of every kernel at the shape
        ops.pair_stats(x)
        ops.pair_stats(x, None, edges)
        ops.lag_distances(x, (1, 2))
        cdist_mean(x64, block)
    t = {k: [] for k in ("pair_stats", "pair_stats_64bins", "lag", "cdist_f64", "report")}
    for _ in range(reps):                                                    # alternating
        ms, (out, counts, _) = event_ms(lambda: ops.pair_stats(x))
        t["pair_stats"].append(ms)
        ms, ref = event_ms(lambda: cdist_mean(x64, block))
        t["cdist_f64"].append(ms)
        ms, _ = event_ms(lambda: ops.pair_stats(x, None, edges))
        t["pair_stats_64bins"].append(ms)
        ms, _ = event_ms(lambda: ops.lag_distances(x, (1, 2)))
        t["lag"].append(ms)
        ms, _ = event_ms(lambda: repdist.representation_report(x, seed=0))
        t["report"].append(ms)
    mean = float(out[0]) / int(counts[0])
    rec = {"N": N, "E": E, "reps": reps, "pairs": int(counts[0]), "run": ops.pair_stats_run(N), "cdist_block_rows": block,
           "workspace_MiB": ops.pair_stats_workspace(N, 0, E, 64) / 2 ** 20, "pdist_would_store_GiB": N * (N - 1) / 2 * 8 / 2 ** 30,
           "mean": mean, "cdist_mean_rel_diff": abs(float(ref) - mean) / mean}
    for k, v in t.items():
        rec[f"{k}_ms_median"] = statistics.median(v)
        rec[f"{k}_ms_min"] = min(v)
    W = (N + 63) // 64
    flop = 2.0 * 64 * 64 * ((E + 15) // 16 * 16) * (W * (W + 1) // 2)
    rec["pair_stats_tflops"] = flop / (rec["pair_stats_ms_median"] * 1e-3) / 1e12
    rec["pair_stats_frac_f64_mfma_peak"] = rec["pair_stats_tflops"] * 1e12 / PEAK_F64_MFMA
    rec["cdist_over_pair_stats"] = rec["cdist_f64_ms_median"] / rec["pair_stats_ms_median"]
    if N in pdist_rows:
        try:
            from scipy.spatial.distance import pdist
        except ImportError:
            rec["pdist"] = "skipped: scipy is not installed here"
        else:
            t0 = time.perf_counter()
            host = float(pdist(x.cpu().numpy().astype("float64")).mean())
            rec["pdist_ms"] = (time.perf_counter() - t0) * 1e3
            rec["pdist_mean_rel_diff"] = abs(host - mean) / mean
            rec["pdist_over_pair_stats"] = rec["pdist_ms"] / rec["pair_stats_ms_median"]
    else:
        rec["pdist"] = "skipped: not among --pdist-rows" if N <= 16384 else "skipped: the N (N - 1) / 2 float64 distances are not held on the host at this N"
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="4096,32768,131072")
    ap.add_argument("--pdist-rows", dest="pdist_rows", default="4096,16384", help="rows scipy's pdist is run at; '' leaves it out")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only-new", action="store_true", help="the kernels alone (for a rocprofv3 --kernel-trace --stats run)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: there is nothing to time on a CPU"
    pdist_rows = [int(v) for v in filter(None, a.pdist_rows.split(","))]
    rows = sorted(set(int(v) for v in filter(None, a.rows.split(","))) | (set() if a.only_new else set(pdist_rows)))
    if a.only_new:
        for N in rows:
            x = blob_latents(N)
            for _ in range(a.reps):
                ops.pair_stats(x)
                ops.lag_distances(x, (1, 2))
            torch.cuda.synchronize()
        return
    recs = []
    for N in rows:
        recs.append(bench(N, a.reps if N <= 32768 else max(5, a.reps - 2), pdist_rows))
        print(json.dumps(recs[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
