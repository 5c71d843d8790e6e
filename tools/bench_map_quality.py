#!/usr/bin/env python
"""Times `embedding.map_quality` (trustworthiness and continuity, csrc/map_quality.hip) of an exact t-SNE map of N clustered rows,
against the PCA scores the map was made from (d = 50) and against the raw rows (d = 400), k = 5, beside the `TSNE.fit` that drew
the map.  Parts, each the median of device-synchronised host-clock times after a warm call: the two neighbour searches
(`kneighbors`), the two rank passes (`ops.neighbor_ranks`) and the whole call.  The host leg is the float64 restatement of
tests/_mapq_ref.py (two N x N float64 matrices and an argsort of each row) at --host-rows rows of the same inputs, which is about as
far as it is reasonable to hold; its scores are compared with the device's there.  One JSON line per (N, d).

    python tools/bench_map_quality.py --out profiles/map_quality.jsonl [--rows 32768] [--host-rows 4096] [--reps 5]"""
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
from gesture2vec_amd import ops  # noqa: E402
from gesture2vec_amd.embedding import PCA, TSNE, _pitch4, kneighbors, map_quality  # noqa: E402

DEV = "cuda:0"
E, D_PCA, K = 400, 50, 5


def clustered(N, seed=0):
    """16 Gaussian clusters of spread 0.5 around centres of unit entries"""
    g = torch.Generator(device=DEV).manual_seed(seed + N)
    centres = torch.randn(16, E, generator=g, device=DEV)
    which = torch.randint(0, 16, (N,), generator=g, device=DEV)
    return (centres[which] + 0.5 * torch.randn(N, E, generator=g, device=DEV)).contiguous()


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def median_ms(fn, reps):
    fn()
    times = [clock(fn)[0] for _ in range(reps)]
    return statistics.median(times), min(times), max(times)


def bench(N, reps, host_rows):
    raw = clustered(N)
    scores = PCA(D_PCA).fit_transform(raw)
    tsne = TSNE(init="random", random_state=0)
    fit_ms, _ = clock(lambda: tsne.fit(scores))
    Y = tsne.embedding_
    recs = []
    for name, X in (("pca50", scores), ("raw400", raw)):
        xs, ys = _pitch4(X), _pitch4(Y)
        me = torch.arange(N, dtype=torch.int64, device=DEV)
        nn_y, nn_x = kneighbors(Y, K, return_distance=False), kneighbors(X, K, return_distance=False)
        q = map_quality(X, Y, n_neighbors=K)
        rec = {"N": N, "d": int(X.shape[1]), "rows": name, "k": K, "reps": reps, "tsne_fit_ms": fit_ms, "tsne_n_iter": tsne.n_iter_,
               "trustworthiness": q["trustworthiness"], "continuity": q["continuity"], "redecided": q["redecided"],
               "redecided_ranks_x": int(ops.neighbor_ranks(xs, xs, nn_y, me)[1].item()),
               "redecided_ranks_y": int(ops.neighbor_ranks(ys, ys, nn_x, me)[1].item())}
        for part, fn in (("kneighbors_y", lambda: kneighbors(Y, K, return_distance=False)),
                         ("kneighbors_x", lambda: kneighbors(X, K, return_distance=False)),
                         ("ranks_x", lambda: ops.neighbor_ranks(xs, xs, nn_y, me)),
                         ("ranks_y", lambda: ops.neighbor_ranks(ys, ys, nn_x, me)),
                         ("map_quality", lambda: map_quality(X, Y, n_neighbors=K))):
            rec[f"{part}_ms_median"], rec[f"{part}_ms_min"], rec[f"{part}_ms_max"] = median_ms(fn, reps)
        rec["map_quality_over_tsne_fit"] = rec["map_quality_ms_median"] / fit_ms
        rec["ranks_x_pairs_per_s"] = float(N) * N / (rec["ranks_x_ms_median"] * 1e-3)
        if host_rows:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import _mapq_ref as MR
            n = min(N, host_rows)
            xh, yh = X[:n].contiguous(), Y[:n].contiguous()
            dev_q = map_quality(xh, yh, n_neighbors=K)
            t0 = time.perf_counter()
            ref = MR.map_quality(xh.cpu().numpy(), yh.cpu().numpy(), K)
            rec.update(host_rows=n, host_restatement_ms=(time.perf_counter() - t0) * 1e3,
                       host_trust_minus_device=ref["trustworthiness"] - dev_q["trustworthiness"],
                       host_cont_minus_device=ref["continuity"] - dev_q["continuity"],
                       device_ms_at_host_rows=median_ms(lambda: map_quality(xh, yh, n_neighbors=K), reps)[0])
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="32768")
    ap.add_argument("--host-rows", dest="host_rows", type=int, default=4096, help="rows of the host restatement; 0 leaves it out")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: there is nothing to time on a CPU"
    recs = []
    for N in (int(v) for v in a.rows.split(",")):
        recs += bench(N, a.reps, a.host_rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
