#!/usr/bin/env python
"""Times every entry of DENSE_ROUTE_SHAPES (tests/_dense_route_shapes.py: one call per route, variant and form of the dense forward
/ data-gradient plan) through the ops.* call of its form: device events around `--inner` back-to-back calls, the
median and the minimum of `--reps` such groups after `--warmup` of them, in microseconds per call.  These are launch-bound
calls (5 - 40 us), so the figure is launch + host arithmetic + kernel: what a change of the dispatch code would move.
One JSON line per entry, with the route the library names for it (absent where the library has no g2v_linear_route).

    python tools/bench_dense.py --out FILE [--root TREE] [--reps 30] [--inner 20] [--only pair]

--root: import gesture2vec_amd from that tree (another build of the library) instead of this one; the table stays this tree's."""
import argparse
import json
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner


def call_of(ops, DS, case):
    """the entry's operands on the device (seeded) -> a closure that makes the entry's call into preallocated outputs"""
    form, M, K, N = case["form"], case["M"], case["K"], case["N"]
    g = torch.Generator().manual_seed(1)
    rnd = lambda *shape: torch.randn(*shape, generator=g).to(DEV)
    w, b = rnd(N, K) * 0.2, rnd(N) if case.get("bias", True) else None
    act = case.get("act", 0)
    if form == "BWD_DATA":
        dy, out = rnd(M, N), torch.empty(M, K, device=DEV)
        return lambda: ops.linear_bwd_data(dy, w, M=M, out=out)
    rm, ldx, off = case.get("row_map"), case.get("ldx"), case.get("x_offset", 0)
    if rm is not None:
        x = rnd(rm[0], rm[1], K)
    elif ldx is not None:
        x = rnd(M, ldx)
    else:
        x = rnd(M * K + off)[off:]
    keep = (torch.rand(M, K, generator=g) < 0.8).to(torch.uint8).to(DEV) if case.get("keep") else None
    if form == "FWD":
        ldy = case.get("ldy") or N
        out = torch.empty(M, ldy, device=DEV)
        return lambda: ops.linear_fwd(x, w, b, act=act, M=M, ldx=ldx, row_map=DS.strides(K, rm), keep=keep, scale=1.25, out=out, ldy=ldy)
    Nb = case["N_b"] if form == "FWD_DUAL" else N
    wb, bb = rnd(Nb, K) * 0.2, rnd(Nb) if b is not None else None
    if form == "FWD_PAIR":
        return lambda: ops.linear_fwd_pair(x, w, b, wb, bb, act, M=M)
    x2, ya, yb = x.view(M, K), torch.empty(M, N, device=DEV), torch.empty(M, Nb, device=DEV)
    return lambda: ops.linear_fwd_dual(x2, w, b, ya, wb, bb, yb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", help="entries whose name contains this")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(HERE, "tests"))
    sys.path.insert(0, os.path.abspath(a.root))
    from gesture2vec_amd import _lib, ops  # noqa: E402
    import _dense_route_shapes as DS  # noqa: E402
    rows = []
    for case in DS.DENSE_ROUTE_SHAPES:
        if a.only not in case["name"]:
            continue
        with _lib.Context.current().scoped(smallm_rows=case.get("smallm_rows", 1024)):
            fn = call_of(ops, DS, case)
            for _ in range(a.warmup):
                timed(fn, a.inner)
            us = [timed(fn, a.inner) for _ in range(a.reps)]
            row = {"name": case["name"], "form": case["form"], "M": case["M"], "K": case["K"], "N": case["N"], "table_route": case["route"],
                   "us": round(statistics.median(us), 3), "us_min": round(min(us), 3), "reps": a.reps, "inner": a.inner}
            if hasattr(ops, "linear_route"):
                row["route"] = DS.route(**{**case, "smallm_rows": -1})
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("".join(json.dumps(r) + "\n" for r in rows))


if __name__ == "__main__":
    main()
