#!/usr/bin/env python3
"""Times the two routes of the frame-level quantised autoencoder (VQ_Frame) against each other on the device, in one process:

    python scripts/time_vq_frame.py [--iters 300] [--rounds 5] [--out FILE.json]

  * train_iter_DAE (keep mask + step + clip/Adam + the loss read-back) per iteration at (B, D, L, K) = (16, 135, 40, 80),
    (128, 135, 40, 80), (256, 135, 40, 80), (256, 135, 45, 128) and (1024, 135, 200, 100) -- the last on the staged route only
    where the plan does not admit the fused step;
  * VQ_Frame.codes over 1024, 65536 and 2^20 frames at (135, 40, 80) and (135, 200, 100): the grid kernel against the staged eval
    forward.
The routes alternate round by round inside one timed loop each (device events around `iters` iterations after a warm-up); the
figure reported per route is the median of the rounds, with the spread (min, max) beside it.  One JSON line per measurement.
`--kernel-only ITERS` runs just the fused calls (for a kernel trace taken in a run of its own)."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
for _p in (_HERE, _ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from gesture2vec_amd import ops  # noqa: E402
from gesture2vec_amd.flat import FlatClipAdam  # noqa: E402
from gesture2vec_amd.model.DAE_model import VQ_Frame  # noqa: E402
from gesture2vec_amd.train_eval.train_seq2seq import train_iter_DAE  # noqa: E402
from utils.route_timing import compare  # noqa: E402

DEV = "cuda:0"
ARGS = argparse.Namespace(autoencoder_vq="True", autoencoder_vae="False")


def model(shape, route, training):
    B, D, L, K = shape
    torch.manual_seed(0)
    net = VQ_Frame(D, L, False, K)
    q = net.vq_layer                               # a warm quantiser: the codebook does not blow up inside the timed window
    q._embedding.weight.data.normal_()
    q._ema_cluster_size.fill_(B / K)
    q._ema_w.data.copy_(q._embedding.weight.data * (B / K))
    net = net.to(DEV)
    net.train(training)
    net.route = route
    return net


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", type=int, nargs="+", default=[1024, 65536, 1 << 20])
    ap.add_argument("--out", default="")
    ap.add_argument("--kernel-only", type=int, default=0)
    cli = ap.parse_args()
    lines = []

    def emit(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    for shape in ((16, 135, 40, 80), (128, 135, 40, 80), (256, 135, 40, 80), (256, 135, 45, 128), (1024, 135, 200, 100)):
        B, D, L, K = shape
        _, fused_ok, reason = ops.vqframe_plan(B, D, L, K, True)
        x = torch.randn(B, D, 1, device=DEV)
        noisy = x + 0.1 * torch.randn_like(x)
        fns = {}
        for route in (("fused", "staged") if fused_ok else ("staged",)):
            if cli.kernel_only and route != "fused":
                continue
            net = model(shape, route, True)
            optim = FlatClipAdam(net.parameters(), lr=5e-4, betas=(0.5, 0.999))
            fns[route] = (lambda net=net, optim=optim: train_iter_DAE(ARGS, 1, noisy, x, net, optim))
        if cli.kernel_only:
            for fn in fns.values():
                for _ in range(cli.kernel_only):
                    fn()
            continue
        emit(what="train_iter_DAE", shape=shape, iters=cli.iters, rounds=cli.rounds, fused_admitted=fused_ok, plan=reason,
             **compare(fns, cli.iters, cli.rounds, 30))
    for dims in ((135, 40, 80), (135, 200, 100)):
        D, L, K = dims
        nets = {route: model((128, D, L, K), route, False) for route in ("fused", "staged")}
        for rows in cli.rows:
            x = torch.randn(rows, D, device=DEV)
            fns = {route: (lambda net=net: net.codes(x)) for route, net in nets.items()}
            if cli.kernel_only:
                for _ in range(max(1, cli.kernel_only // 10)):
                    fns["fused"]()
                continue
            a, b = (fn() for fn in fns.values())
            emit(what="codes", rows=rows, dims=dims, ids_differ=int((a != b).sum()),
                 **compare(fns, 10 if rows > 100000 else 200, cli.rounds, 3))
    torch.cuda.synchronize()
    if cli.out:
        with open(cli.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
