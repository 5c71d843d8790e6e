#!/usr/bin/env python
"""Times generate.decode_codes on its two routes, alternating in one process (device events around each warmed call, medians):
  chain   : g2v_dec_chain_fwd, the whole chain of every clip in one launch (csrc/dec_chain.hip)
  rollout : one eval-mode g2v_dec_rollout_fwd per chunk -- the kernels the tree had before the chain kernel: the yardstick
for (B, C) in {(1, 60), (128, 12), (4096, 6)} x (D, H, T) in {(40, 200, 20), (135, 64, 34)}, five warm-up steps per chunk.
The masks of the inline Dropout(0.95) are drawn once, outside the timed calls (keep probability 0.05, as in use), so both routes
decode the same thing; their outputs are compared before anything is timed.  One JSON line per shape: both times, the chain's
time per decoder step (C (warmup + T - 1) serial steps) and, at H = 200, that step time over the 25.8 us MFMA floor of a decoder
step at B = 4096.  generate.AUTO_CHAIN_MIN_CLIPS is set from this table.

    python tools/bench_generate.py --out profiles/generate_routes.jsonl"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gesture2vec_amd import generate, ops  # noqa: E402
from gesture2vec_amd.model.Autoencoder_VQVAE_model import Autoencoder_VQVAE  # noqa: E402

DEV = "cuda:0"
MFMA_FLOOR_US_H200_B4096 = 25.8
WARMUP_STEPS = 5


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def make_net(D, H, T, K=512):
    args = argparse.Namespace(rep_learning_dim=D, hidden_size=H, n_layers=2, dropout_prob=0.0, autoencoder_vae="False",
                              autoencoder_vq="True", autoencoder_vq_components=K, autoencoder_vq_commitment_cost=0.25, n_pre_poses=1,
                              autoencoder_conditioned="True", autoencoder_att="False", autoencoder_fixed_weight="False", n_poses=T,
                              loss_l1_weight=5.0, loss_cont_weight=0.1, loss_var_weight=0.5, learning_rate=5e-4, epochs=10)
    torch.manual_seed(D + H)
    net = Autoencoder_VQVAE(args, D, T).to(DEV).eval()
    bn = net.decoder.decoder.pre_linear[1]
    bn.running_mean.normal_(0.0, 0.1)
    bn.running_var.uniform_(0.5, 1.5)
    return net


def bench_shape(B, C, D, H, T, reps):
    net = make_net(D, H, T)
    g = torch.Generator(device=DEV).manual_seed(B + C)
    codes = torch.randint(0, net.vq_components, (B, C), generator=g, device=DEV)
    start = torch.randn(B, D, generator=g, device=DEV)
    S = WARMUP_STEPS + T - 1
    keep95 = ops.keep_mask(torch.empty((C, S, B, D), dtype=torch.uint8, device=DEV), 0.05, 7, torch.zeros(1, dtype=torch.int64, device=DEV))
    routes = {r: (lambda r=r: generate.decode_codes(net, codes, start=start, keep95=keep95, warmup=WARMUP_STEPS, route=r))
              for r in ("chain", "rollout")}
    outs = {}
    for r, fn in routes.items():
        for _ in range(3):
            outs[r] = fn()
    torch.cuda.synchronize()
    scale = float(outs["rollout"].abs().max())
    diff = float((outs["chain"] - outs["rollout"]).abs().max()) / scale
    times = {r: [] for r in routes}
    for _ in range(reps):
        for r, fn in routes.items():                                      # alternating
            times[r].append(timed(fn))
    steps = C * S
    rec = {"B": B, "C": C, "D": D, "H": H, "T": T, "warmup": WARMUP_STEPS, "steps": steps, "reps": reps, "routes_max_rel_diff": diff}
    for r, v in times.items():
        rec[f"{r}_ms_median"] = statistics.median(v)
        rec[f"{r}_ms_min"] = min(v)
    rec["chain_over_rollout"] = rec["chain_ms_median"] / rec["rollout_ms_median"]
    rec["chain_us_per_step"] = 1e3 * rec["chain_ms_median"] / steps
    rec["rollout_us_per_step"] = 1e3 * rec["rollout_ms_median"] / steps
    if H == 200 and B == 4096:
        rec["chain_step_over_mfma_floor"] = rec["chain_us_per_step"] / MFMA_FLOOR_US_H200_B4096
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="1x60,128x12,4096x6", help="BxC list")
    ap.add_argument("--dims", default="40x200x20,135x64x34", help="DxHxT list")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: there is nothing to time on a CPU"
    recs = []
    for dims in a.dims.split(","):
        D, H, T = (int(v) for v in dims.split("x"))
        for s in a.shapes.split(","):
            B, C = (int(v) for v in s.split("x"))
            recs.append(bench_shape(B, C, D, H, T, a.reps))
            print(json.dumps(recs[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
