#!/usr/bin/env python
"""Times one graph-free training iteration of Part d on continuous latents (text2_embedding_discrete: False) at the shipped width
(H = 200, E = 400, S = 6, Tw = 20, no attention), the two decoder routes alternating in one process (events around each
train_iter_text2embedding call, medians):
  fused        : the fused step kernels forced (rollout_t2e.LATENT_FUSED_MIN_ROWS = 1; csrc/t2e_latent.hip)
  per_operator : one autograd node per operator and step (LATENT_FUSED_MIN_ROWS = 2^30)
  discrete     : the discrete iteration (codes, cross-entropy, K = 512) on the same box and shapes, its own route selection: scale only
for B in {128, 256, 512, 1024, 2048, 4096}.  One JSON line per batch size; the crossover these lines show is what
LATENT_FUSED_MIN_ROWS is set to.

    python tools/bench_t2e_latent.py --out profiles/t2e_latent_iteration.jsonl [--batches 128,1024] [--reps 15]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gesture2vec_amd import rollout_t2e  # noqa: E402
from gesture2vec_amd.flat import FlatClipAdam  # noqa: E402
from gesture2vec_amd.model.text2embedding_model import text2embedding_model  # noqa: E402
from gesture2vec_amd.train_eval.train_seq2seq import train_iter_text2embedding  # noqa: E402

DEV = "cuda:0"
H, L, S, TW, NW, EMB, K = 200, 2, 6, 20, 3863, 300, 512


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def build(discrete, B, seed=0):
    args = argparse.Namespace(hidden_size=H, n_layers=L, dropout_prob=0.2, autoencoder_vq_components=K, autoencoder_att="False",
                              n_pre_poses=1, n_poses=20, sentence_frame_length=20 * S, text2_embedding_discrete="True" if discrete else "False")
    torch.manual_seed(seed)
    net = text2embedding_model(args, 135, 20, NW, EMB, np.random.RandomState(0).randn(NW, EMB).astype(np.float32), None).to(DEV)
    net.train(True)
    return args, net, FlatClipAdam(net.parameters(), lr=5e-4, betas=(0.5, 0.999))


def bench_batch(B, reps, warmup):
    g = torch.Generator().manual_seed(B)
    lengths = torch.randint(4, TW + 1, (B,), generator=g).sort(descending=True).values
    lengths[0] = TW
    ids = torch.zeros(B, TW, dtype=torch.int64)
    for b in range(B):
        ids[b, : lengths[b]] = torch.randint(4, NW, (int(lengths[b]),), generator=g)
    ids = ids.to(DEV)
    lat = torch.tanh(torch.randn(B, S, L * H, generator=g)).to(DEV)
    codes = torch.randint(0, K, (B, S), generator=g).to(DEV)
    la, ln, lo = build(False, B)
    da, dn, do = build(True, B)

    def latent(min_rows):
        rollout_t2e.LATENT_FUSED_MIN_ROWS = min_rows
        return train_iter_text2embedding(la, 1, ids, lengths, None, lat, None, None, ln, lo)["loss"]

    routes = {"fused": lambda: latent(1), "per_operator": lambda: latent(1 << 30),
              "discrete": lambda: train_iter_text2embedding(da, 1, ids, lengths, None, None, codes, None, dn, do)["loss"]}
    keep = rollout_t2e.LATENT_FUSED_MIN_ROWS
    times = {k: [] for k in routes}
    try:
        for fn in routes.values():
            for _ in range(warmup):
                fn()
        calls0 = rollout_t2e.LATENT_FUSED_CALLS
        for _ in range(reps):                      # alternating: drift of the box hits every route alike
            for k, fn in routes.items():
                times[k].append(timed(fn))
        fused_calls = rollout_t2e.LATENT_FUSED_CALLS - calls0
    finally:
        rollout_t2e.LATENT_FUSED_MIN_ROWS = keep
    assert fused_calls == reps, "the fused route did not run the fused kernels"
    row = {"B": B, "H": H, "E": L * H, "S": S, "Tw": TW, "reps": reps}
    for k, v in times.items():
        row[k + "_ms"] = round(statistics.median(v), 4)
        row[k + "_ms_min"] = round(min(v), 4)
    row["fused_over_per_operator"] = round(row["fused_ms"] / row["per_operator_ms"], 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="128,256,512,1024,2048,4096")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    rows = []
    for b in a.batches.split(","):
        rows.append(bench_batch(int(b), a.reps, a.warmup))
        print(json.dumps(rows[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("".join(json.dumps(r) + "\n" for r in rows))


if __name__ == "__main__":
    main()
