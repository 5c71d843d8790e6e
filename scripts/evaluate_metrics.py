#!/usr/bin/env python3
"""Scores a generated gesture set against the ground truth with the table columns of the reference's
`scripts/Clustering.py::Metrics_analysis`, on the MI355X kernels (gesture2vec_amd/metrics.py).

    python evaluate_metrics.py --checkpoint vqvae_checkpoint.bin [--dae_checkpoint dae_checkpoint.bin] --real x.npy --generated y.npy

Both arrays hold (N, T, D) pose chunks: D = the chunk autoencoder's `rep_learning_dim`, or the raw pose dimension when a DAE
checkpoint is given (frames then go through its encoder first, as in `stacked_autoencode`).  Prints the four numbers in the order of
the reference's Metrics.txt lines (:1546-1558); the code metrics read "None" for a checkpoint without a quantiser.

    ... --real_clips a.npy --generated_clips b.npy        (or --clip_chunks N: every clip holds N chunks)

adds the BLEU line (:1601-1608): the code sequence of generated clip i scored against that of real clip i.  Both .npy files hold
the number of consecutive chunks of each clip.

    ... --energy

adds one line, `Energy distance --> v`: the energy distance between the two sets' latents (gesture2vec_amd.metrics.energy_distance),
a two-sample distance that assumes no Gaussians; not a reference column.  t-SNE, k-means and the plots of `Metrics_analysis` are not computed."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
for _p in (_HERE, _ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from utils.train_utils import load_checkpoint_and_model  # noqa: E402
from gesture2vec_amd.metrics import energy_distance, gesture_metrics, set_latents  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--checkpoint", required=True, help="chunk autoencoder checkpoint (train_autoencoder_VQVAE.py)")
    ap.add_argument("--dae_checkpoint", default=None, help="frame DAE checkpoint (train_DAE.py): chunks are raw poses")
    ap.add_argument("--real", required=True, help=".npy of (N, T, D) ground-truth chunks")
    ap.add_argument("--generated", required=True, help=".npy of (N, T, D) generated chunks")
    ap.add_argument("--real_clips", default=None, help=".npy of ints: chunks per ground-truth clip (adds the BLEU line)")
    ap.add_argument("--generated_clips", default=None, help=".npy of ints: chunks per generated clip")
    ap.add_argument("--clip_chunks", type=int, default=None, help="shorthand: every clip of both sets holds this many chunks")
    ap.add_argument("--energy", action="store_true", help="add the energy distance between the two sets' latents (one more line)")
    ap.add_argument("--batch_rows", type=int, default=65536)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    dev = torch.device(a.device)
    _, net, _, _, _ = load_checkpoint_and_model(a.checkpoint, dev, "autoencoder_vq")
    dae = None
    if a.dae_checkpoint:
        _, dae, _, _, _ = load_checkpoint_and_model(a.dae_checkpoint, dev, "DAE")
    real = torch.from_numpy(np.load(a.real).astype(np.float32, copy=False)).to(dev)
    gen = torch.from_numpy(np.load(a.generated).astype(np.float32, copy=False)).to(dev)
    clips = {}
    if a.clip_chunks is not None:
        if a.real_clips or a.generated_clips or a.clip_chunks < 1:
            ap.error("--clip_chunks is a positive count and replaces --real_clips / --generated_clips")
        if real.shape[0] % a.clip_chunks or gen.shape[0] % a.clip_chunks:
            ap.error(f"--clip_chunks {a.clip_chunks} does not divide {real.shape[0]} real and {gen.shape[0]} generated chunks")
        clips = dict(real_clips=[a.clip_chunks] * (real.shape[0] // a.clip_chunks),
                     generated_clips=[a.clip_chunks] * (gen.shape[0] // a.clip_chunks))
    elif a.real_clips or a.generated_clips:
        if not (a.real_clips and a.generated_clips):
            ap.error("--real_clips and --generated_clips go together")
        clips = dict(real_clips=np.load(a.real_clips), generated_clips=np.load(a.generated_clips))
    m = gesture_metrics(net, real, gen, dae=dae, batch_rows=a.batch_rows, **clips)
    print(f"chunks: {m['n_real']} real, {m['n_generated']} generated")
    print(" Perplexity: " + repr(m["perplexity_generated"]))
    print("hell_dist --> " + repr(m["hellinger"]))
    print("Frechet Distance --> " + repr(m["frechet"]))
    print("wasserstein_distance -> " + repr(m["wasserstein"]))
    if clips:
        print(" BLEU: " + repr(m["bleu_sum"]) + " AVG_BLEU Score:" + repr(m["bleu"]) + " +-" + repr(m["bleu_var"]))
    if a.energy:
        m["energy"] = energy_distance(set_latents(net, real, dae, a.batch_rows), set_latents(net, gen, dae, a.batch_rows))
        print("Energy distance --> " + repr(m["energy"]))
    return m


if __name__ == "__main__":
    main()
