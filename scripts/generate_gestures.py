#!/usr/bin/env python3
"""Generates pose clips on the MI355X kernels (gesture2vec_amd/generate.py): the decode loops of the reference's
`inference_Autoencoder.py`, `Clustering.py::make_VQ_Centers` and `inference_text2embedding.py` as one command.

    python generate_gestures.py --autoencoder-checkpoint ae.bin [--dae-checkpoint dae.bin]
                                (--codes x.npy | --latents x.npy | --poses x.npy | --codebook) --out y.npy
                                [--smooth savgol] [--seed N] [--kmeans kmeans_model.pk]
                                [--angles-out a.npy] [--rotation-fit {markley,procrustes}] [--spline-smooth P|none]

Exactly one source:
  --codes    (B, C) integer codes: rows of the autoencoder's codebook, or of `--kmeans` for a quantiser-free autoencoder
             (default: <checkpoint dir>/clusters/kmeans_model.pk, where cluster_latents.py writes it)
  --latents  (B, C, L * H) latent rows, as gesture2vec_amd.pipeline.chunk_latents returns them
  --poses    (B, F, D_raw) raw poses to reconstruct (inference_Autoencoder.generate_gestures: the chunks start at
             range(0, F - n_poses, n_poses), which drops a trailing full chunk)
  --codebook one gesture per code (make_VQ_Centers) -> (K, n_poses, D_raw)
The frames go through the DAE's decoder (when a DAE checkpoint is given and it is no identity), are blended over 10 frames across
the chunk boundaries and un-normalised with the checkpoint's data_mean / data_std; `--smooth savgol` adds the Savitzky-Golay
filter (window 25, order 5) along time.  `--seed` seeds the masks of the decoder's inline Dropout(0.95).
`--angles-out` also writes the (B, frames, D_raw / 3) joint angles the reference's make_bvh hands to pymo: D_raw holds one row-major
3x3 matrix per joint; per frame they become intrinsic "ZXY" Euler angles in degrees (`--rotation-fit markley`: scipy 1.10.1's
from_matrix, the reference's pin; `procrustes`: scipy 1.15.3's, the nearest rotation first) and every channel is then smoothed
along time by a cubic smoothing spline (`--spline-smooth`, default 0.5, the reference's smooth_f; `none` writes the raw angles).
`--smooth savgol` still filters the matrices first, as in the reference.  BVH writing, audio and word timing are out of scope: the
outputs are .npy files."""
from __future__ import annotations

import argparse
import os
import pickle
import sys

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
for _p in (_HERE, _ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from utils.train_utils import load_checkpoint_and_model  # noqa: E402
from gesture2vec_amd import generate  # noqa: E402


def _smooth_arg(text):
    if text.lower() == "none":
        return None
    p = float(text)
    if not 0.0 <= p <= 1.0:
        raise argparse.ArgumentTypeError(f"--spline-smooth lies in [0, 1] or is 'none', got {text!r}")
    return p


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--autoencoder-checkpoint", dest="autoencoder_checkpoint", required=True)
    ap.add_argument("--dae-checkpoint", dest="dae_checkpoint", default=None)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--codes", default=None, help=".npy of (B, C) codes")
    src.add_argument("--latents", default=None, help=".npy of (B, C, L * H) latent rows")
    src.add_argument("--poses", default=None, help=".npy of (B, F, D_raw) raw poses")
    src.add_argument("--codebook", action="store_true", help="one gesture per code")
    ap.add_argument("--out", required=True, help=".npy to write")
    ap.add_argument("--smooth", choices=["savgol"], default=None)
    ap.add_argument("--angles-out", dest="angles_out", default=None, help=".npy of (B, frames, D_raw / 3) joint angles to write")
    ap.add_argument("--rotation-fit", dest="rotation_fit", choices=list(generate.NEAREST), default="markley")
    ap.add_argument("--spline-smooth", dest="spline_smooth", type=_smooth_arg, default=generate.SPLINE_SMOOTH,
                    help="smoothing parameter of the spline over the angles in [0, 1], or 'none'")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--kmeans", default=None, help="pickled KMeans model of a quantiser-free autoencoder")
    ap.add_argument("--route", choices=list(generate.ROUTES), default="auto")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    dev = torch.device(a.device)
    args, net, _, _, _ = load_checkpoint_and_model(a.autoencoder_checkpoint, dev, "autoencoder_vq")
    net.rng_seed = int(a.seed)
    dae = None
    if a.dae_checkpoint:
        _, dae, _, _, _ = load_checkpoint_and_model(a.dae_checkpoint, dev, "DAE")
    mean, std = getattr(args, "data_mean", None), getattr(args, "data_std", None)
    if mean is not None:
        mean, std = np.asarray(mean, dtype=np.float64).squeeze(), np.asarray(std, dtype=np.float64).squeeze()
    km = None
    if not getattr(net, "vq", True) and (a.codes or a.codebook):
        path = a.kmeans or os.path.join(os.path.dirname(os.path.abspath(a.autoencoder_checkpoint)), "clusters", "kmeans_model.pk")
        with open(path, "rb") as f:
            km = pickle.load(f)
    T = int(net.n_frames)
    load = lambda p, dt: torch.from_numpy(np.load(p).astype(dt, copy=False)).to(dev)
    if a.codebook:
        clips = generate.codebook_gestures(net, dae, mean, std, kmeans=km, route=a.route)
    elif a.poses:
        clips = generate.reconstruct_clips(dae, net, load(a.poses, np.float32), mean, std, smooth=a.smooth, route=a.route)
    else:
        if a.codes:
            frames = generate.decode_codes(net, load(a.codes, np.int64), kmeans=km, route=a.route)
        else:
            frames = generate.decode_latents(net, load(a.latents, np.float32), route=a.route)
        clips = generate.finish_clips(dae, frames, mean, std, n_poses=T, smooth=a.smooth)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.save(a.out, clips.cpu().numpy())
    print(f"wrote {a.out}: {tuple(clips.shape)}")
    if a.angles_out:
        angles = generate.clip_angles(clips, nearest=a.rotation_fit, spline=a.spline_smooth)
        os.makedirs(os.path.dirname(os.path.abspath(a.angles_out)), exist_ok=True)
        np.save(a.angles_out, angles.cpu().numpy())
        print(f"wrote {a.angles_out}: {tuple(angles.shape)}")
    return clips


if __name__ == "__main__":
    main()
