#!/usr/bin/env python3
"""Golden vectors for the frame-level variational autoencoder of Part a (autoencoder_vq == "False", autoencoder_vae == "True"), by
IMPORTING the reference on the CPU (build container only): VAE_Network (scripts/model/DAE_model.py:600-725) under train_iter_DAE
(train_eval/train_seq2seq.py:161-241) and torch.optim.Adam(lr, betas=(0.5, 0.999)), with make_fixtures.py's reference import and
dropout-mask recording and make_fixtures_vae.py's noise recording.

vaeframe.npz (B, D, L):
  a/  (128, 135, 40): three iterations at lr 5e-4, then an eval-mode forward(x) and a forward(x, get_latent=True), noise recorded;
  b/  (100, 135, 45): two iterations (B and L off the tile sizes);
  c/  (37, 20, 8): three iterations;
  e/  the reference's state_dict keys and shapes.
  Per case: seed, shape, lr, w0/<key> (the initial state_dict, whole), x_sha256 (the batches come from the seed:
  _vqframe_ref.batches()), and per step s<i>/: mask (np.packbits of the keep mask), eps (the noise, whole), loss (the total, mse +
  12.5 kl), out, mean, logvar, latent (a forward hook); s1/grad/<key> for the ten tensors; wN/<key> the state after the last step;
  eval/ eps, out, mean, logvar and latent/ eps, out, latent (case a).
  Arrays above 1024 elements are stored as <name>_norm (float64 L2 norm) + <name>_sample (a strided sample); eps is stored whole.

The bars.  bar/<name> = max(4 x the distance of the reference's own fp32 value from the float64 restatement
(tests/_vaeframe_ref.py), 1e-6), distance = max |a - b| / max |b| over the stored parts.  The reference's fp32 and the kernels' fp32
are two orderings of one expression; four times one ordering's error covers the other.  The bars never see the code under test.

vaeframe_ckpt.bin: case a's model after its iterations, written the way train_DAE.py:216-229 writes a checkpoint.

usage:  python tests/golden/make_fixtures_vaeframe.py
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_fixtures as MF  # noqa: E402
from make_fixtures_vae import NoiseRecorder  # noqa: E402
import _vaeframe_ref as R  # noqa: E402

CASES = {"a": dict(shape=(128, 135, 40), steps=3, infer=True),
         "b": dict(shape=(100, 135, 45), steps=2, infer=False),
         "c": dict(shape=(37, 20, 8), steps=3, infer=False)}
LR = 5e-4


def put(fx, bars, name, ref32, f64):
    packed = R.pack(ref32)
    for part, v in packed.items():
        fx[name + part] = v
    bars["bar/" + name] = np.float64(max(4.0 * R.distance(packed, R.pack(f64)), 1e-6))


def record(dae, ts, tag, seed, shape, steps, infer):
    B, D, L = shape
    torch.manual_seed(seed)
    net = dae.VAE_Network(D, L)
    sd0 = {k: v.detach().numpy().copy() for k, v in net.state_dict().items()}
    assert tuple(sd0) == R.STATE_KEYS
    args = argparse.Namespace(autoencoder_vq="False", autoencoder_vae="True")
    optim = torch.optim.Adam(net.parameters(), lr=LR, betas=(0.5, 0.999))
    net.train(True)
    seen = {}
    hooks = [net.register_forward_hook(lambda m, i, o: seen.update(out=o[0].detach().squeeze(2).numpy().copy(),
                                                                   logvar=o[1].detach().numpy().copy(), mean=o[2].detach().numpy().copy())),
             net.encoder.register_forward_hook(lambda m, i, o: seen.update(latent=o.detach().numpy().copy()))]
    data = R.batches(seed, B, D, steps)
    fx = {f"{tag}/seed": np.int64(seed), f"{tag}/shape": np.array(shape, np.int64), f"{tag}/lr": np.float64(LR)}
    fx[f"{tag}/x_sha256"] = np.array(R.batches_sha256(data))
    for k, v in sd0.items():
        fx[f"{tag}/w0/{k}"] = np.asarray(v)
    ref, masks, noise = [], [], []
    for i, (noisy, original) in enumerate(data, 1):
        torch.manual_seed(50 + i)
        with MF.MaskRecorder() as rec, NoiseRecorder() as nz:
            loss = ts.train_iter_DAE(args, 1, noisy, original, net, optim)
        assert len(rec.masks) == 1 and rec.ps == [0.5] and len(nz.eps) == 1
        masks.append(rec.masks[0])
        noise.append(nz.eps[0])
        ref.append(dict(loss=loss["loss"], **{k: seen[k] for k in R.FORWARD}))
        if i == 1:
            ref[0]["grads"] = {k: dict(net.named_parameters())[k].grad.numpy().copy() for k in R.TRAINABLE}
    for h in hooks:
        h.remove()
    res64, state64 = R.iterate(sd0, [(n.squeeze(2).numpy(), o.squeeze(2).numpy(), m, e)
                                     for (n, o), m, e in zip(data, masks, noise)], LR)
    bars = {}
    for i, (r32, r64, m, e) in enumerate(zip(ref, res64, masks, noise), 1):
        s = f"{tag}/s{i}/"
        fx[s + "mask"] = np.packbits(m.reshape(-1))
        fx[s + "eps"] = e
        put(fx, bars, s + "loss", np.float64(r32["loss"]), r64["loss"])
        for k in R.FORWARD:
            put(fx, bars, s + k, r32[k], r64[k])
        if i == 1:
            for k in R.TRAINABLE:
                put(fx, bars, s + "grad/" + k, r32["grads"][k], r64["grads"][k])
    for k, v in net.state_dict().items():
        put(fx, bars, f"{tag}/wN/{k}", v.detach().numpy().copy(), state64[k])
    if infer:
        net.train(False)
        x = data[-1][0]
        x64 = x.squeeze(2).numpy().astype(np.float64)
        with torch.no_grad():
            torch.manual_seed(77)
            with NoiseRecorder() as nz:
                out, logvar, mean = net(x)
            e64 = R.infer(state64, x64, nz.eps[0].astype(np.float64))
            fx[f"{tag}/eval/eps"] = nz.eps[0]
            put(fx, bars, f"{tag}/eval/out", out.squeeze(2).numpy(), e64["out"])
            put(fx, bars, f"{tag}/eval/mean", mean.numpy(), e64["mean"])
            put(fx, bars, f"{tag}/eval/logvar", logvar.numpy(), e64["logvar"])
            with NoiseRecorder() as nz:
                out, latent = net(x, get_latent=True)
            e64 = R.infer(state64, x64, nz.eps[0].astype(np.float64))
            fx[f"{tag}/latent/eps"] = nz.eps[0]
            put(fx, bars, f"{tag}/latent/out", out.squeeze(2).numpy(), e64["out"])
            put(fx, bars, f"{tag}/latent/latent", latent.numpy(), e64["latent"])
        net.train(True)
    fx.update(bars)
    return fx, net


def main():
    _vq, dae, ts = MF._import_reference()
    torch.set_num_threads(1)
    fx = {}
    for seed, (tag, case) in enumerate(CASES.items()):
        got = record(dae, ts, tag, seed, **case)
        fx.update(got[0])
        print(f"[vaeframe] case {tag}: losses", [float(got[0][f"{tag}/s{i}/loss"]) for i in range(1, case["steps"] + 1)])
        if tag == "a":
            args = argparse.Namespace(autoencoder_vq="False", autoencoder_vae="True", input_motion_dim=135, hidden_size=40,
                                      name="Frame_Level")
            torch.save({"args": args, "epoch": 20, "lang_model": None, "pose_dim": 135, "gen_dict": got[1].state_dict()},
                       os.path.join(HERE, "vaeframe_ckpt.bin"))
    net = dae.VAE_Network(135, 40)
    fx["e/state_dict"] = np.array(json.dumps({k: list(v.shape) for k, v in net.state_dict().items()}))
    bars = {k: float(v) for k, v in fx.items() if k.startswith("bar/")}
    print("[vaeframe] largest bars:", sorted(bars.items(), key=lambda kv: -kv[1])[:8])
    np.savez_compressed(os.path.join(HERE, "vaeframe.npz"), **fx)
    print("[vaeframe] wrote", os.path.getsize(os.path.join(HERE, "vaeframe.npz")), "bytes")


if __name__ == "__main__":
    main()
