#!/usr/bin/env python3
"""Golden vectors for the frame-level quantised autoencoder of Part a (autoencoder_vq == "True"), by IMPORTING the reference on the
CPU (build container only): VQ_Frame (scripts/model/DAE_model.py:118-275) with its VQ_Payam_EMA (:351-482) under
train_iter_DAE (train_eval/train_seq2seq.py:161-241) and torch.optim.Adam(lr, betas=(0.5, 0.999)), with make_fixtures.py's reference
import and dropout-mask recording.

vqframe.npz (B, D, L, K):
  a/  warm quantiser, (128, 135, 40, 80): three iterations at lr 5e-4, then an eval-mode forward(x, Inference=True);
  b/  warm, (100, 135, 45, 100): two iterations (B, L and K off the tile sizes);
  c/  fresh initialisation, (37, 20, 8, 5): three iterations -- the blow-up of the second step;
  d/  fresh initialisation, (128, 135, 40, 80): one iteration;
  e/  the reference's state_dict keys and shapes.
  warm = codebook N(0, 1), _ema_cluster_size = B / K, _ema_w = codebook B / K (tests/_vqframe_ref.py: warm_quantiser).
  Per case: seed, shape, lr, w0/<key> (the initial state_dict, whole), x_sha256 (the batches come from the seed: batches()), and per
  step s<i>/: mask (np.packbits of the keep mask), loss (the reconstruction term), perplexity, ids (every row), latent, margin and
  bound (float64, per row); s1/grad/<key> (encoder.0.bias: no bar, see record()); wN/<key> the state after the last step; eval/ out, latent, ids, margin, bound (case a).
  Arrays above 1024 elements are stored as <name>_norm (float64 L2 norm) + <name>_sample (a strided sample).

The margin check.  Every recorded training step is restated in float64 (tests/_vqframe_ref.py) and each row's margin between its
nearest and its second-nearest code is ASSERTED to be at least 1e-5 (|z| + max(|e1|, |e2|))^2 -- about twice the worst-case fp32
rounding of |z|^2 + |e|^2 - 2 z.e at L <= 45, plus the rounding of z itself --, and the reference's ids are asserted equal to the
restatement's.  Seeds are searched from 0 until both hold; the margins are stored.  A test may then compare EVERY id.

The bars.  bar/<name> = max(4 x the distance of the reference's own fp32 value from the float64 restatement, 1e-6), distance = max
|a - b| / max |b| over the stored parts.  The reference's fp32 and the kernels' fp32 are two orderings of one expression; four times
one ordering's error covers the other.  The bars never see the code under test.

vqframe_ckpt.bin: case a's model after its iterations, written the way train_DAE.py:216-229 writes a checkpoint.

usage:  python tests/golden/make_fixtures_vqframe.py
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
import _vqframe_ref as R  # noqa: E402

CASES = {"a": dict(shape=(128, 135, 40, 80), warm=True, steps=3, infer=True),
         "b": dict(shape=(100, 135, 45, 100), warm=True, steps=2, infer=False),
         "c": dict(shape=(37, 20, 8, 5), warm=False, steps=3, infer=False),
         "d": dict(shape=(128, 135, 40, 80), warm=False, steps=1, infer=False)}
LR = 5e-4


def put(fx, bars, name, ref32, f64):
    packed = R.pack(ref32)
    for part, v in packed.items():
        fx[name + part] = v
    bars["bar/" + name] = np.float64(max(4.0 * R.distance(packed, R.pack(f64)), 1e-6))


def record(dae, ts, tag, seed, shape, warm, steps, infer):
    B, D, L, K = shape
    torch.manual_seed(seed)
    net = dae.VQ_Frame(D, L, False, K)
    sd0 = {k: v.detach().numpy().copy() for k, v in net.state_dict().items()}
    if warm:
        sd0 = R.warm_quantiser(sd0, B, seed)
        net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd0.items()}, strict=True)
    args = argparse.Namespace(autoencoder_vq="True", autoencoder_vae="False")
    optim = torch.optim.Adam(net.parameters(), lr=LR, betas=(0.5, 0.999))
    net.train(True)
    seen = {}
    hook = net.vq_layer.register_forward_hook(lambda m, i, o: seen.update(z=i[0].detach().numpy().copy(),
                                                                         ids=o[3].argmax(1).numpy().copy()))
    data = R.batches(seed, B, D, steps)
    fx = {f"{tag}/seed": np.int64(seed), f"{tag}/shape": np.array(shape, np.int64), f"{tag}/lr": np.float64(LR)}
    fx[f"{tag}/x_sha256"] = np.array(R.batches_sha256(data))
    for k, v in sd0.items():
        fx[f"{tag}/w0/{k}"] = np.asarray(v)
    ref, masks = [], []
    for i, (noisy, original) in enumerate(data, 1):
        torch.manual_seed(50 + i)
        with MF.MaskRecorder() as rec:
            loss, perplexity = ts.train_iter_DAE(args, 1, noisy, original, net, optim)
        assert len(rec.masks) == 1 and rec.ps == [0.5]
        masks.append(rec.masks[0])
        ref.append(dict(loss=loss["loss"], perplexity=float(perplexity), latent=seen["z"], ids=seen["ids"]))
        if i == 1:
            ref[0]["grads"] = {k: dict(net.named_parameters())[k].grad.numpy().copy() for k in R.TRAINABLE}
            others = [n for n, p in net.named_parameters() if n not in R.TRAINABLE and p.grad is not None]
            assert not others, others      # the quantiser's tensors never receive a gradient
    hook.remove()
    res64, state64 = R.iterate(sd0, [(n.squeeze(2).numpy(), o.squeeze(2).numpy(), m) for (n, o), m in zip(data, masks)], LR)
    for r32, r64 in zip(ref, res64):
        if not np.array_equal(r32["ids"], r64["ids"]) or not np.all(r64["margin"] >= r64["bound"]):
            return None
    bars = {}
    for i, (r32, r64, m) in enumerate(zip(ref, res64, masks), 1):
        s = f"{tag}/s{i}/"
        fx[s + "mask"] = np.packbits(m.reshape(-1))
        fx[s + "ids"] = r32["ids"].astype(np.int16)
        fx[s + "margin"], fx[s + "bound"] = r64["margin"], r64["bound"]
        put(fx, bars, s + "loss", np.float64(r32["loss"]), r64["rec"])
        put(fx, bars, s + "perplexity", np.float64(r32["perplexity"]), r64["perplexity"])
        put(fx, bars, s + "latent", r32["latent"], r64["latent"])
        if i == 1:
            for k in R.TRAINABLE:
                put(fx, bars, s + "grad/" + k, r32["grads"][k], r64["grads"][k])
            # d loss / d encoder.0.bias is exactly zero (BatchNorm removes a column's mean): what arrives is rounding alone and
            # has no relative bar; it is held against the restatement's bound for the fp32 sum instead (_vqframe_ref.step)
            del bars["bar/" + s + "grad/encoder.0.bias"]
            assert np.all(np.abs(r32["grads"]["encoder.0.bias"]) <= r64["dbe_bound"])
    sdN = {k: v.detach().numpy().copy() for k, v in net.state_dict().items()}
    assert int(sdN["bachnorm.num_batches_tracked"]) == steps == int(state64["bachnorm.num_batches_tracked"])
    for k, v in sdN.items():
        if k == "bachnorm.num_batches_tracked":
            fx[f"{tag}/wN/{k}"] = v
        else:
            put(fx, bars, f"{tag}/wN/{k}", v, state64[k])
    if infer:
        net.train(False)
        x = data[-1][0]
        with torch.no_grad():
            out, latent, enc = net(x, Inference=True)
        e64 = R.infer(state64, x.squeeze(2).numpy().astype(np.float64))
        ids = enc.argmax(1).numpy()
        if not np.array_equal(ids, e64["ids"]) or not np.all(e64["margin"] >= e64["bound"]):
            return None
        fx[f"{tag}/eval/ids"] = ids.astype(np.int16)
        fx[f"{tag}/eval/margin"], fx[f"{tag}/eval/bound"] = e64["margin"], e64["bound"]
        put(fx, bars, f"{tag}/eval/out", out.squeeze(2).numpy(), e64["out"])
        put(fx, bars, f"{tag}/eval/latent", latent.numpy(), e64["latent"])
        net.train(True)
    fx.update(bars)
    return fx, net


def main():
    _vq, dae, ts = MF._import_reference()
    torch.set_num_threads(1)
    fx = {}
    for tag, case in CASES.items():
        for seed in range(200):
            got = record(dae, ts, tag, seed, **case)
            if got is not None:
                break
        else:
            raise SystemExit(f"case {tag}: no seed below 200 leaves every row decided")
        fx.update(got[0])
        print(f"[vqframe] case {tag}: seed {seed}, losses", [float(got[0][f"{tag}/s{i}/loss"]) for i in range(1, case["steps"] + 1)],
              "perplexities", [float(got[0][f"{tag}/s{i}/perplexity"]) for i in range(1, case["steps"] + 1)])
        if tag == "a":
            args = argparse.Namespace(autoencoder_vq="True", autoencoder_vae="False", input_motion_dim=135, hidden_size=40,
                                      autoencoder_vq_components=80, name="Frame_Level")
            torch.save({"args": args, "epoch": 20, "lang_model": None, "pose_dim": 135, "gen_dict": got[1].state_dict()},
                       os.path.join(HERE, "vqframe_ckpt.bin"))
    net = dae.VQ_Frame(135, 40, False, 80)
    fx["e/state_dict"] = np.array(json.dumps({k: list(v.shape) for k, v in net.state_dict().items()}))
    bars = {k: float(v) for k, v in fx.items() if k.startswith("bar/")}
    print("[vqframe] largest bars:", sorted(bars.items(), key=lambda kv: -kv[1])[:8])
    np.savez_compressed(os.path.join(HERE, "vqframe.npz"), **fx)
    print("[vqframe] wrote", os.path.getsize(os.path.join(HERE, "vqframe.npz")), "bytes")


if __name__ == "__main__":
    main()
