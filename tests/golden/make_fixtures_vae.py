#!/usr/bin/env python3
"""Golden vectors for the VARIATIONAL chunk autoencoder (autoencoder_vae == "True"), by IMPORTING the reference (build container
only), with make_fixtures.py's reference import, dropout-mask recording and make_args, and the noise of `reparameterize`
(model/Autoencoder_VQVAE_model.py:879-899) recorded by wrapping torch.randn_like.

Autoencoder_VQVAE (:776-789, 989-1010) then owns VAE_fc_mean / VAE_fc_std / VAE_fc_decoder (E -> E), runs them behind the
quantiser (if any) and returns (outputs, decoder_first_hidden, mean, logvar[, loss_vq, perplexity_vq]);
train_iter_Autoencoder_VQ_seq2seq (train_eval/train_seq2seq.py:692-758) adds KLD * 0.1 * epoch / args.epochs for epoch > 0.

vae.npz:
  a/  B = 8, T = 12, D = 40, H = 32, dropout 0.2, no quantiser: three iterations at epochs 0, 1, 2 -- inputs, every mask, eps,
      losses (total, custom_loss, KLD), the encoder state, mean, logvar, first hidden, outputs, the gradient arriving at
      VAE_fc_decoder's output, the six VAE tensors in front of step 2 (the first with the KL term), their gradients at every step
      (whole at step 2), every gradient of the epoch-1 step, the state after the last step -- and an eval-mode forward (the noise is drawn there too);
  b/  config/seq2seq.yml's dimensions (T = 20, D = 40, H = 200, dropout 0.0) at B = 8: one iteration at epoch 1;
  c/  shape a with autoencoder_vq "True", i.e. the soft quantiser the reference ships (:816-820), K = 48: two iterations at
      epochs 1, 2 -- where the reference's trainer starts (train_autoencoder_VQVAE.py:163) -- and an eval-mode forward.  (At epoch 0
      loss_vq is not in the loss, the quantiser's tensors have no gradient and torch.optim.Adam skips them, so their bias
      correction starts one step later than everything else's; the fused clip + Adam keeps ONE step count for the flat buffer
      and differs there by up to 0.115 lr on the first step that moves them -- an optimiser corner outside the trainer's epochs,
      written down in DESIGN.md 3.6c, not a property of the variational block);
  d/  the reference's state_dict keys and shapes at H = 200 for both autoencoder_vq settings.
  Gradients and final tensors above 1024 elements are stored as their float64 L2 norm + a strided sample (<name>_norm/,
  <name>_sample/); case a's VAE tensors in front of step 2 and their gradients there (4096 elements) stay whole for
  tests/test_vae_ref_host.py.  The inputs x are torch.randn(B, T, D, generator seeded 1234 + seed), stored as a sha256.
  Initial states: oracle/g2v_oracle.py's init_vqvae_state without vq_layer.*, tests/_vae_ref.py's vae_state for the block (both
  from seeds; a sha256 per tensor lets a test know it regenerated the same bits); case c's vq_layer.* tensors are stored whole.
vae_ckpt.bin: case a's model after its three iterations, written the way train_autoencoder_VQVAE.py:233-244 writes a checkpoint.

usage:  python tests/golden/make_fixtures_vae.py
"""
from __future__ import annotations

import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_fixtures as MF  # noqa: E402
from make_fixtures_plain_ae import plain_state, put  # noqa: E402
from _vae_ref import NAMES, vae_state  # noqa: E402

WHOLE_MAX = 4096         # what the block's float64 restatement is fed with (case a: the six VAE tensors, E = 64) stays whole
SAMPLE_ABOVE = 1024      # every other gradient / final tensor above this size: norm + strided sample


class NoiseRecorder:
    """Wraps torch.randn_like (reparameterize's only draw, :894); records the noise in call order."""

    def __init__(self):
        self.eps = []

    def __enter__(self):
        self._orig = torch.randn_like

        def randn_like(t, *a, **k):
            e = self._orig(t, *a, **k)
            self.eps.append(e.detach().numpy().copy())
            return e

        torch.randn_like = randn_like
        return self

    def __exit__(self, *a):
        torch.randn_like = self._orig


def replay(seed, plan):
    """make_fixtures.replay_gru_masks with normal draws in the plan: [("bern", shape, p) | ("randn", shape)] in draw order"""
    torch.manual_seed(seed)
    out = []
    for item in plan:
        if item[0] == "randn":
            out.append(torch.empty(item[1]).normal_().numpy().copy())
            continue
        _, shape, p = item
        if shape[0] == "T01":        # in_poses.transpose(0, 1) is a non-contiguous view and ATen draws into empty_like(view)
            _, (T, B, D) = shape
            e = torch.empty(B, T, D).transpose(0, 1)
        else:
            e = torch.empty(shape)
        out.append(e.bernoulli_(1 - p).to(torch.uint8).numpy().copy())
    return out


def record(vq, ts, fx, tag, *, B, T, D, H, p, epochs_run, seed, with_vq, K=48):
    L, E = 2, 2 * H
    args = MF.make_args(rep_learning_dim=D, hidden_size=H, n_layers=L, dropout_prob=p, n_poses=T, autoencoder_vae="True",
                        autoencoder_vq="True" if with_vq else "False", autoencoder_vq_components=K)
    torch.manual_seed(seed)
    net = vq.Autoencoder_VQVAE(args, D, T)
    assert net.VAE is True and net.vq is with_vq
    sd0 = dict(plain_state(D, H, seed))
    sd0.update(vae_state(E, seed))
    for k_, v_ in sd0.items():
        fx[f"{tag}/w0_sha256/{k_}"] = np.array(hashlib.sha256(v_.contiguous().numpy().tobytes()).hexdigest())
    if with_vq:
        assert type(net.vq_layer).__name__ == "VQ_Payam_GSSoft"
        for k_, v_ in net.vq_layer.state_dict().items():
            sd0["vq_layer." + k_] = v_.detach().clone()
            fx[f"{tag}/w0/vq_layer.{k_}"] = v_.detach().numpy().copy()
    net.load_state_dict(sd0, strict=True)
    net.train(True)
    x = torch.randn(B, T, D, generator=torch.Generator().manual_seed(1234 + seed))
    optim = torch.optim.Adam(net.parameters(), lr=args.learning_rate, betas=(0.5, 0.999))
    fx[f"{tag}/x_sha256"] = np.array(hashlib.sha256(x.numpy().tobytes()).hexdigest())      # (from the seed, like the weights)
    fx[f"{tag}/cfg"] = np.array([B, T, D, H, L, len(epochs_run), seed, K if with_vq else 0, args.epochs], dtype=np.int64)
    fx[f"{tag}/cfg_f"] = np.array([p, args.learning_rate, args.loss_l1_weight, args.loss_cont_weight, args.loss_var_weight,
                                   float(args.autoencoder_vq_commitment_cost)], dtype=np.float64)
    fx[f"{tag}/epochs_run"] = np.array(epochs_run, dtype=np.int64)
    for step, epoch in enumerate(epochs_run, 1):
        step_seed = 9300 + 17 * step + seed
        cap = {}
        key = f"{tag}/s{step}"
        if tag == "a" and step == 2:            # (step 1 starts from vae_state(E, seed); step 2 is the first with the KL term)
            for n_ in NAMES:
                fx[f"{key}/vae_w/{n_}"] = net.state_dict()[n_].numpy().copy()

        def enc_hook(mod, inp, out):
            cap["encoder_hidden"] = out[1].detach().numpy().copy()

        def dec_fc_hook(mod, inp, out):       # the gradient that reaches the block from the decoder, in (B,E) layout
            out.register_hook(lambda g: cap.__setitem__("g_fc_decoder", g.detach().numpy().copy()))

        def net_hook(mod, inp, out):
            cap["first_hidden"] = out[1].detach().numpy().copy()
            cap["mean"], cap["logvar"] = out[2].detach().numpy().copy(), out[3].detach().numpy().copy()
            if with_vq:
                cap["loss_vq"], cap["perplexity"] = float(out[4]), float(out[5])

        orig = ts.custom_loss

        def spy(output, target, a):
            cap["outputs"] = output.detach().numpy().copy()
            v = orig(output, target, a)
            cap["custom_loss"] = float(v)
            return v

        hooks = [net.encoder.register_forward_hook(enc_hook), net.VAE_fc_decoder.register_forward_hook(dec_fc_hook),
                 net.register_forward_hook(net_hook)]
        ts.custom_loss = spy
        torch.manual_seed(step_seed)
        with MF.MaskRecorder() as rec, NoiseRecorder() as noise:
            ret = ts.train_iter_Autoencoder_VQ_seq2seq(args, epoch, x, x, net, optim)
        ts.custom_loss = orig
        for h in hooks:
            h.remove()
        if with_vq:
            assert isinstance(ret, tuple) and len(ret) == 2 and set(ret[0]) == {"loss"}
            loss = ret[0]["loss"]
            assert float(ret[1]) == cap["perplexity"]
        else:
            assert isinstance(ret, dict) and set(ret) == {"loss"}
            loss = ret["loss"]
        assert len(noise.eps) == 1 and noise.eps[0].shape == (B, E)
        masks = rec.masks
        k = 1 if p > 0 else 0
        dec = np.stack([m.reshape(B, D) for m in masks[k:]])
        assert dec.shape[0] == T - 1
        fx[f"{key}/mask_dec"] = np.packbits(dec, axis=None)
        fx[f"{key}/eps"] = noise.eps[0]
        if p > 0:
            fx[f"{key}/mask_in"] = np.packbits(masks[0], axis=None)          # (T,B,D)
            plan = [("bern", ("T01", (T, B, D)), p), ("bern", (T, B, 2 * H), p), ("randn", (B, E))]
            for _ in range(T - 1):
                plan += [("bern", (1, B, D), 0.95), ("bern", (1, B, H), p)]
            rp = replay(step_seed, plan)
            assert np.array_equal(rp[0], masks[0]), "RNG replay misaligned (input dropout)"
            assert np.array_equal(rp[2], noise.eps[0]), "RNG replay misaligned (reparameterize's noise)"
            for t in range(T - 1):
                assert np.array_equal(rp[3 + 2 * t].reshape(B, D), dec[t]), "RNG replay misaligned (dec)"
            fx[f"{key}/mask_dec_l0"] = np.packbits(np.stack([rp[4 + 2 * t].reshape(B, H) for t in range(T - 1)]), axis=None)
        mean, logvar = cap["mean"].astype(np.float64), cap["logvar"].astype(np.float64)
        fx[f"{key}/epoch"] = np.int64(epoch)
        fx[f"{key}/loss"] = np.float64(loss)
        fx[f"{key}/custom_loss"] = np.float64(cap["custom_loss"])
        fx[f"{key}/kld"] = np.float64(0.5 * np.mean(np.exp(logvar) - logvar - 1 + mean ** 2))
        if with_vq:
            fx[f"{key}/loss_vq"], fx[f"{key}/perplexity"] = np.float64(cap["loss_vq"]), np.float64(cap["perplexity"])
        for n_ in ("encoder_hidden", "mean", "logvar", "first_hidden", "outputs", "g_fc_decoder"):
            fx[f"{key}/{n_}"] = cap[n_][:L].copy() if n_ == "encoder_hidden" else cap[n_]
        for n_, p_ in net.named_parameters():
            if n_ in NAMES:
                put(fx, f"{key}/vae_grad", n_, p_.grad, WHOLE_MAX if (tag == "a" and step == 2) else SAMPLE_ABOVE)
        if epoch == 1:
            for n_, p_ in net.named_parameters():
                if p_.grad is not None:
                    put(fx, f"{tag}/grad", n_, p_.grad, SAMPLE_ABOVE)
                else:
                    fx[f"{tag}/gradnone/{n_}"] = np.zeros(0, dtype=np.float32)
            fx[f"{tag}/grad_step"] = np.int64(step)
    for k_, v_ in net.state_dict().items():
        put(fx, f"{tag}/wN", k_, v_, SAMPLE_ABOVE)
    net.train(False)
    torch.manual_seed(4242 + seed)
    with torch.no_grad(), MF.MaskRecorder() as rec, NoiseRecorder() as noise:
        res = net(x, x)
    assert len(res) == (6 if with_vq else 4) and len(rec.masks) == T - 1 and len(noise.eps) == 1
    fx[f"{tag}/eval/mask_dec"] = np.packbits(np.stack([m.reshape(B, D) for m in rec.masks]), axis=None)
    fx[f"{tag}/eval/eps"] = noise.eps[0]
    for n_, v_ in zip(("outputs", "first_hidden", "mean", "logvar"), res):
        fx[f"{tag}/eval/{n_}"] = v_.numpy().copy()
    if with_vq:
        fx[f"{tag}/eval/loss_vq"], fx[f"{tag}/eval/perplexity"] = np.float64(float(res[4])), np.float64(float(res[5]))
    return net, args


def main():
    vq, _dae, ts = MF._import_reference()
    from model.vocab import Vocab
    torch.set_num_threads(1)  # deterministic summation order for the golden numbers
    fx = {}
    net_a, args_a = record(vq, ts, fx, "a", B=8, T=12, D=40, H=32, p=0.2, epochs_run=(0, 1, 2), seed=31, with_vq=False)
    record(vq, ts, fx, "b", B=8, T=20, D=40, H=200, p=0.0, epochs_run=(1,), seed=32, with_vq=False)
    record(vq, ts, fx, "c", B=8, T=12, D=40, H=32, p=0.2, epochs_run=(1, 2), seed=33, with_vq=True)
    for name, with_vq in (("plain", "False"), ("vq", "True")):
        ref = vq.Autoencoder_VQVAE(MF.make_args(rep_learning_dim=40, hidden_size=200, n_poses=20, autoencoder_vae="True",
                                                autoencoder_vq=with_vq, autoencoder_vq_components=512), 40, 20)
        sd = ref.state_dict()
        fx[f"d/{name}/keys"] = np.array(list(sd))
        fx[f"d/{name}/shapes"] = np.array(["x".join(str(s) for s in v.shape) for v in sd.values()])
    out = os.path.join(HERE, "vae.npz")
    np.savez_compressed(out, **fx)

    lang = Vocab("words")
    for w in "the quick brown fox jumps over the lazy dog the end".split():
        lang.index_word(w)
    lang.word_embedding_weights = np.random.RandomState(3).randn(lang.n_words, 300).astype(np.float32)
    ckpt = os.path.join(HERE, "vae_ckpt.bin")
    torch.save({"args": args_a, "epoch": 3, "lang_model": lang, "pose_dim": 40, "gen_dict": net_a.state_dict()}, ckpt)
    print("[vae] losses a", [float(fx[f"a/s{s}/loss"]) for s in (1, 2, 3)], "kld a", [float(fx[f"a/s{s}/kld"]) for s in (1, 2, 3)],
          "b", float(fx["b/s1/loss"]), "c", [float(fx[f"c/s{s}/loss"]) for s in (1, 2)],
          "gradnone", sorted({k.split("/", 2)[2] for k in fx if "/gradnone/" in k}), "bytes", os.path.getsize(out), os.path.getsize(ckpt))


if __name__ == "__main__":
    main()
