#!/usr/bin/env python3
"""Golden vectors for the QUANTISER-FREE chunk autoencoder (autoencoder_vq == "False": the reference's config/seq2seq.yml, whose
checkpoint AI2_11_HQ is the "high-quality" autoencoder of its text-to-gesture inference), by IMPORTING the reference (build
container only), with make_fixtures.py's reference import, dropout-mask recording and make_args.

Autoencoder_VQVAE (model/Autoencoder_VQVAE_model.py:686) then has no vq_layer (:829-830), feeds encoder_hidden[:L] to the decoder
as it is (:971-973, 1018) and returns (outputs, decoder_first_hidden) (:1082-1085); train_iter_Autoencoder_VQ_seq2seq
(train_eval/train_seq2seq.py:702-703, 755-758) takes loss = custom_loss alone and returns {"loss": float}.

plain_ae.npz:
  a/  tiny shape with dropout_prob > 0 (B = 8, T = 12, D = 40, H = 32): two iterations -- inputs, every mask (F.dropout draws
      recorded, nn.GRU's inter-layer ones re-derived by RNG replay), losses, encoder states, outputs, step-1 gradients, every
      tensor of the state after step 2 (BatchNorm running statistics included) -- and an eval-mode forward with recorded masks;
  b/  config/seq2seq.yml's dimensions (T = 20, D = 40, H = 200, dropout 0.0) at B = 8: one iteration and an eval-mode forward;
      2.3 M parameters, so tensors above 4096 elements are stored as their float64 L2 norm + a strided sample (<name>_norm/,
      <name>_sample/, as make_fixtures_h200.py does);
  c/  the reference's state_dict key list and shapes at config/seq2seq.yml's dimensions.
  The initial states are oracle/g2v_oracle.py's init_vqvae_state(D, H, 2, K=1, seed) without the vq_layer.* tensors, loaded into
  the reference model with load_state_dict(strict=True); a sha256 per tensor lets a test know it regenerated the same bits.
plain_ae_ckpt.bin: shape a's model after its two iterations, written the way train_autoencoder_VQVAE.py:233-244 writes a
  checkpoint (torch.save of args Namespace, epoch, a model.vocab.Vocab, pose_dim, gen_dict).

usage:  python tests/golden/make_fixtures_plain_ae.py
"""
from __future__ import annotations

import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_fixtures as MF  # noqa: E402
from oracle import g2v_oracle as O  # noqa: E402


def sample_index(numel: int) -> np.ndarray:
    """the strided sample of a flattened tensor that fixture and tests agree on (tests/_h200.py)"""
    stride = max(1, numel // 512)
    return np.arange(0, numel, stride)[:512]


def plain_state(D: int, H: int, seed: int):
    return {k: v for k, v in O.init_vqvae_state(D, H, 2, 1, seed=seed).items() if not k.startswith("vq_layer.")}


def put(fx: dict, head: str, name: str, t: torch.Tensor, whole_max: int) -> None:
    """head/name -> the whole tensor, or head_norm/name + head_sample/name when it has more than whole_max elements"""
    t = t.detach()
    if t.numel() <= whole_max or not t.dtype.is_floating_point:
        fx[f"{head}/{name}"] = t.numpy().copy()
        return
    fx[f"{head}_norm/{name}"] = np.float64(t.double().norm())
    fx[f"{head}_sample/{name}"] = t.reshape(-1).numpy()[sample_index(t.numel())].copy()


def record(vq, ts, fx: dict, tag: str, B: int, T: int, D: int, H: int, p: float, n_steps: int, seed: int, whole_max: int):
    L = 2
    args = MF.make_args(rep_learning_dim=D, hidden_size=H, n_layers=L, dropout_prob=p, n_poses=T, autoencoder_vq="False")
    torch.manual_seed(seed)
    net = vq.Autoencoder_VQVAE(args, D, T)
    assert net.vq is False and not hasattr(net, "vq_layer")
    sd0 = plain_state(D, H, seed)
    net.load_state_dict(sd0, strict=True)
    net.train(True)
    x = torch.randn(B, T, D, generator=torch.Generator().manual_seed(1234 + seed))
    optim = torch.optim.Adam(net.parameters(), lr=args.learning_rate, betas=(0.5, 0.999))
    fx[f"{tag}/x"] = x.numpy().copy()
    fx[f"{tag}/cfg"] = np.array([B, T, D, H, L, n_steps, seed], dtype=np.int64)
    fx[f"{tag}/cfg_f"] = np.array([p, args.learning_rate, args.loss_l1_weight, args.loss_cont_weight, args.loss_var_weight],
                                  dtype=np.float64)
    for k_, v_ in sd0.items():
        fx[f"{tag}/w0_sha256/{k_}"] = np.array(hashlib.sha256(v_.contiguous().numpy().tobytes()).hexdigest())
    for step in range(1, n_steps + 1):
        step_seed = 9100 + 17 * step + seed
        cap = {}

        def enc_hook(mod, inp, out):
            cap["encoder_hidden"] = out[1].detach().numpy().copy()

        orig = ts.custom_loss

        def spy(output, target, a):
            cap["outputs"] = output.detach().numpy().copy()
            v = orig(output, target, a)
            cap["custom_loss"] = float(v)
            return v

        h = net.encoder.register_forward_hook(enc_hook)
        ts.custom_loss = spy
        torch.manual_seed(step_seed)
        with MF.MaskRecorder() as rec:
            ret = ts.train_iter_Autoencoder_VQ_seq2seq(args, step, x, x, net, optim)
        ts.custom_loss = orig
        h.remove()
        assert isinstance(ret, dict) and set(ret) == {"loss"} and ret["loss"] == cap["custom_loss"]
        # masks: make_fixtures.gen_vqvae_train's bookkeeping (a quantiser draws nothing, so the draw order is the same)
        masks = rec.masks
        k = 1 if p > 0 else 0
        dec = np.stack([m.reshape(B, D) for m in masks[k:]])
        assert dec.shape[0] == T - 1
        fx[f"{tag}/s{step}/mask_dec"] = np.packbits(dec, axis=None)
        if p > 0:
            fx[f"{tag}/s{step}/mask_in"] = np.packbits(masks[0], axis=None)          # (T,B,D)
            plan = [(("T01", (T, B, D)), p), ((T, B, 2 * H), p)]
            for _ in range(T - 1):
                plan += [((1, B, D), 0.95), ((1, B, H), p)]
            rp = MF.replay_gru_masks(step_seed, plan)
            assert np.array_equal(rp[0], masks[0]), "RNG replay misaligned (input dropout)"
            for t in range(T - 1):
                assert np.array_equal(rp[2 + 2 * t].reshape(B, D), dec[t]), "RNG replay misaligned (dec)"
            fx[f"{tag}/s{step}/mask_dec_l0"] = np.packbits(np.stack([rp[3 + 2 * t].reshape(B, H) for t in range(T - 1)]), axis=None)
        fx[f"{tag}/s{step}/loss"] = np.float64(ret["loss"])
        fx[f"{tag}/s{step}/encoder_hidden"] = cap["encoder_hidden"][:L].copy()
        fx[f"{tag}/s{step}/outputs"] = cap["outputs"]
        if step == 1:
            for n_, p_ in net.named_parameters():
                if p_.grad is not None:
                    put(fx, f"{tag}/s1/grad", n_, p_.grad, whole_max)
                else:
                    fx[f"{tag}/s1/gradnone/{n_}"] = np.zeros(0, dtype=np.float32)
    for k_, v_ in net.state_dict().items():
        put(fx, f"{tag}/wN", k_, v_, whole_max)
    net.train(False)
    torch.manual_seed(4242 + seed)
    with torch.no_grad(), MF.MaskRecorder() as rec:
        outs, first_hidden = net(x, x)
    assert len(rec.masks) == T - 1
    fx[f"{tag}/eval/mask_dec"] = np.packbits(np.stack([m.reshape(B, D) for m in rec.masks]), axis=None)
    fx[f"{tag}/eval/outputs"] = outs.numpy().copy()
    fx[f"{tag}/eval/first_hidden"] = first_hidden.numpy().copy()
    return net, args


def main():
    vq, _dae, ts = MF._import_reference()
    from model.vocab import Vocab
    torch.set_num_threads(1)  # deterministic summation order for the golden numbers
    fx = {}
    net_a, args_a = record(vq, ts, fx, "a", B=8, T=12, D=40, H=32, p=0.2, n_steps=2, seed=21, whole_max=1 << 30)
    record(vq, ts, fx, "b", B=8, T=20, D=40, H=200, p=0.0, n_steps=1, seed=22, whole_max=4096)
    ref = vq.Autoencoder_VQVAE(MF.make_args(rep_learning_dim=40, hidden_size=200, n_poses=20, autoencoder_vq="False"), 40, 20)
    sd = ref.state_dict()
    fx["c/keys"] = np.array(list(sd))
    fx["c/shapes"] = np.array(["x".join(str(s) for s in v.shape) for v in sd.values()])
    out = os.path.join(HERE, "plain_ae.npz")
    np.savez_compressed(out, **fx)

    lang = Vocab("words")
    for w in "the quick brown fox jumps over the lazy dog the end".split():
        lang.index_word(w)
    lang.word_embedding_weights = np.random.RandomState(3).randn(lang.n_words, 300).astype(np.float32)
    ckpt = os.path.join(HERE, "plain_ae_ckpt.bin")
    torch.save({"args": args_a, "epoch": 2, "lang_model": lang, "pose_dim": 40, "gen_dict": net_a.state_dict()}, ckpt)
    print("[plain_ae] losses a", [float(fx[f"a/s{s}/loss"]) for s in (1, 2)], "b", float(fx["b/s1/loss"]),
          "gradnone", [k for k in fx if "gradnone" in k], "bytes", os.path.getsize(out), os.path.getsize(ckpt))


if __name__ == "__main__":
    main()
