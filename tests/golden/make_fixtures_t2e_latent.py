#!/usr/bin/env python3
"""Golden vectors for Part d on continuous latents (text2_embedding_discrete: False) by IMPORTING the reference (build container
only), the way make_fixtures_text2embedding.py records the discrete mode.

Exercises model/text2embedding_model.py::text2embedding_model (:535-546, 630-746) with BahdanauAttnDecoderRNN(
discrete_representation=False) (:257-296, 338-395) and train_eval/train_seq2seq.py::train_iter_text2embedding (:499-510, 532-538):
two training iterations on one batch, then the eval-mode forward.  `use_TCN = False` on the module before construction, as in the
sibling.

Dropout: this mode never calls F.dropout (no embedding dropout), so MaskRecorder has nothing to record; every mask is ATen-internal
(nn.GRU's inter-layer dropout) and is recovered by replaying the global CPU RNG -- the packed encoder mask first, then one (1,B,H)
draw per decode step.  The alignment is PROVEN here: the float64 restatement (tests/_t2e_latent_ref.py) fed with the replayed masks
must reproduce the reference's recorded loss to 1e-6 relative, which misaligned masks cannot."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_fixtures as mf  # noqa: E402
import _t2e_latent_ref as R  # noqa: E402


def main():
    vq, dae, ts = mf._import_reference()
    import model.text2embedding_model as t2e
    t2e.use_TCN = False
    torch.set_num_threads(1)
    for name, att, p in (("t2e_latent_noatt", "False", 0.2), ("t2e_latent_att", "True", 0.2)):
        H, L, NW, EMB, S, Tw, B = 32, 2, 120, 300, 6, 12, 16
        E = L * H
        args = mf.make_args(hidden_size=H, n_layers=L, dropout_prob=p, autoencoder_vq_components=64, autoencoder_att=att,
                            n_pre_poses=1, n_poses=20, sentence_frame_length=120, text2_embedding_discrete="False")
        torch.manual_seed(3)
        emb = torch.randn(NW, EMB).numpy()
        net = t2e.text2embedding_model(args, 135, args.n_poses, NW, EMB, emb, None)
        assert net.pose_dim == E and not hasattr(net.decoder.decoder, "embedding")
        net.train(True)
        g = torch.Generator().manual_seed(77)
        lengths = torch.randint(4, Tw + 1, (B,), generator=g).sort(descending=True).values
        lengths[0] = Tw
        ids = torch.zeros(B, Tw, dtype=torch.int64)
        for b in range(B):
            ids[b, : lengths[b]] = torch.randint(4, NW, (int(lengths[b]),), generator=g)
        latents = torch.tanh(torch.randn(B, S, E, generator=g))
        fx = dict(mf.sd_np(net, "w0/"))
        fx.update(ids=ids.numpy(), lengths=lengths.numpy(), latents=latents.numpy(),
                  cfg=np.array([B, Tw, S, H, L, E, NW, EMB], dtype=np.int64), cfg_f=np.array([p, 5e-4]))
        optim = torch.optim.Adam(net.parameters(), lr=5e-4, betas=(0.5, 0.999))
        for step in (1, 2):
            seed = 5000 + step
            cap = {}
            orig_fwd, orig_enc = net.forward, net.encoder.forward

            def spy(*a, **k):
                out = orig_fwd(*a, **k)
                cap["outputs"] = out[0].detach().numpy().copy()
                return out

            def spy_enc(*a, **k):
                out = orig_enc(*a, **k)
                cap["enc_out"], cap["hidden0"] = out[0].detach().numpy().copy(), out[1][:L].detach().numpy().copy()
                return out

            net.forward, net.encoder.forward = spy, spy_enc
            before = {k: v.detach().clone() for k, v in net.state_dict().items()}
            torch.manual_seed(seed)
            with mf.MaskRecorder() as rec:
                loss = ts.train_iter_text2embedding(args, 1, ids, lengths, None, latents, None, None, net, optim)
            net.forward, net.encoder.forward = orig_fwd, orig_enc
            assert len(rec.masks) == 0, "this mode calls F.dropout nowhere"
            plan = [((int(lengths.sum()), 2 * H), p)] + [((1, B, H), p)] * (S - 1)
            rp = mf.replay_gru_masks(seed, plan)
            fx[f"s{step}/mask_dec_l0"] = np.stack([rp[1 + t].reshape(B, H) for t in range(S - 1)])
            # encoder inter-layer mask: packed rows are time-major over the still-valid batch rows -> padded layout, pads = keep
            enc = np.ones((Tw, B, 2 * H), dtype=bool)
            pk, off = rp[0].reshape(-1, 2 * H), 0
            for t in range(Tw):
                nb = int((lengths > t).sum())
                enc[t, :nb] = pk[off:off + nb]
                off += nb
            assert off == pk.shape[0]
            fx[f"s{step}/mask_enc_l0"] = enc
            fx[f"s{step}/loss"] = np.float64(loss["loss"])
            fx[f"s{step}/outputs"] = cap["outputs"]
            fx[f"s{step}/hidden0"] = cap["hidden0"]
            if att == "True":
                fx[f"s{step}/enc_out"] = cap["enc_out"]
            for k, v in before.items():                      # the decoder as this step saw it: what the restatement needs
                if k.startswith("decoder.decoder.") and step > 1:
                    fx[f"w{step - 1}/{k}"] = v.numpy().copy()
            # ---- the proof of the mask alignment (and of the restatement): its loss is the reference's
            P = R.decoder_params(before, requires_grad=False)
            tgt = latents.transpose(0, 1).double()
            outs, _ = R.rollout(P, torch.from_numpy(cap["hidden0"]).double(), tgt, args.n_pre_poses, p,
                                torch.from_numpy(fx[f"s{step}/mask_dec_l0"]),
                                torch.from_numpy(cap["enc_out"]).double() if att == "True" else None)
            got, ref = float(R.mse(outs, tgt)), float(loss["loss"])
            assert abs(got - ref) <= 1e-6 * abs(ref), ("RNG replay misaligned (or the restatement is wrong)", name, step, got, ref)
            assert np.array_equal(cap["outputs"][:, 0], latents.numpy()[:, 0])
            if step == 1:
                for n_, p_ in net.named_parameters():
                    if p_.grad is not None:
                        fx[f"s1/grad/{n_}"] = p_.grad.detach().numpy().copy()
                    else:
                        fx[f"s1/gradnone/{n_}"] = np.zeros(0, dtype=np.float32)
        fx.update(mf.sd_np(net, "wN/"))
        net.train(False)
        with torch.no_grad():
            out, _ = net(ids, lengths, None, latents, None, None)
        fx["eval/outputs"] = out.numpy().copy()
        # three files per case, each below the repository's 1 MiB limit for a committed file (random mantissas do not compress):
        # <name>.npz = inputs, initial state_dict, per-step records, eval outputs; <name>_grads.npz = the gradients of step 1;
        # <name>_final.npz = the final state_dict.  tests/_t2e_latent_ref.py::load_golden reads them back as one mapping.
        parts = {"_grads": {k: v for k, v in fx.items() if k.startswith(("s1/grad/", "s1/gradnone/"))},
                 "_final": {k: v for k, v in fx.items() if k.startswith("wN/")}}
        parts[""] = {k: v for k, v in fx.items() if k not in parts["_grads"] and k not in parts["_final"]}
        for suffix, part in parts.items():
            path = os.path.join(HERE, name + suffix + ".npz")
            np.savez_compressed(path, **part)
            assert os.path.getsize(path) < (1 << 20), (path, os.path.getsize(path))
        print(name, "losses", [float(fx[f"s{s}/loss"]) for s in (1, 2)],
              "grad keys", sum(k.startswith("s1/grad/") for k in fx), "none", [k for k in fx if k.startswith("s1/gradnone/")],
              "zero grads", [k for k in fx if k.startswith("s1/grad/") and np.abs(fx[k]).max() == 0])


if __name__ == "__main__":
    main()
