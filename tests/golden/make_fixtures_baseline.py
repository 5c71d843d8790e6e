#!/usr/bin/env python3
"""Golden vectors for the text -> pose baseline by IMPORTING the reference (build container only), the way
make_fixtures_t2e_latent.py records Part d: model/seq2seq_net.py::Seq2SeqNet and train_eval/train_seq2seq.py::custom_loss /
train_iter_seq2seq (:91-133), two training iterations on one batch, then the eval-mode forward; plus one reference-written
checkpoint (`baseline_ckpt.bin`, the five keys of scripts/train.py) for the strict state_dict load.

Shape: B = 8, Tw = 7, n_frames = 6, n_pre = 2, D = 135, H = 16, p = 0.2.

Dropout: the model never calls F.dropout; every mask is ATen-internal (nn.GRU's inter-layer dropout) and is recovered by replaying
the global CPU RNG -- the packed encoder mask first, then one (1,B,H) draw per decode step.  The alignment is PROVEN here: the
float64 restatement (tests/_pose_attn_ref.py) fed with the replayed masks must reproduce the reference's recorded loss to 1e-6.

The bars of tests/test_gpu_baseline_seq2seq.py::test_baseline_matches_reference_golden (loss 1e-5 relative, gradients 5e-4, eval
outputs 1e-4) are checked here against the reference's own precision: its float32 run must stay inside a quarter of each against its
float64 twin (the same module in double, fed the recorded masks through the replayed RNG) for the recorded inputs; seeds whose
inputs do not are passed over (MARGIN below), the bars stay."""
import argparse
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_fixtures as mf  # noqa: E402
import _pose_attn_ref as R  # noqa: E402

NAME = "baseline_seq2seq"


def relerr(got, ref):
    got, ref = torch.as_tensor(got).double().reshape(-1), torch.as_tensor(ref).double().reshape(-1)
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


# Two float32 implementations may each sit as far from the exact result as the reference's own float32 run does, on opposite sides:
# the recorded inputs must leave the reference at most a quarter of each bar, or the bar would measure the inputs' conditioning
# rather than the port.  Inputs (seeds) that do not are passed over; the bars stay.
MARGIN = 0.25


class IllConditioned(Exception):
    pass


def main():
    _vq, _dae, ts = mf._import_reference()
    import model.seq2seq_net as s2s
    torch.set_num_threads(1)
    for seed in range(11, 40):
        try:
            return record(ts, s2s, seed)
        except IllConditioned as e:
            print("seed", seed, "passed over:", e)
    raise SystemExit("no seed leaves the reference's float32 run inside a quarter of the bars")


def record(ts, s2s, seed0):
    B, Tw, S, NPRE, D, H, L, NW, EMB, p, lr = 8, 7, 6, 2, 135, 16, 2, 40, 24, 0.2, 5e-4
    args = mf.make_args(hidden_size=H, n_layers=L, dropout_prob=p, n_pre_poses=NPRE, n_poses=S, wordembed_dim=EMB)
    torch.manual_seed(seed0)
    emb = torch.randn(NW, EMB).numpy()
    net = s2s.Seq2SeqNet(args, D, S, NW, EMB, emb, None)
    net.train(True)
    g = torch.Generator().manual_seed(67 + seed0)
    lengths = torch.randint(3, Tw + 1, (B,), generator=g).sort(descending=True).values
    lengths[0] = Tw
    ids = torch.zeros(B, Tw, dtype=torch.int64)
    for b in range(B):
        ids[b, : lengths[b]] = torch.randint(4, NW, (int(lengths[b]),), generator=g)
    poses = torch.tanh(torch.randn(B, 1, D, generator=g) + (0.2 * torch.randn(B, S, D, generator=g)).cumsum(1))
    fx = dict(mf.sd_np(net, "w0/"))
    fx.update(ids=ids.numpy(), lengths=lengths.numpy(), poses=poses.numpy(),
              cfg=np.array([B, Tw, S, NPRE, D, H, L, NW, EMB], dtype=np.int64),
              cfg_f=np.array([p, lr, args.loss_l1_weight, args.loss_cont_weight, args.loss_var_weight]))
    # ---- the checkpoint, as the reference's trainer writes it (initial weights) ----
    lang = argparse.Namespace(n_words=NW, word_embedding_weights=emb)
    torch.save({"args": args, "epoch": 20, "lang_model": lang, "pose_dim": D, "gen_dict": net.state_dict()},
               os.path.join(HERE, "baseline_ckpt.bin"))
    twin = copy.deepcopy(net).double()                       # the float64 twin: same weights, same masks (same seeds below)
    optim = torch.optim.Adam(net.parameters(), lr=lr, betas=(0.5, 0.999))
    optim64 = torch.optim.Adam(twin.parameters(), lr=lr, betas=(0.5, 0.999))
    worst = {"loss": 0.0, "grad": 0.0}
    for step in (1, 2):
        seed = 6000 + step
        cap = {}
        orig_enc = net.encoder.forward

        def spy_enc(*a, **k):
            out = orig_enc(*a, **k)
            cap["enc_out"], cap["hidden0"] = out[0].detach().numpy().copy(), out[1][:L].detach().numpy().copy()
            return out

        net.encoder.forward = spy_enc
        before = {k: v.detach().clone() for k, v in net.state_dict().items()}
        torch.manual_seed(seed)
        with mf.MaskRecorder() as rec:
            loss = ts.train_iter_seq2seq(args, 1, ids, lengths, poses, net, optim)
        net.encoder.forward = orig_enc
        assert len(rec.masks) == 0, "the baseline calls F.dropout nowhere"
        plan = [((int(lengths.sum()), 2 * H), p)] + [((1, B, H), p)] * (S - 1)
        rp = mf.replay_gru_masks(seed, plan)
        fx[f"s{step}/mask_dec_l0"] = np.stack([rp[1 + t].reshape(B, H) for t in range(S - 1)])
        enc = np.ones((Tw, B, 2 * H), dtype=bool)
        pk, off = rp[0].reshape(-1, 2 * H), 0
        for t in range(Tw):
            nb = int((lengths > t).sum())
            enc[t, :nb] = pk[off:off + nb]
            off += nb
        assert off == pk.shape[0]
        fx[f"s{step}/mask_enc_l0"] = enc
        fx[f"s{step}/loss"] = np.float64(loss["loss"])
        # ---- the proof of the mask alignment (and of the restatement): its loss is the reference's ----
        P = R.decoder_params(before, requires_grad=False)
        r = R.rollout(P, torch.from_numpy(cap["hidden0"]).double(), poses.transpose(0, 1).double(),
                      torch.from_numpy(cap["enc_out"]).double(), NPRE, p, torch.from_numpy(fx[f"s{step}/mask_dec_l0"]))
        outs = torch.cat([poses.transpose(0, 1)[:1].double(), r["y"]]).transpose(0, 1)
        got = float(R.custom_loss(outs, poses.double(), args.loss_l1_weight, args.loss_cont_weight, args.loss_var_weight))
        ref = float(loss["loss"])
        assert abs(got - ref) <= 1e-6 * abs(ref), ("RNG replay misaligned (or the restatement is wrong)", step, got, ref)
        # ---- the float64 twin: the reference's own precision against the test's bars ----
        torch.manual_seed(seed)
        loss64 = ts.train_iter_seq2seq(args, 1, ids, lengths, poses.double(), twin, optim64)
        e = abs(loss["loss"] - loss64["loss"]) / abs(loss64["loss"])
        worst["loss"] = max(worst["loss"], e)
        if e > MARGIN * 1e-5:
            raise IllConditioned(f"step {step}: float32 loss {e:.2e} from the float64 twin")
        if step == 1:
            g64 = dict(twin.named_parameters())
            for n_, p_ in net.named_parameters():
                assert p_.grad is not None, n_
                fx[f"s1/grad/{n_}"] = p_.grad.detach().numpy().copy()
                if n_ == "decoder.decoder.pre_linear.0.bias":
                    continue
                e = relerr(p_.grad, g64[n_].grad)
                worst["grad"] = max(worst["grad"], e)
                if e > MARGIN * 5e-4:
                    raise IllConditioned(f"gradient {n_}: float32 {e:.2e} from the float64 twin")
    fx.update(mf.sd_np(net, "wN/"))
    net.train(False)
    twin.train(False)
    with torch.no_grad():
        out = net(ids, lengths, poses, None)
        out64 = twin(ids, lengths, poses.double(), None)
    e_eval = relerr(out, out64)
    if e_eval > MARGIN * 1e-4:
        raise IllConditioned(f"eval outputs: float32 {e_eval:.2e} from the float64 twin")
    fx["eval/outputs"] = out.numpy().copy()
    assert np.array_equal(fx["eval/outputs"][:, 0], poses.numpy()[:, 0])
    path = os.path.join(HERE, NAME + ".npz")
    np.savez_compressed(path, **fx)
    for f in (path, os.path.join(HERE, "baseline_ckpt.bin")):
        assert os.path.getsize(f) < 397396, (f, os.path.getsize(f))      # no larger than the smallest t2e_latent_* fixture
    print(NAME, "losses", [float(fx[f"s{s}/loss"]) for s in (1, 2)], "float32 vs float64 twin: loss %.2e grad %.2e eval %.2e"
          % (worst["loss"], worst["grad"], e_eval), "sizes", [os.path.getsize(f) for f in (path, os.path.join(HERE, "baseline_ckpt.bin"))])


if __name__ == "__main__":
    main()
