"""GPU parity of Part d on continuous latents (text2_embedding_discrete: False): the reference's golden vectors, the fused step
kernels (csrc/t2e_latent.hip) against the per-operator path and the float64 restatement (tests/_t2e_latent_ref.py), the feedback
gradient, eval mode, the deferred BatchNorm commit, the trainer script, the data path and the graphed step's refusal."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _t2e_latent_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def relerr(got, ref):
    got = got.detach().cpu().double().reshape(-1)
    ref = torch.as_tensor(ref).detach().cpu().double().reshape(-1)
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-12)


def _args(H, att, p, n_pre, S):
    return argparse.Namespace(hidden_size=H, n_layers=2, dropout_prob=p, autoencoder_vq_components=64, autoencoder_att=att,
                              n_pre_poses=n_pre, n_poses=20, sentence_frame_length=20 * S, text2_embedding_discrete="False",
                              autoencoder_conditioned="True", autoencoder_fixed_weight="False")


def _route(monkeypatch, kernels):
    from gesture2vec_amd import rollout_t2e
    monkeypatch.setattr(rollout_t2e, "LATENT_FUSED_MIN_ROWS", 1 if kernels == "fused_step" else 1 << 30)


# ---- 1. the reference's own numbers ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernels", ["per_operator", "fused_step"])
@pytest.mark.parametrize("name,att", [("t2e_latent_noatt", "False"), ("t2e_latent_att", "True")])
def test_latent_text2embedding_matches_reference_golden(golden_dir, name, att, kernels, monkeypatch):
    """Two training iterations and the eval forward against the reference's recorded run (tests/golden/make_fixtures_t2e_latent.py),
    at the bars of test_text2embedding_matches_reference_golden.  kernels = "fused_step": g2v_latent_rollout_fwd / _bwd, selected
    from LATENT_FUSED_MIN_ROWS rows in production and forced here; they do not serve attention."""
    if kernels == "fused_step" and att == "True":
        pytest.skip("the fused latent step kernels serve the attention-free decoder")
    from gesture2vec_amd import rollout_t2e
    from gesture2vec_amd.flat import FlatClipAdam
    from gesture2vec_amd.model.text2embedding_model import text2embedding_model
    from gesture2vec_amd.train_eval.train_seq2seq import train_iter_text2embedding
    _route(monkeypatch, kernels)
    calls0 = rollout_t2e.LATENT_FUSED_CALLS
    fx = R.load_golden(golden_dir, name)
    B, Tw, S, H, L, E, NW, EMB = [int(v) for v in fx["cfg"]]
    p, lr = [float(v) for v in fx["cfg_f"]]
    args = _args(H, att, p, 1, S)
    net = text2embedding_model(args, 135, 20, NW, EMB, np.zeros((NW, EMB), dtype=np.float32), None)
    net.load_state_dict({k[3:]: torch.from_numpy(fx[k].copy()) for k in fx if k.startswith("w0/")}, strict=True)
    net = net.to(DEV)
    net.train(True)
    optim = FlatClipAdam(net.parameters(), lr=lr, betas=(0.5, 0.999))
    ids = torch.from_numpy(fx["ids"].copy()).to(DEV)
    lengths = torch.from_numpy(fx["lengths"].copy())
    lat = torch.from_numpy(fx["latents"].copy()).to(DEV)
    for step in (1, 2):
        net.set_dropout_masks(None, torch.from_numpy(fx[f"s{step}/mask_dec_l0"].copy()).to(DEV),
                              torch.from_numpy(fx[f"s{step}/mask_enc_l0"].copy()).to(DEV).to(torch.uint8))
        loss = train_iter_text2embedding(args, 1, ids, lengths, None, lat, None, None, net, optim)
        ref = float(fx[f"s{step}/loss"])
        print(f"{name} {kernels} step {step}: loss {loss['loss']:.8f} ref {ref:.8f}")
        assert abs(loss["loss"] - ref) <= 1e-5 * ref, (loss, ref)
        if step == 1:
            for n, prm in net.named_parameters():
                gref = fx["s1/grad/" + n]
                if n == "decoder.decoder.pre_linear.0.bias":
                    continue                       # feeds BatchNorm: mathematically zero
                if np.abs(gref).max() == 0:
                    assert prm.grad is None or float(prm.grad.abs().max()) == 0.0, n     # encoder layer 1 without attention: dead compute
                else:
                    err = relerr(prm.grad, gref) if prm.grad is not None else float("inf")
                    print(f"  grad {n}: {err:.2e}")
                    assert err < 5e-4, (n, err)
    assert rollout_t2e.LATENT_FUSED_CALLS - calls0 == (2 if kernels == "fused_step" else 0)
    for k in fx:
        if k.startswith("wN/"):
            n = k[3:]
            ref, got = torch.from_numpy(fx[k].copy()), net.state_dict()[n].cpu()
            if n in ("decoder.decoder.pre_linear.0.bias", "decoder.decoder.pre_linear.1.running_mean"):
                assert float((got - ref).abs().max()) <= 1.01 * 2 * lr, n
            elif ref.dtype.is_floating_point:
                err = float((got.double() - ref.double()).abs().max())
                assert err <= 1e-4 * float(ref.abs().max()) + 0.02 * 2 * lr, (n, err)
            else:
                assert torch.equal(got, ref), n
    net.train(False)
    with torch.no_grad():
        out, attn_list = net(ids, lengths, None, lat, None, None)
    assert out.shape == (B, S, E)
    assert (len(attn_list) == S - 1 and attn_list[0].shape == (B, 1, Tw)) if att == "True" else attn_list == []
    assert relerr(out, fx["eval/outputs"]) < 1e-4
    assert torch.equal(out[:, 0], lat[:, 0])                   # outputs[:, 0] is the target's slot 0, bit for bit
    for train in (True, False):                                # the reference's inference branch makes no sense on latents: refused
        net.train(train)
        with pytest.raises(ValueError, match="vid_indices"):
            net(ids, lengths, None, lat, None, torch.zeros(B, dtype=torch.int64, device=DEV))


# ---- 2. fused kernels / per-operator path / restatement ------------------------------------------------------------------------
def _case(H, B, S, n_pre, p, att="False", seed=5):
    from gesture2vec_amd.model.text2embedding_model import text2embedding_model
    NW, EMB, Tw = 50, 30, 9
    args = _args(H, att, p, n_pre, S)
    g = torch.Generator().manual_seed(6)
    torch.manual_seed(seed)
    net = text2embedding_model(args, 135, 20, NW, EMB, np.random.RandomState(0).randn(NW, EMB).astype(np.float32), None).to(DEV)
    net.train(True)
    ids = torch.randint(1, NW, (B, Tw), generator=g).to(DEV)
    lengths = torch.sort(torch.randint(3, Tw + 1, (B,), generator=g), descending=True).values
    lengths[0] = Tw
    lat = torch.tanh(torch.randn(B, S, 2 * H, generator=g)).to(DEV)
    masks = (None, (torch.rand(S - 1, B, H, generator=g) < 1 - p).to(torch.uint8).to(DEV) if p > 0 else None,
             (torch.rand(Tw, B, 2 * H, generator=g) < 1 - p).to(torch.uint8).to(DEV) if p > 0 else None)
    return args, net, ids, lengths, lat, masks


def _forward_backward(net, ids, lengths, lat, masks, monkeypatch, kernels, train_mode=True):
    """one forward + the trainer's loss backward on the chosen route -> outputs (S,B,E), loss, the decoder's initial state and its
    gradient, every parameter gradient"""
    from gesture2vec_amd.train_eval import train_seq2seq as TS
    _route(monkeypatch, kernels)
    cap = {}
    orig = net.encoder.forward

    def enc(*a, **k):
        out, hid = orig(*a, **k)
        cap["hidden0"], cap["enc_out"] = hid.detach()[:2].clone(), None if out is None else out.detach().clone()
        if hid.requires_grad:
            hid.register_hook(lambda gr: cap.__setitem__("d_hidden0", gr.detach()[:2].clone()))
        return out, hid

    net.encoder.forward = enc
    try:
        net.zero_grad()
        net.set_dropout_masks(*masks)
        if not train_mode:
            with torch.no_grad():
                outputs, _ = net(ids, lengths, None, lat, None, None)
            return dict(outputs=outputs.transpose(0, 1).contiguous(), **cap)
        outputs, _ = net(ids, lengths, None, lat, None, None)
        loss = TS._latent_loss_backward(outputs, lat)
    finally:
        net.encoder.forward = orig
    return dict(outputs=outputs.detach().transpose(0, 1).contiguous(), loss=float(loss), grads={n: q.grad.detach().clone() for n, q in net.named_parameters() if q.grad is not None}, **cap)


def _restate(net, r, lat, n_pre, p, mask_l0, detach_feedback=False, training=True):
    P = R.decoder_params({k: v.detach().cpu() for k, v in net.state_dict().items()})
    h0 = r["hidden0"].cpu().double().requires_grad_(True)
    tgt = lat.detach().cpu().transpose(0, 1).double()
    enc = r["enc_out"].cpu().double() if "attn.v" in P else None
    outs, stats = R.rollout(P, h0, tgt, n_pre, p, mask_l0.cpu() if mask_l0 is not None else None, enc, training=training,
                            detach_feedback=detach_feedback)
    loss = R.mse(outs, tgt)
    if training:
        loss.backward()
    return dict(outputs=outs.detach(), loss=float(loss), d_hidden0=h0.grad, stats=stats,
                grads={"decoder.decoder." + k: v.grad for k, v in P.items() if v.grad is not None})


def _compare(got, ref, bar_loss, bar_out, bar_grad, tag):
    """outputs, loss, d hidden0 and EVERY decoder gradient; nothing skipped.  pre_linear.0.bias feeds BatchNorm, its gradient is
    the column sum of du, which BatchNorm's backward makes zero -- rounding noise on every side, so a ratio to its own largest entry
    says nothing; it is held to bar_grad times the largest entry of pre_linear.0.weight's gradient instead (the same du summed over
    the same rows, weighted by inputs of magnitude <= 1)."""
    figures = [("outputs", relerr(got["outputs"], ref["outputs"]), bar_out),
               ("loss", abs(got["loss"] - ref["loss"]) / abs(ref["loss"]), bar_loss),
               ("d_hidden0", relerr(got["d_hidden0"], ref["d_hidden0"]), bar_grad)]
    names = [n for n in ref["grads"] if n.startswith("decoder.decoder.")]
    assert len(names) == 14 and all(n in got["grads"] for n in names), (tag, sorted(got["grads"]))
    wmax = float(ref["grads"]["decoder.decoder.pre_linear.0.weight"].abs().max())
    for n in names:
        if n == "decoder.decoder.pre_linear.0.bias":
            err = float((got["grads"][n].cpu().double() - ref["grads"][n].cpu().double()).abs().max()) / wmax
        else:
            err = relerr(got["grads"][n], ref["grads"][n])
        figures.append((n, err, bar_grad))
    print(tag, " ".join(f"{n.replace('decoder.decoder.', '')}={e:.1e}" for n, e, _ in figures))
    for n, e, bar in figures:
        assert e < bar, (tag, n, e, bar)


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("n_pre", [1, 2])
@pytest.mark.parametrize("S1", [1, 5])
@pytest.mark.parametrize("H", [32, 200])
@pytest.mark.parametrize("B", [16, 20, 33])
def test_fused_latent_kernels_match_per_operator_path_and_restatement(B, H, S1, n_pre, p, monkeypatch):
    """g2v_latent_rollout_fwd / _bwd against the chain of per-operator autograd nodes (2e-4, the bar of
    test_fused_step_kernels_match_per_operator_path when the discrete decisions agree -- here there are none) and both against the
    float64 restatement at the golden bars (loss 1e-5, outputs 1e-4, gradients 5e-4 of the tensor's largest entry): one full row
    tile, a ragged second, a ragged third; H = 200 pads to 208 and E = 400 gives 25 output tiles; one step has no feedback term;
    n_pre moves the first fed-back step; with and without inter-layer dropout."""
    from gesture2vec_amd import rollout_t2e
    args, net, ids, lengths, lat, masks = _case(H, B, S1 + 1, n_pre, p)
    calls0 = rollout_t2e.LATENT_FUSED_CALLS
    fused = _forward_backward(net, ids, lengths, lat, masks, monkeypatch, "fused_step")
    assert rollout_t2e.LATENT_FUSED_CALLS - calls0 == 1, "the fused step kernels did not serve this shape (g2v_latent_rollout_ok)"
    perop = _forward_backward(net, ids, lengths, lat, masks, monkeypatch, "per_operator")
    assert rollout_t2e.LATENT_FUSED_CALLS - calls0 == 1
    assert torch.equal(fused["hidden0"], perop["hidden0"])
    ref = _restate(net, perop, lat, n_pre, p, masks[1])
    tag = f"B{B} H{H} S1={S1} n_pre{n_pre} p{p}"
    _compare(fused, perop, 2e-4, 2e-4, 2e-4, tag + " fused/per-op")
    _compare(fused, ref, 1e-5, 1e-4, 5e-4, tag + " fused/f64")
    _compare(perop, ref, 1e-5, 1e-4, 5e-4, tag + " per-op/f64")
    enc_names = [n for n in perop["grads"] if n.startswith("encoder.")]       # the encoder's share: it all went through d hidden0
    assert len(enc_names) >= 9 and all(n in fused["grads"] for n in enc_names)
    for n in enc_names:
        assert relerr(fused["grads"][n], perop["grads"][n]) < 2e-4, (tag, n, relerr(fused["grads"][n], perop["grads"][n]))


@pytest.mark.parametrize("att", ["False", "True"])
def test_per_operator_path_with_attention_matches_restatement(att, monkeypatch):
    """the only route with attention, at a ragged batch: against the float64 restatement at the golden bars"""
    args, net, ids, lengths, lat, masks = _case(48, 20, 6, 1, 0.2, att=att)
    perop = _forward_backward(net, ids, lengths, lat, masks, monkeypatch, "per_operator")
    ref = _restate(net, perop, lat, 1, 0.2, masks[1])
    if att == "True":          # d hidden0 of the restatement is the decoder's share only; with attention the encoder's final states
        ref["d_hidden0"] = perop["d_hidden0"]      # also receive gradient through the outputs: not comparable, the 17 parameters are
        assert len([n for n in ref["grads"]]) == 17
        for n in ("decoder.decoder.attn.attn.weight", "decoder.decoder.attn.attn.bias", "decoder.decoder.attn.v"):
            assert relerr(perop["grads"][n], ref["grads"].pop(n)) < 5e-4, n
    _compare(perop, ref, 1e-5, 1e-4, 5e-4, f"att={att} per-op/f64")


# ---- 3. the feedback gradient -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,B", [(32, 20), (200, 33)])
def test_feedback_gradient_is_attached(H, B, monkeypatch):
    """decoder_input = decoder_output, NOT detached (reference :741): for S-1 = 5, n_pre = 1 the gradient of the loss w.r.t.
    pre_linear.0.weight differs from the run with detached fed-back inputs by more than 100x the comparison bar (5e-4 of the
    largest entry), and both GPU routes match the attached form -- a port of the discrete backward would match the detached one."""
    args, net, ids, lengths, lat, masks = _case(H, B, 6, 1, 0.0)
    fused = _forward_backward(net, ids, lengths, lat, masks, monkeypatch, "fused_step")
    perop = _forward_backward(net, ids, lengths, lat, masks, monkeypatch, "per_operator")
    n = "decoder.decoder.pre_linear.0.weight"
    attached = _restate(net, perop, lat, 1, 0.0, None)["grads"][n]
    detached = _restate(net, perop, lat, 1, 0.0, None, detach_feedback=True)["grads"][n]
    gap = relerr(detached, attached)
    print(f"H{H} B{B}: detached vs attached {gap:.3e}; fused {relerr(fused['grads'][n], attached):.2e} per-op {relerr(perop['grads'][n], attached):.2e}")
    assert gap > 100 * 5e-4, gap
    for r in (fused, perop):
        assert relerr(r["grads"][n], attached) < 5e-4
        assert relerr(r["grads"][n], detached) > 50 * 5e-4


# ---- 4. eval mode ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("att", ["False", "True"])
def test_eval_forward_runs_on_the_running_statistics(att, monkeypatch):
    args, net, ids, lengths, lat, masks = _case(48, 20, 6, 1, 0.2, att=att)
    bn = net.decoder.decoder.pre_linear[1]
    g = torch.Generator().manual_seed(1)
    bn.running_mean.copy_(torch.randn(48, generator=g) * 0.3)
    bn.running_var.copy_(torch.rand(48, generator=g) + 0.5)
    net.train(False)
    before = (bn.running_mean.clone(), bn.running_var.clone(), int(bn.num_batches_tracked))
    r = _forward_backward(net, ids, lengths, lat, masks, monkeypatch, "fused_step", train_mode=False)
    ref = _restate(net, r, lat, 1, 0.2, masks[1], training=False)
    assert relerr(r["outputs"], ref["outputs"]) < 1e-4
    assert torch.equal(r["outputs"][0], lat[:, 0])
    assert torch.equal(bn.running_mean, before[0]) and torch.equal(bn.running_var, before[1]) and int(bn.num_batches_tracked) == before[2]
    net.train(True)
    with pytest.raises(ValueError, match="vid_indices"):
        net(ids, lengths, None, lat, None, torch.zeros(20, dtype=torch.int64, device=DEV))


# ---- 5. deferred BatchNorm commit -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernels,att", [("fused_step", "False"), ("per_operator", "False"), ("per_operator", "True")])
def test_deferred_batchnorm_commit(kernels, att, monkeypatch):
    """After one trainer iteration the running statistics equal nn.BatchNorm1d's step-by-step updates on the restatement's batch
    statistics (2e-6, the project's bar for g2v_bn_running_update_invstd); a forward whose commit is held back leaves them alone."""
    from gesture2vec_amd.flat import FlatClipAdam
    from gesture2vec_amd.train_eval.train_seq2seq import train_iter_text2embedding
    B, H, S = 20, 48, 6
    args, net, ids, lengths, lat, masks = _case(H, B, S, 1, 0.2, att=att)
    bn = net.decoder.decoder.pre_linear[1]
    # held back: nothing moves
    _route(monkeypatch, kernels)
    net.set_dropout_masks(*masks)
    net.deferred_bn = []
    net(ids, lengths, None, lat, None, None)
    assert float(bn.running_mean.abs().max()) == 0.0 and float((bn.running_var - 1).abs().max()) == 0.0
    assert len(net.deferred_bn) == (1 if kernels == "fused_step" else S - 1)
    net.deferred_bn = None
    bn.num_batches_tracked.zero_()
    # what the iteration should commit: from the weights as they stand before it
    probe = _forward_backward(net, ids, lengths, lat, masks, monkeypatch, "per_operator")
    stats = _restate(net, probe, lat, 1, 0.2, masks[1])["stats"]
    rm, rv = R.running_stats(stats, B)
    bn.running_mean.zero_(); bn.running_var.fill_(1.0); bn.num_batches_tracked.zero_()
    _route(monkeypatch, kernels)
    optim = FlatClipAdam(net.parameters(), lr=1e-3, betas=(0.5, 0.999))
    net.set_dropout_masks(*masks)
    loss = train_iter_text2embedding(args, 1, ids, lengths, None, lat, None, None, net, optim)
    assert np.isfinite(loss["loss"]) and net.deferred_bn is None
    assert int(bn.num_batches_tracked) == S - 1
    print(kernels, att, relerr(bn.running_mean, rm), relerr(bn.running_var, rv))
    assert relerr(bn.running_mean, rm) < 2e-6 and relerr(bn.running_var, rv) < 2e-6


# ---- 6. trainer script, data path, graphed step ---------------------------------------------------------------------------------
def test_trainer_script_trains_on_synthetic_latents(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import train_text2embedding as T
    import utils.train_utils as tu
    from config.parse_args import parse_args
    out = str(tmp_path / "run")
    os.makedirs(out)
    a = parse_args(["--config", os.path.join(ROOT, "config", "seq2seq_latent_synthetic.yml"), "--synthetic", "--synthetic_batches", "4",
                    "--batch_size", "16", "--hidden_size", "32", "--epochs", "2", "--model_save_path", out, "--name", "t"])
    net, val, losses = T.main({"args": a})
    assert len(losses) == 2 and all(np.isfinite(v) for v in losses) and losses[1] < losses[0], losses
    assert all(np.isfinite(v[0]) and v[1] == 0 for v in val), val          # MSE over all slots; the perplexity meter stays empty
    keys = set(net.state_dict())
    assert "decoder.decoder.embedding.weight" not in keys and net.state_dict()["decoder.decoder.out.weight"].shape == (64, 32)
    import types
    lang = types.SimpleNamespace(n_words=3863, word_embedding_weights=np.zeros((3863, a.wordembed_dim), dtype=np.float32))
    path = os.path.join(out, "t_checkpoint_002.bin")
    tu.save_checkpoint({"args": a, "epoch": 2, "lang_model": lang, "pose_dim": 512, "gen_dict": net.state_dict()}, path)
    args2, net2, _loss_fn, _lang, _dim = tu.load_checkpoint_and_model(path, DEV, "text2embedding")
    assert args2.text2_embedding_discrete == "False" and not net2.training and set(net2.state_dict()) == keys
    for k, v in net.state_dict().items():
        assert torch.equal(v.cpu(), net2.state_dict()[k].cpu()), k


def test_sentence_loader_yields_latents_without_a_quantiser(tmp_path):
    """neither a vq_layer nor a k-means model: the latents with cluster_ids = None (it used to die on self.vq_net.vq_layer)"""
    from gesture2vec_amd.data import serialize, write_lmdb
    from gesture2vec_amd.data.dataset import TrinityDataset_sentencelevel, sample_key
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from model.vocab import Vocab
    E, S, D, n = 64, 6, 135, 8
    rng = np.random.default_rng(11)
    vocab = Vocab("t")
    for w in ("so", "we", "went", "there", "and", "then", "home"):
        vocab.index_word(w)
    vocab.word_embedding_weights = rng.standard_normal((vocab.n_words, 300)).astype(np.float32)
    words_all = list(vocab.word2index)
    msp = str(tmp_path) + "/"
    os.makedirs(msp + "lmdb")
    items, lats = {}, []
    for i in range(n):
        nw = int(rng.integers(2, 7))
        words = [[words_all[int(rng.integers(0, len(words_all)))], 0.2 * j, 0.2 * j + 0.1] for j in range(nw)]
        lats.append(np.tanh(rng.standard_normal((S, E))).astype(np.float32))
        items[sample_key(i)] = serialize([words, rng.standard_normal((120, D)).astype(np.float16), [0], [[0.0]],
                                          {"vid": "v", "start_time": 0.0, "end_time": 9.0}, lats[-1], np.zeros(2, dtype=np.float32)])
    write_lmdb(msp + "lmdb/trn_sentence_level_cache", items)
    ds = TrinityDataset_sentencelevel(argparse.Namespace(model_save_path=msp, sentence_level="True"), str(tmp_path / "data" / "trn"),
                                      20, 10, 20, np.zeros(D), np.ones(D), lang_model=vocab, vq_net=argparse.Namespace(), kmeans=None)
    (words, lengths, poses, audio, aux, lat, codes, gpt3), = list(ds.batches(n, DEV, shuffle=False))
    assert codes is None and lat.shape == (n, S, E) and lat.is_cuda and lat.dtype == torch.float32
    assert lengths.tolist() == sorted(lengths.tolist(), reverse=True)
    got = sorted(float(x) for x in lat.sum((1, 2)).cpu())
    assert np.allclose(got, sorted(float(l.sum()) for l in lats), rtol=1e-5, atol=1e-4)


def test_graphed_step_refuses_continuous_latents():
    from gesture2vec_amd.flat import FlatClipAdam
    from gesture2vec_amd.train_eval.train_seq2seq import GraphedText2EmbeddingStep
    args, net, ids, lengths, lat, masks = _case(32, 16, 6, 1, 0.2)
    optim = FlatClipAdam(net.parameters(), lr=1e-3, betas=(0.5, 0.999))
    with pytest.raises(ValueError, match="not graphed"):
        GraphedText2EmbeddingStep(args, net, optim, ids, lengths, lat, warmup=1)
    assert not torch.cuda.is_current_stream_capturing()
