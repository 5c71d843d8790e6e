"""Autoencoder_VQVAE exactly as the reference ships it (VQ_Payam_GSSoft override left in place, reference
model/Autoencoder_VQVAE_model.py:816-820) on the MI355X kernels: train iterations, eval forward and checkpoint interop
against golden vectors captured from the reference import (tests/golden/make_fixtures_shipped.py)."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import g2v_oracle as O
from test_gpu_vqvae import fixture_args, relerr, state_from

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _shipped_args(fx):
    dims, args = fixture_args(fx)
    args.autoencoder_vq_quantizer = "gssoft"
    return dims, args


@pytest.mark.parametrize("fused", ["1", "0"])
def test_shipped_model_train_steps_match_reference_golden(golden_dir, monkeypatch, fused):
    """fused = 1: the iteration as ONE kernel sequence of the engine (VQVAEEngine._forward_gssoft / _backward_gssoft, what
    train_iter takes by default); 0: the module-level autograd path over the same kernels.  Both against the reference's numbers."""
    monkeypatch.setenv("G2V_GSSOFT_FUSED", fused)
    from gesture2vec_amd.model.Autoencoder_VQVAE_model import Autoencoder_VQVAE, VQ_Payam_GSSoft
    from gesture2vec_amd.train_eval.train_seq2seq import FusedClipAdam, train_iter_Autoencoder_VQ_seq2seq
    fx = np.load(os.path.join(golden_dir, "vqvae_shipped.npz"))
    (B, T, D, H, L, K, n_steps), args = _shipped_args(fx)
    net = Autoencoder_VQVAE(args, D, T)
    assert isinstance(net.vq_layer, VQ_Payam_GSSoft)
    net.load_state_dict(state_from(fx, "w0/"), strict=True)          # identical key set, incl. the unused pre_linear
    net = net.to(DEV)
    net.train(True)
    optim = FusedClipAdam(net, lr=args.learning_rate, betas=(0.5, 0.999))
    x = torch.from_numpy(fx["x"].copy()).to(DEV)
    for step in range(1, n_steps + 1):
        net.set_dropout_masks(O.unpack_mask(fx[f"s{step}/mask_dec"], (T - 1, B, D)).to(DEV))
        loss, perp = train_iter_Autoencoder_VQ_seq2seq(args, 1, x, x, net, optim)
        eng = net.engine()
        b = eng.buffers(B)
        assert ("gs_probs" in b) == (fused == "1")                    # the path under test is the one that ran
        ref_loss = float(fx[f"s{step}/loss"])
        assert abs(loss["loss"] - ref_loss) <= 2e-5 * abs(ref_loss), (loss["loss"], ref_loss)
        assert abs(float(perp) - float(fx[f"s{step}/perplexity"])) <= 1e-4 * float(fx[f"s{step}/perplexity"])
        assert relerr(b["quant"], fx[f"s{step}/quantized"]) < 1e-4
        assert relerr(b["y"].transpose(0, 1), fx[f"s{step}/outputs"]) < 1e-4, "reconstructed poses"
        if step == 1:
            for k in fx.files:
                if k.startswith("s1/grad/"):
                    n = k[len("s1/grad/"):]
                    assert n in eng.offsets, f"{n} has a gradient in the reference but is not trainable here"
                    g, ref = eng.view(n, True), fx[k]
                    if n == "decoder.decoder.pre_linear.0.bias":      # mathematically zero (feeds BatchNorm)
                        assert float(g.abs().max()) < 1e-6 and np.abs(ref).max() < 1e-6
                    elif np.abs(ref).max() == 0:
                        assert float(g.abs().max()) == 0, n           # encoder GRU layer 1: exactly zero on both sides
                    else:
                        assert relerr(g, ref) < 5e-4, (n, relerr(g, ref))
                elif k.startswith("s1/gradnone/"):
                    assert k[len("s1/gradnone/"):] not in eng.offsets
    for n, ref in state_from(fx, "wN/").items():
        got = net.state_dict()[n]
        if n in ("decoder.decoder.pre_linear.0.bias", "decoder.decoder.pre_linear.1.running_mean"):
            assert float((got.cpu() - ref).abs().max()) <= 1.01 * n_steps * args.learning_rate, n
        elif ref.dtype.is_floating_point:
            err = float((got.cpu().double() - ref.double()).abs().max())
            assert err <= 1e-4 * float(ref.abs().max()) + 0.02 * args.learning_rate, (n, err)
        else:
            assert torch.equal(got.cpu(), ref), n


def _eval_check(net, fx, B, T, D):
    x = torch.from_numpy(fx["x"].copy()).to(DEV)
    net.train(False)
    net.set_dropout_masks(O.unpack_mask(fx["eval/mask_dec"], (T - 1, B, D)).to(DEV))
    with torch.no_grad():
        outs, first_hidden, loss_vq, perp = net(x, x)
    assert relerr(outs, fx["eval/outputs"]) < 1e-4
    assert relerr(first_hidden, fx["eval/first_hidden"]) < 1e-4
    assert abs(float(loss_vq) - float(fx["eval/loss_vq"])) <= 1e-4 * abs(float(fx["eval/loss_vq"]))
    assert abs(float(perp) - float(fx["eval/perplexity"])) <= 1e-4 * float(fx["eval/perplexity"])


def test_shipped_model_eval_forward_matches_reference_golden(golden_dir):
    from gesture2vec_amd.model.Autoencoder_VQVAE_model import Autoencoder_VQVAE
    fx = np.load(os.path.join(golden_dir, "vqvae_shipped.npz"))
    (B, T, D, H, L, K, _), args = _shipped_args(fx)
    net = Autoencoder_VQVAE(args, D, T)
    net.load_state_dict(state_from(fx, "wN/"), strict=True)
    _eval_check(net.to(DEV), fx, B, T, D)


def test_reference_checkpoint_file_loads_and_reproduces_eval(golden_dir):
    """A checkpoint written by the reference's own save path (pickled args Namespace + model.vocab.Vocab + gen_dict of the
    as-shipped GSSoft model) goes through load_checkpoint_and_model unchanged and reproduces the reference's eval forward."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from utils.train_utils import load_checkpoint_and_model
    fx = np.load(os.path.join(golden_dir, "vqvae_shipped.npz"))
    B, T, D = [int(v) for v in fx["cfg"][:3]]
    args, net, loss_fn, lang_model, pose_dim = load_checkpoint_and_model(os.path.join(golden_dir, "vqvae_shipped_ckpt.bin"),
                                                                        DEV, "autoencoder_vq")
    assert args.autoencoder_vq_quantizer == "gssoft" and pose_dim == D and not net.training
    assert lang_model.n_words == 13 and lang_model.get_word_index("fox") == lang_model.word2index["fox"]
    _eval_check(net, fx, B, T, D)


@pytest.mark.parametrize("B,p,mode,hidden", [
    pytest.param(64, 0.0, "eager", None, id="64-0.0-eager"), pytest.param(48, 0.2, "eager", None, id="48-0.2-eager"),
    pytest.param(1024, 0.0, "graph", None, id="1024-0.0-graph"), pytest.param(96, 0.0, "eager", 200, id="96-0.0-eager-h200")])
def test_fused_soft_quantiser_step_equals_the_autograd_path(B, p, mode, hidden, monkeypatch):
    """Three iterations of train_iter with the soft quantiser: the engine's kernel sequence (eager, and replayed from the hipGraph
    train_iter captures at large batch) against the module-level autograd path over the same kernels.  Same products, same
    element-wise kernels; the codebook gradient's two addends meet in the other order, so weights agree to fp32 rounding.
    hidden = 200: the shipped width E = 400, which csrc/vq_soft.hip does not serve -- the engine's non-fused forward and
    _backward_gssoft_chain."""
    from gesture2vec_amd import _lib
    from gesture2vec_amd.model.Autoencoder_VQVAE_model import Autoencoder_VQVAE
    from gesture2vec_amd.train_eval.train_seq2seq import FusedClipAdam, train_iter_Autoencoder_VQ_seq2seq
    import bench
    args = bench.model_args()
    args.autoencoder_vq_quantizer = "gssoft"
    if hidden is not None:
        args.hidden_size = hidden
        E = hidden * args.n_layers
        assert E == 400 and _lib.load().g2v_vq_soft_fused_ok((2 * B * hidden) // E, E, args.autoencoder_vq_components) == 0
    else:
        E = args.hidden_size * args.n_layers
        assert _lib.load().g2v_vq_soft_fused_ok((2 * B * args.hidden_size) // E, E, args.autoencoder_vq_components) == 1
    args.dropout_prob = p
    args.loss_l1_weight, args.loss_cont_weight, args.loss_var_weight, args.learning_rate = 5.0, 0.1, 0.5, 5e-4
    T, D = 34, 135
    xs = [torch.randn(B, T, D, generator=torch.Generator().manual_seed(400 + s)).to(DEV) for s in range(4)]
    out = {}
    for fused in ("0", "1"):
        monkeypatch.setenv("G2V_GSSOFT_FUSED", fused)
        torch.manual_seed(7)
        net = Autoencoder_VQVAE(args, D, T).to(DEV)
        net.train(True)
        net.rng_seed = 11
        if mode == "graph":
            net.engine().overlap_min_rows = 0
        optim = FusedClipAdam(net, lr=5e-4, betas=(0.5, 0.999))
        losses = []
        for s, x in enumerate(xs):
            loss, perp = train_iter_Autoencoder_VQ_seq2seq(args, 1, x, x, net, optim)
            losses.append((loss["loss"], float(perp)))
        eng = net.engine()
        assert ("gs_probs" in eng.buffers(B)) == (fused == "1")
        if fused == "1" and mode == "graph":
            assert getattr(eng, "_iter_graph", None) and eng._iter_graph["graph"], "the large-batch iteration was to be replayed"
        out[fused] = (losses, eng.flat.clone(), int(net.decoder.decoder.pre_linear[1].num_batches_tracked))
    for (l0, p0), (l1, p1) in zip(out["0"][0], out["1"][0]):
        assert abs(l0 - l1) <= 2e-5 * abs(l0) and abs(p0 - p1) <= 1e-4 * abs(p0), (l0, l1, p0, p1)
    assert out["0"][2] == out["1"][2] == len(xs) * (T - 1)      # BatchNorm's call counter: bumped by the fused step itself (side branch)
    err = float((out["0"][1] - out["1"][1]).abs().max())
    # a few per cent of the 4 Adam steps' lr: Adam turns the RELATIVE rounding difference of a small gradient element into a
    # difference of that fraction of lr (the engine's quantiser is one fused kernel each way since round 4, csrc/vq_soft.hip,
    # whose K- and E-long sums meet in another order than the separate launches'; element-wise parity of the two at 3e-4:
    # tests/test_gpu_thin_models.py::test_fused_soft_quantiser_kernels_equal_the_separate_kernels)
    assert err <= 4 * 5e-4 * 0.05 + 1e-6, err


def test_soft_quantiser_data_parallel_halves_on_one_gpu():
    """Two engine replicas play rank 0 / 1 (as tests/test_gpu_dp_engine.py does for the EMA model): train_step_local on each
    shard, the comm buffers summed by hand (= the RCCL SUM all-reduce), train_step_apply(world=2) on both.  The replicas must end
    bitwise identical, and equal to a third engine that is handed the MEAN of the two local gradients."""
    from gesture2vec_amd.engine import VQVAEEngine
    B, T, D, H, K = 64, 34, 135, 64, 512
    kw = dict(w_l1=5.0, w_cont=0.1, w_var=0.5)
    g = torch.Generator().manual_seed(9)
    init = None
    engs = []
    for r in range(3):
        eng = VQVAEEngine(D, H, 2, K, T, beta=0.25, dropout_prob=0.0, device=DEV, quantizer="gssoft")
        if init is None:
            init = (torch.randn(eng.n_flat, generator=g) * 0.08).to(DEV)
        eng.flat.copy_(init)
        eng.bn_rv.fill_(1.0)
        eng.seed = 100 + r
        engs.append(eng)
    xs = [torch.randn(B, T, D, generator=torch.Generator().manual_seed(50 + r)).to(DEV) for r in range(2)]
    for step in range(2):
        for r in range(2):
            engs[r].train_step_local(xs[r], xs[r], dp=True, epoch=1, **kw)
        torch.cuda.synchronize()
        local = [engs[r].comm.clone() for r in range(2)]
        total = local[0] + local[1]
        for r in range(2):
            engs[r].comm.copy_(total)
            engs[r].train_step_apply(B, lr=5e-4, world=2, dp=True)
        # the reference of the apply half: mean gradient -> clip 5 -> Adam, on the third engine
        engs[2].gflat.copy_(total[:engs[2].n_flat] / 2)
        engs[2].optimizer_step(5e-4)
        torch.cuda.synchronize()
        assert torch.equal(engs[0].flat, engs[1].flat), step
        err = float((engs[0].flat - engs[2].flat).abs().max())
        assert err <= 1e-6, (step, err)
        xs = [x + 0.01 for x in xs]
