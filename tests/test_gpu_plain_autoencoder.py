"""GPU: the quantiser-free chunk autoencoder (autoencoder_vq == "False": the reference's config/seq2seq.yml, whose checkpoint
AI2_11_HQ is the "high-quality" autoencoder of its text-to-gesture inference) through every layer -- module surface,
train_iter_Autoencoder_VQ_seq2seq, the engine's quantizer="none" step, the trainer and the checkpoint loader -- against the
reference's own numbers (tests/golden/make_fixtures_plain_ae.py), a float64 oracle at B = 4096, the eager iterations, one
full-batch step, and a checkpoint the reference wrote."""
import argparse
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import g2v_oracle as O
from _f64 import as64, default64
from _h200 import sample_index

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BN = "decoder.decoder.pre_linear.1."
PRE_B = "decoder.decoder.pre_linear.0.bias"      # feeds BatchNorm in training: its gradient is rounding noise on both sides


def make_args(**kw):
    d = dict(rep_learning_dim=40, hidden_size=200, n_layers=2, dropout_prob=0.0, autoencoder_vae="False", autoencoder_vq="False",
             autoencoder_vq_components=512, autoencoder_vq_commitment_cost=0.25, n_pre_poses=1, autoencoder_conditioned="True",
             autoencoder_att="False", autoencoder_fixed_weight="False", n_poses=20, loss_l1_weight=5.0, loss_cont_weight=0.1,
             loss_var_weight=0.5, learning_rate=5e-4, epochs=10)
    d.update(kw)
    return argparse.Namespace(**d)


def plain_state(D, H, seed):
    """make_fixtures_plain_ae.py's initial states: init_vqvae_state without the quantiser's tensors"""
    return {k: v for k, v in O.init_vqvae_state(D, H, 2, 1, seed=seed).items() if not k.startswith("vq_layer.")}


def relerr(got, ref):
    got = got.detach().cpu().double().reshape(-1)
    ref = torch.as_tensor(ref).detach().cpu().double().reshape(-1)
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-12)


def relerr_l2(got, ref):
    got = got.detach().cpu().double().reshape(-1)
    ref = torch.as_tensor(ref).detach().cpu().double().reshape(-1)
    return float((got - ref).norm()) / max(float(ref.norm()), 1e-30)


def load_fixture(golden_dir, tag):
    fx = np.load(os.path.join(golden_dir, "plain_ae.npz"))
    B, T, D, H, L, n_steps, seed = [int(v) for v in fx[f"{tag}/cfg"]]
    p, lr, w1, w2, w3 = [float(v) for v in fx[f"{tag}/cfg_f"]]
    args = make_args(rep_learning_dim=D, hidden_size=H, n_layers=L, dropout_prob=p, n_poses=T, learning_rate=lr,
                     loss_l1_weight=w1, loss_cont_weight=w2, loss_var_weight=w3)
    sd = plain_state(D, H, seed)
    for k, v in sd.items():
        assert hashlib.sha256(v.contiguous().numpy().tobytes()).hexdigest() == str(fx[f"{tag}/w0_sha256/{k}"]), k
    return fx, (B, T, D, H, n_steps), args, sd


def fixture_masks(fx, key, B, T, D, H, p):
    m = {"dec": O.unpack_mask(fx[f"{key}/mask_dec"], (T - 1, B, D)).to(DEV)}
    if p > 0:
        m["in"] = O.unpack_mask(fx[f"{key}/mask_in"], (T, B, D)).to(DEV)
        m["dec_l0"] = O.unpack_mask(fx[f"{key}/mask_dec_l0"], (T - 1, B, H)).to(DEV)
    return m


def ref_scale(fx, head, name):
    key = f"{head}/{name}"
    return float(np.abs(fx[key]).max()) if key in fx.files else float(fx[f"{head}_norm/{name}"])


def check_ref(got, fx, head, name, tol):
    """`got` against the reference's tensor head/name: whole (max-abs error relative to its max-abs value) or, for the big ones,
    through its float64 L2 norm + strided sample (head_norm/name, head_sample/name)"""
    key = f"{head}/{name}"
    if key in fx.files:
        err = relerr(got, fx[key])
        assert err < tol, (key, err)
        return
    g = got.detach().cpu().double().reshape(-1)
    ref_n = float(fx[f"{head}_norm/{name}"])
    assert abs(float(g.norm()) - ref_n) <= tol * ref_n, (key, "norm", float(g.norm()), ref_n)
    s = fx[f"{head}_sample/{name}"].astype(np.float64)
    err = float(np.abs(g.numpy()[sample_index(g.numel())] - s).max()) / max(float(np.abs(s).max()), 1e-30)
    assert err < tol, (key, "sample", err)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_train_iterations_match_reference_golden(golden_dir, tag):
    """(a) two iterations with every dropout active, (b) one at config/seq2seq.yml's dimensions: the loss train_iter returns
    (custom_loss alone, whatever the epoch), the encoder states the decoder starts from, the reconstructed poses, every step-1
    gradient, the state after the last step (BatchNorm running statistics included) and an eval-mode forward, against the
    reference's own numbers."""
    from gesture2vec_amd.model.Autoencoder_VQVAE_model import Autoencoder_VQVAE
    from gesture2vec_amd.train_eval.train_seq2seq import FusedClipAdam, train_iter_Autoencoder_VQ_seq2seq
    fx, (B, T, D, H, n_steps), args, sd0 = load_fixture(golden_dir, tag)
    p, lr = args.dropout_prob, args.learning_rate
    net = Autoencoder_VQVAE(args, D, T)
    assert net.vq is False and not hasattr(net, "vq_layer")
    net.load_state_dict(sd0, strict=True)
    net = net.to(DEV)
    net.train(True)
    optim = FusedClipAdam(net, lr=lr, betas=(0.5, 0.999))
    x = torch.from_numpy(fx[f"{tag}/x"].copy()).to(DEV)
    for step in range(1, n_steps + 1):
        m = fixture_masks(fx, f"{tag}/s{step}", B, T, D, H, p)
        net.set_dropout_masks(m["dec"], m.get("in"), m.get("dec_l0"))
        ret = train_iter_Autoencoder_VQ_seq2seq(args, step, x, x, net, optim)     # (the reference ran epochs 1, 2: no effect)
        assert isinstance(ret, dict) and set(ret) == {"loss"}, ret
        ref = float(fx[f"{tag}/s{step}/loss"])
        assert abs(ret["loss"] - ref) <= 2e-6 * abs(ref), (ret["loss"], ref)
        eng = net.engine()
        b = eng.buffers(B)
        assert relerr(b["enc_hidden"], fx[f"{tag}/s{step}/encoder_hidden"]) < 1e-4
        assert relerr(b["y"].transpose(0, 1), fx[f"{tag}/s{step}/outputs"]) < 1e-4, "reconstructed poses"
        if step == 1:
            names = [k.split("/", 3)[3] for k in fx.files
                     if k.startswith(f"{tag}/s1/grad/") or k.startswith(f"{tag}/s1/grad_norm/")]
            assert sorted(names) == sorted(n for n, _ in eng.layout), "the trainable set differs from the reference's"
            for n in names:
                g = eng.view(n, True)
                scale = ref_scale(fx, f"{tag}/s1/grad", n)
                if n == PRE_B:
                    assert float(g.abs().max()) < 1e-6 and scale < 1e-5
                elif scale == 0.0:
                    assert float(g.abs().max()) == 0.0, n          # encoder GRU layer 1: dead compute, exactly zero
                else:
                    check_ref(g, fx, f"{tag}/s1/grad", n, 1e-4)
    after = net.state_dict()
    for n, v in after.items():
        if n in (PRE_B, BN + "running_mean"):
            # Adam turns the pre-BatchNorm bias gradient's rounding noise into +-lr steps (running_mean follows that bias)
            assert float((v.cpu() - torch.from_numpy(fx[f"{tag}/wN/{n}"])).abs().max()) <= 1.01 * n_steps * lr, n
        elif not v.dtype.is_floating_point:
            assert np.array_equal(v.cpu().numpy(), fx[f"{tag}/wN/{n}"]), n
        else:
            check_ref(v, fx, f"{tag}/wN", n, 1e-5)
    # eval mode: BatchNorm on its running statistics, the inline Dropout(0.95) still on
    if tag == "a":
        net.load_state_dict({n: torch.from_numpy(fx[f"a/wN/{n}"].copy()) for n in after}, strict=True)
    else:
        with torch.no_grad():       # the reference's values of the tensors the step's rounding noise moves (above)
            for n in (PRE_B, BN + "running_mean", BN + "running_var"):
                after[n].copy_(torch.from_numpy(fx[f"{tag}/wN/{n}"].copy()))
    net.train(False)
    state = {n: v.clone() for n, v in net.state_dict().items()}
    net.set_dropout_masks(O.unpack_mask(fx[f"{tag}/eval/mask_dec"], (T - 1, B, D)).to(DEV))
    with torch.no_grad():
        res = net(x, x)
    assert len(res) == 2
    outputs, first_hidden = res
    assert outputs.shape == (B, T, D) and first_hidden.shape == (2, B, H)
    assert relerr(outputs, fx[f"{tag}/eval/outputs"]) < 1e-4
    assert relerr(first_hidden, fx[f"{tag}/eval/first_hidden"]) < 1e-4
    for n, v in net.state_dict().items():
        assert torch.equal(v, state[n]), n                      # eval mode moves no state


def _oracle_step(sd, adam, x, masks, p, lr, forced):
    """train_iter_Autoencoder_VQ_seq2seq without a quantiser (train_seq2seq.py:702-707, 740-744) from the oracle's pieces:
    Autoencoder_VQVAE.forward with vq == False (:956-1054: encoder_hidden[:L] straight into the decoder), custom_loss alone, clip 5,
    Adam.  sd / adam are updated in place.  forced: the discrete decisions of the run under test (see test_gpu_vqvae.py)."""
    keys = O.vqvae_trainable_keys(sd)
    leaves = {k: sd[k].detach().clone().requires_grad_(True) for k in keys}
    w = dict(sd)
    w.update(leaves)
    xt = x.transpose(0, 1)
    _, enc_hidden = O.encoder_forward(O.dropout_apply(xt, masks.get("in"), p), w, 2, p, [masks["enc_l0"]] if p > 0 else None)
    hidden = enc_hidden[:2].contiguous()
    bn = {"running_mean": sd[BN + "running_mean"], "running_var": sd[BN + "running_var"],
          "num_batches_tracked": sd[BN + "num_batches_tracked"]}
    outs, dec_in = [xt[0]], xt[0]
    for t in range(1, xt.shape[0]):
        y, hidden = O.decoder_step(dec_in, hidden, w, 2, True, masks["dec"][t - 1], p, masks["dec_l0"][t - 1] if p > 0 else None,
                                   bn, True, relu_mask=forced["relu"][t - 1])
        outs.append(y)
        dec_in = y                                                   # n_pre_poses == 1
    out = torch.stack(outs).transpose(0, 1)
    loss = O.custom_loss(out, x, 5.0, 0.1, 0.5, forced)
    gl = torch.autograd.grad(loss, [leaves[k] for k in keys], allow_unused=True)
    grads = {k: (g if g is not None else torch.zeros_like(leaves[k])) for k, g in zip(keys, gl)}
    raw = {k: g.clone() for k, g in grads.items()}
    clipped, gnorm = O.clip_grad_norm(grads, 5.0)
    params = {k: sd[k] for k in keys}
    O.adam_step(params, clipped, adam, lr)
    sd.update(params)
    sd[BN + "running_mean"], sd[BN + "running_var"] = bn["running_mean"], bn["running_var"]
    return {"loss": loss.detach(), "outputs": out.detach(), "first_hidden": enc_hidden[:2].detach(), "grads": raw,
            "grad_norm": gnorm}


@pytest.mark.parametrize("T,D,H,p", [(20, 40, 200, 0.0), (34, 135, 64, 0.2)])
def test_large_batch_step_vs_oracle(T, D, H, p):
    """B = 4096: the engine's quantizer="none" step against the float64 oracle built above, with the DISCRETE decisions (the
    decoder's ReLU pattern, the signs of custom_loss's |.| terms) pinned to the kernels' as test_gpu_vqvae.py does; the pinned
    signs are the oracle's own wherever its argument is clear of the rounding band."""
    from gesture2vec_amd.engine import VQVAEEngine
    B, lr = 4096, 5e-4
    sd = plain_state(D, H, seed=3)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, T, D, generator=g)
    masks = {"dec": (torch.rand(T - 1, B, D, generator=g) < 0.05).to(torch.uint8)}
    if p > 0:
        masks["in"] = (torch.rand(T, B, D, generator=g) < 1 - p).to(torch.uint8)
        masks["enc_l0"] = torch.ones(T, B, 2 * H, dtype=torch.uint8)      # layer 1 is dead compute: any mask works
        masks["dec_l0"] = (torch.rand(T - 1, B, H, generator=g) < 1 - p).to(torch.uint8)
    eng = VQVAEEngine(D, H, 2, 0, T, beta=0.0, dropout_prob=p, device=DEV, quantizer="none")
    assert eng.comm.numel() == eng.n_flat + 4 and eng.vq_stats is None and eng.vq_scalars is None and eng.codebook is None
    for name, _ in eng.layout:
        eng.view(name).copy_(sd[name])
    xd = x.to(DEV)
    eng.set_masks(B, masks["dec"].to(DEV), masks["in"].to(DEV) if p > 0 else None, masks["dec_l0"].to(DEV) if p > 0 else None)
    eng.train_step(xd, xd, lr=lr, w_l1=5.0, w_cont=0.1, w_var=0.5, draw_masks=False)
    torch.cuda.synchronize()
    b = eng.buffers(B)
    assert "quant" not in b and "idx" not in b and "ws_stats" not in b
    y = b["y"].transpose(0, 1)
    forced = {"relu": (b["a"] > 0).cpu().double(), "sign_l1": torch.sign(y - xd).cpu().double(),
              "sign_cont": torch.sign(y[:, 1:] - y[:, :-1]).cpu().double()}
    sd64, x64 = as64(sd), x.double()
    with default64():
        r = _oracle_step(sd64, {}, x64, masks, p, lr, forced)
    ro = r["outputs"]
    clear = (ro - x64).abs() > 1e-5 * (1 + ro.abs())
    assert torch.equal(torch.sign(ro - x64)[clear], forced["sign_l1"][clear]), "sign(y - target) outside the rounding band"
    dc = ro[:, 1:] - ro[:, :-1]
    clear = dc.abs() > 1e-5 * (1 + ro[:, 1:].abs())
    assert torch.equal(torch.sign(dc)[clear], forced["sign_cont"][clear]), "sign(y_t - y_{t-1}) outside the rounding band"
    assert relerr(b["enc_hidden"], r["first_hidden"]) < 1e-4
    assert relerr(y, ro) < 1e-4, "reconstructed poses"
    rb = eng.readback.tolist()
    assert abs(rb[0] - float(r["loss"])) <= 1e-5 * abs(float(r["loss"]))
    assert rb[1] == 0.0 and rb[2] == 0.0 and rb[3] == 0.0         # no loss_vq / perplexity; no fault
    assert abs(eng.gnorm.item() - float(r["grad_norm"])) <= 2e-4 * float(r["grad_norm"])
    for name, _ in eng.layout:
        if name == PRE_B:
            continue
        ref, got = r["grads"][name], eng.view(name, True)
        if float(ref.abs().max()) == 0.0:
            assert float(got.abs().max()) == 0.0, name                 # encoder layer 1: exactly zero
        else:
            assert relerr_l2(got, ref) < 2e-5, (name, relerr_l2(got, ref))
            assert relerr(got, ref) < 5e-5, (name, relerr(got, ref))
    for name, _ in eng.layout:
        if name == PRE_B:
            continue
        # the first Adam step is ~lr * sign(g): an element whose gradient is inside the rounding band may take the other sign
        diff = (eng.view(name).cpu().double() - sd64[name]).abs()
        n_off = int((diff > 0.1 * lr).sum())
        assert float(diff.max()) <= 2.1 * lr and n_off <= max(2, diff.numel() // 500), (name, float(diff.max()), n_off)
    assert relerr(eng.bn_rv, sd64[BN + "running_var"]) < 1e-4


def _net(B_seed=3):
    from gesture2vec_amd.model.Autoencoder_VQVAE_model import Autoencoder_VQVAE
    args = make_args()
    torch.manual_seed(B_seed)
    net = Autoencoder_VQVAE(args, 40, 20).to(DEV)
    net.train(True)
    net.rng_seed = 11
    return args, net


@pytest.mark.parametrize("B", [128, 4096])
def test_train_iter_replayed_from_a_graph_equals_eager_iterations(monkeypatch, B):
    """config/seq2seq.yml's dims: at B = 128 the step runs on the cluster kernels, at 4096 on the large-batch ones.  Through the
    replayed-graph route (first iteration eager, second captures, later ones replay; a new input tensor every iteration) the
    losses, weights, Adam moments and BatchNorm statistics are bitwise those of the same iterations run eagerly."""
    import gesture2vec_amd.train_eval.train_seq2seq as ts
    runs = {}
    for mode in ("graph", "eager"):
        monkeypatch.setattr(ts, "_GRAPH_REPLAY", mode == "graph")
        args, net = _net()
        optim = ts.FusedClipAdam(net, 5e-4, betas=(0.5, 0.999))
        g = torch.Generator(device=DEV).manual_seed(5)
        losses = []
        for _ in range(5):
            x = torch.randn(B, 20, 40, generator=g, device=DEV)
            ret = ts.train_iter_Autoencoder_VQ_seq2seq(args, 1, x, x, net, optim)
            assert set(ret) == {"loss"}
            losses.append(ret["loss"])
        eng = net.engine()
        if mode == "graph":
            assert eng._iter_graph["graph"] not in (None, False), "the iteration was not replayed from a graph"
        runs[mode] = (losses, eng.flat.clone(), eng.m.clone(), eng.v.clone(), eng.bn_rm.clone(), eng.bn_rv.clone(),
                      int(net.decoder.decoder.pre_linear[1].num_batches_tracked))
    a, b = runs["graph"], runs["eager"]
    assert a[0] == b[0], (a[0], b[0])
    for ta, tb in zip(a[1:6], b[1:6]):
        assert torch.equal(ta, tb)
    assert a[6] == b[6] == 5 * 19


def test_two_half_batch_shards_equal_one_full_batch_step():
    """Data parallelism on one GPU: two engines play rank 0 / rank 1 (train_step_local on a half batch each, comm buffers summed by
    hand as the RCCL SUM all-reduce would, train_step_apply(world=2, dp=True)) against one engine's full-batch step.  The full
    batch is the shard twice, so BatchNorm's batch statistics -- per rank under data parallelism -- are the same: the two agree up
    to summation order.  comm = [grads | fault flag]: no statistics slots."""
    from gesture2vec_amd.engine import VQVAEEngine
    B, T, D, H, lr = 128, 20, 40, 200, 5e-4
    sd = plain_state(D, H, seed=7)
    g = torch.Generator().manual_seed(9)
    half = torch.randn(B // 2, T, D, generator=g).to(DEV)
    keep_half = (torch.rand(T - 1, B // 2, D, generator=g) < 0.05).to(torch.uint8).to(DEV)
    full, keep_full = torch.cat([half, half]), torch.cat([keep_half, keep_half], dim=1)
    kw = dict(w_l1=5.0, w_cont=0.1, w_var=0.5, draw_masks=False)

    def engine():
        eng = VQVAEEngine(D, H, 2, 0, T, beta=0.0, dropout_prob=0.0, device=DEV, quantizer="none")
        for name, _ in eng.layout:
            eng.view(name).copy_(sd[name])
        return eng

    ref = engine()
    ref.set_masks(B, keep_full)
    ref.train_step_local(full, full, **kw)
    torch.cuda.synchronize()
    ref_grads = ref.gflat.clone()
    ref.train_step_apply(B, lr=lr)
    ranks = [engine(), engine()]
    for eng in ranks:
        assert eng.comm.numel() == eng.n_flat + 4 and eng.vq_stats is None
        eng.set_masks(B // 2, keep_half)
        eng.train_step_local(half, half, dp=True, **kw)
    torch.cuda.synchronize()
    total = ranks[0].comm + ranks[1].comm
    assert float(total[ranks[0].n_flat:].abs().max()) == 0.0          # no rank latched a fault
    for name, _ in ref.layout:
        if name == PRE_B:
            continue
        off, n, _ = ref.offsets[name]
        got, want = total[off:off + n] / 2, ref_grads[off:off + n]
        if float(want.abs().max()) == 0.0:
            assert float(got.abs().max()) == 0.0, name
        else:
            assert relerr(got, want) < 1e-5, (name, relerr(got, want))
    for eng in ranks:
        eng.comm.copy_(total)
        eng.train_step_apply(B // 2, lr=lr, world=2, dp=True)
    torch.cuda.synchronize()
    assert torch.equal(ranks[0].flat, ranks[1].flat)                   # replicas bit-identical
    assert abs(ranks[0].gnorm.item() - ref.gnorm.item()) <= 1e-5 * ref.gnorm.item()
    assert abs(ranks[0].readback[0].item() - ref.readback[0].item()) <= 1e-5 * abs(ref.readback[0].item())
    for name, _ in ref.layout:
        if name == PRE_B:
            continue
        err = float((ranks[0].view(name) - ref.view(name)).abs().max())
        assert err <= 1e-5 * float(ref.view(name).abs().max()) + 0.02 * lr, (name, err)


def test_trainer_end_to_end_checkpoint_and_bit_identical_resume(tmp_path):
    """scripts/train_autoencoder_VQVAE.py with config/AE_plain_synthetic.yml (the keys of the reference's seq2seq.yml): epochs,
    evaluation, the reference's checkpoint layout without quantiser tensors, reload through load_checkpoint_and_model, and a run
    resumed from the epoch-2 checkpoint writing the same epoch-4 checkpoint bit for bit."""
    def run(out, extra):
        cmd = [sys.executable, os.path.join(ROOT, "scripts", "train_autoencoder_VQVAE.py"),
               "--config", os.path.join(ROOT, "config", "AE_plain_synthetic.yml"), "--synthetic", "--synthetic_batches", "3",
               "--batch_size", "64", "--epochs", "4", "--save_every", "2", "--model_save_path", out, "--name", "t"] + extra
        r = subprocess.run(cmd, cwd=os.path.join(ROOT, "scripts"), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        return r.stderr + r.stdout
    a, b = os.path.join(tmp_path, "full"), os.path.join(tmp_path, "resumed")
    log = run(a, [])
    ep = [l for l in log.splitlines() if "samples/s | loss:" in l]
    assert "[VAL] loss:" in log and any("EP 2 (  3) |" in l for l in ep) and any("EP 4 (  3) |" in l for l in ep)
    assert not any("perplex" in l.lower() for l in ep)
    ck2 = os.path.join(a, "t_checkpoint_002.bin")
    raw = torch.load(ck2, map_location="cpu", weights_only=False)
    assert {"args", "epoch", "lang_model", "pose_dim", "gen_dict"} <= set(raw) and raw["pose_dim"] == 40
    assert raw["args"].autoencoder_vq == "False" and not any(k.startswith("vq_layer.") for k in raw["gen_dict"])
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import utils.train_utils as tu
    args, net, loss_fn, lang, pose_dim = tu.load_checkpoint_and_model(ck2, DEV, "autoencoder_vq")
    assert net.vq is False and not net.training
    x = torch.randn(8, 20, 40, device=DEV)
    with torch.no_grad():
        res = net(x, x)
    assert len(res) == 2 and res[0].shape == (8, 20, 40) and torch.isfinite(res[0]).all()
    run(b, ["--resume", ck2])
    ca = torch.load(os.path.join(a, "t_checkpoint_004.bin"), map_location="cpu", weights_only=False)
    cb = torch.load(os.path.join(b, "t_checkpoint_004.bin"), map_location="cpu", weights_only=False)
    assert set(ca["gen_dict"]) == set(cb["gen_dict"])
    for k in ca["gen_dict"]:
        assert torch.equal(ca["gen_dict"][k], cb["gen_dict"][k]), k
    assert torch.equal(ca["resume"]["optim"]["m"], cb["resume"]["optim"]["m"])
    assert ca["loss_list"] == cb["loss_list"]


def test_reference_checkpoint_eval_forward(golden_dir):
    """tests/golden/plain_ae_ckpt.bin (the reference's save path, autoencoder_vq "False") loads on the GPU and its eval forward, with
    the fixture's Dropout(0.95) masks, reproduces the reference's outputs"""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from utils.train_utils import load_checkpoint_and_model
    args, net, _, lang, pose_dim = load_checkpoint_and_model(os.path.join(golden_dir, "plain_ae_ckpt.bin"), DEV, "autoencoder_vq")
    assert net.vq is False and not hasattr(net, "vq_layer") and not net.training and pose_dim == 40
    fx = np.load(os.path.join(golden_dir, "plain_ae.npz"))
    B, T, D, H = [int(v) for v in fx["a/cfg"][:4]]
    x = torch.from_numpy(fx["a/x"].copy()).to(DEV)
    net.set_dropout_masks(O.unpack_mask(fx["a/eval/mask_dec"], (T - 1, B, D)).to(DEV))
    with torch.no_grad():
        outputs, first_hidden = net(x, x)
    assert relerr(outputs, fx["a/eval/outputs"]) < 1e-4
    assert relerr(first_hidden, fx["a/eval/first_hidden"]) < 1e-4
