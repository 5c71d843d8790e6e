"""GPU: the variational chunk autoencoder (autoencoder_vae == "True") through every layer -- g2v_vae_latent_fwd / _bwd against the
float64 restatement (tests/_vae_ref.py), the in-kernel noise, the module and train_iter_Autoencoder_VQ_seq2seq against the
reference's own numbers (tests/golden/vae.npz, make_fixtures_vae.py), the checkpoint loader and the latent extraction -- plus the
refusals (data parallel, the fused step) and the guard that no other configuration's flat layout moved.

The kernels' bar (test 1) is not a constant: for every quantity the error of a plain fp32 CPU evaluation of the same formulas
(_vae_ref.latent_block_fp32) against float64 on the same inputs is measured, and the kernel is allowed 4x that -- room for
another, equally valid summation order, not for another algorithm.  Error = relative L2 distance (a max over the 64 elements of
the smallest shape would be a lottery); floor 2^-24, the unit roundoff: a correctly rounded fp32 result is no closer than that, and
a yardstick that happens to hit a scalar exactly must not demand the impossible."""
import argparse
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

import _vae_ref as R
from _h200 import sample_index
from oracle import g2v_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BN = "decoder.decoder.pre_linear.1."
PRE_B = "decoder.decoder.pre_linear.0.bias"      # feeds BatchNorm in training: its gradient is rounding noise on both sides
U = 2.0 ** -24


def rel_l2(got, ref):
    got, ref = torch.as_tensor(got).detach().cpu().double().reshape(-1), torch.as_tensor(ref).detach().cpu().double().reshape(-1)
    return float((got - ref).norm()) / max(float(ref.norm()), 1e-300)


def relerr(got, ref):
    got = got.detach().cpu().double().reshape(-1)
    ref = torch.as_tensor(ref).detach().cpu().double().reshape(-1)
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-12)


def block_inputs(B, E, seed):
    L, H = 2, E // 2
    g = torch.Generator().manual_seed(100 + seed)
    h = torch.tanh(torch.randn(L, B, H, generator=g))                  # a GRU state
    eps = torch.randn(B, E, generator=g)
    g_d = torch.randn(L, B, H, generator=g) * 0.1
    return h, R.vae_state(E, seed), eps, g_d


# ---------------------------------------------------------------------------------------------- 1. kernels against float64
@pytest.fixture(scope="module")
def block_refs():
    """float64 reference and fp32 yardstick per (B, E, g_kl), computed once and shared"""
    cache = {}

    def get(B, E, g_kl):
        key = (B, E, g_kl)
        if key not in cache:
            h, w, eps, g_d = block_inputs(B, E, seed=B + E)
            f64, g64 = R.latent_block_grads(h, w, eps, g_d, g_kl)
            ref = {**{k: f64[k] for k in ("mean", "logvar", "z", "d", "kl", "hf")}, **{k: g64[k] for k in ("dh", "dmean", "dlogvar")}}
            cache[key] = ((h, w, eps, g_d), ref, R.latent_block_fp32(h, w, eps, g_d, g_kl))
        return cache[key]
    return get


@pytest.mark.parametrize("g_kl", [0.0, 0.37])
@pytest.mark.parametrize("B,E", [(1, 64), (8, 64), (33, 128), (128, 400), (513, 400)])
def test_kernels_against_float64(block_refs, B, E, g_kl):
    """explicit eps; mean, logvar, z, d, KL, dh, dmean, dlogvar.  d and dh are compared in their (L,B,H) layout: at E = 400 the
    layer boundary (H = 200) falls inside a 16-wide tile of the row, so a swapped or shifted layer segment fails here."""
    from gesture2vec_amd import ops
    (h, w, eps, g_d), ref, f32 = block_refs(B, E, g_kl)
    wd = {n: v.to(DEV) for n, v in w.items()}
    o = ops.vae_latent_fwd(h.to(DEV), wd["VAE_fc_mean.weight"], wd["VAE_fc_mean.bias"], wd["VAE_fc_std.weight"], wd["VAE_fc_std.bias"],
                           wd["VAE_fc_decoder.weight"], wd["VAE_fc_decoder.bias"], eps=eps.to(DEV))
    gk = torch.full((1,), g_kl, device=DEV) if g_kl != 0.0 else None
    dh, dmean, dlogvar = ops.vae_latent_bwd(g_d.to(DEV), gk, o["mean"], o["logvar"], o["eps"], wd["VAE_fc_mean.weight"],
                                            wd["VAE_fc_std.weight"], wd["VAE_fc_decoder.weight"])
    torch.cuda.synchronize()
    assert o["d"].shape == (2, B, E // 2) and dh.shape == (2, B, E // 2)
    assert torch.equal(o["hf"].cpu(), h.transpose(1, 0).reshape(B, E)), "the gathered rows are a copy of h"
    got = {"mean": o["mean"], "logvar": o["logvar"], "z": o["z"], "d": o["d"], "kl": o["kl"][0], "dh": dh, "dmean": dmean,
           "dlogvar": dlogvar}
    report = {}
    for n, v in got.items():
        yard = max(rel_l2(f32[n], ref[n]), U)
        report[n] = (rel_l2(v, ref[n]), yard)
    print(f"\n[vae_latent B={B} E={E} g_kl={g_kl}] " + " ".join(f"{n}={e:.2e}/{y:.2e}" for n, (e, y) in report.items()))
    for n, (e, y) in report.items():
        assert e <= 4 * y, (n, e, y)


def test_unserved_shapes_are_rejected_without_a_launch():
    from gesture2vec_amd import _lib, ops
    assert ops.vae_latent_ok(1, 64) and ops.vae_latent_ok(513, 400) and ops.vae_latent_ok(7, 512)
    assert not ops.vae_latent_ok(8, 72) and not ops.vae_latent_ok(8, 528) and not ops.vae_latent_ok(0, 64)
    h = torch.zeros(2, 4, 36, device=DEV)                              # E = 72: not a multiple of 16
    w, b = torch.zeros(72, 72, device=DEV), torch.zeros(72, device=DEV)
    with pytest.raises(_lib.G2VLibraryError, match="g2v_vae_latent_ok"):
        ops.vae_latent_fwd(h, w, b, w, b, w, b, eps=torch.zeros(4, 72, device=DEV))
    with pytest.raises(_lib.G2VLibraryError, match="g2v_vae_latent_ok"):
        ops.vae_latent_bwd(h, None, torch.zeros(4, 72, device=DEV), torch.zeros(4, 72, device=DEV), None, w, w, w)


# ---------------------------------------------------------------------------------------------- 2. in-kernel noise
def test_in_kernel_noise():
    """Philox + Box-Muller inside the kernel: reproducible from (seed, counter), the counter advances, z is formed from the eps that
    is written out, the moments of N = 64 * 400 draws sit inside their five-sigma bands (|mean| < 5 / sqrt(N); the variance of
    N normal draws has standard deviation sqrt(2 / N): |var - 1| < 5 sqrt(2 / N)), and sample = 0 gives z = mean bit for bit."""
    from gesture2vec_amd import ops
    B, E = 64, 400
    h, w, _, _ = block_inputs(B, E, seed=9)
    wd = {n: v.to(DEV) for n, v in w.items()}
    hd = h.to(DEV)
    args = (hd, wd["VAE_fc_mean.weight"], wd["VAE_fc_mean.bias"], wd["VAE_fc_std.weight"], wd["VAE_fc_std.bias"],
            wd["VAE_fc_decoder.weight"], wd["VAE_fc_decoder.bias"])
    counter = torch.full((1,), 5, dtype=torch.int64, device=DEV)
    a = ops.vae_latent_fwd(*args, seed=1234, offset_counter=counter)
    assert int(counter.item()) == 6, "the counter advances by one per drawing call"
    b = ops.vae_latent_fwd(*args, seed=1234, offset_counter=counter)
    counter.fill_(5)
    c = ops.vae_latent_fwd(*args, seed=1234, offset_counter=counter)
    other = ops.vae_latent_fwd(*args, seed=1235, offset_counter=torch.full((1,), 5, dtype=torch.int64, device=DEV))
    for n in ("eps", "z", "d", "mean", "logvar", "kl"):
        assert torch.equal(a[n], c[n]), f"{n}: the same seed and counter must give the same bits"
    assert not torch.equal(a["eps"], b["eps"]) and not torch.equal(a["eps"], other["eps"])
    assert torch.equal(a["mean"], b["mean"]) and torch.equal(a["kl"], b["kl"])          # the noise touches z and d only
    eps, mean, logvar, z = (a[n].cpu().double() for n in ("eps", "mean", "logvar", "z"))
    noise = torch.exp(logvar / 2) * eps
    assert bool(((z - (mean + noise)).abs() <= 4 * 2.0 ** -23 * (mean.abs() + noise.abs())).all()), "z = mean + exp(logvar / 2) eps"
    N = B * E
    m, v = float(eps.mean()), float(eps.var(unbiased=True))
    print(f"\n[vae noise] N={N} mean={m:.3e} (band {5 / N ** 0.5:.3e}) var-1={v - 1:.3e} (band {5 * (2 / N) ** 0.5:.3e}) "
          f"max|eps|={float(eps.abs().max()):.2f}")
    assert abs(m) < 5 / N ** 0.5 and abs(v - 1) < 5 * (2 / N) ** 0.5
    assert bool(torch.isfinite(a["eps"]).all())
    before = int(counter.item())
    s0 = ops.vae_latent_fwd(*args, seed=1234, offset_counter=counter, sample=False)
    assert torch.equal(s0["z"], s0["mean"]) and s0["eps"] is None and int(counter.item()) == before
    assert torch.equal(s0["mean"], a["mean"]) and torch.equal(s0["logvar"], a["logvar"])


# ---------------------------------------------------------------------------------------------- 3. module + train_iter
def make_args(**kw):
    d = dict(rep_learning_dim=40, hidden_size=200, n_layers=2, dropout_prob=0.0, autoencoder_vae="True", autoencoder_vq="False",
             autoencoder_vq_components=512, autoencoder_vq_commitment_cost=0.25, n_pre_poses=1, autoencoder_conditioned="True",
             autoencoder_att="False", autoencoder_fixed_weight="False", n_poses=20, loss_l1_weight=5.0, loss_cont_weight=0.1,
             loss_var_weight=0.5, learning_rate=5e-4, epochs=10)
    d.update(kw)
    return argparse.Namespace(**d)


def load_fixture(golden_dir, tag):
    fx = np.load(os.path.join(golden_dir, "vae.npz"))
    B, T, D, H, L, n_steps, seed, K, epochs = [int(v) for v in fx[f"{tag}/cfg"]]
    p, lr, w1, w2, w3, beta = [float(v) for v in fx[f"{tag}/cfg_f"]]
    args = make_args(rep_learning_dim=D, hidden_size=H, n_layers=L, dropout_prob=p, n_poses=T, learning_rate=lr, loss_l1_weight=w1,
                     loss_cont_weight=w2, loss_var_weight=w3, epochs=epochs, autoencoder_vq="True" if K else "False",
                     autoencoder_vq_components=K or 512, autoencoder_vq_commitment_cost=beta)
    if K:
        args.autoencoder_vq_quantizer = "gssoft"          # the quantiser the reference ships (what load_checkpoint_and_model sets)
    sd = {k: v for k, v in O.init_vqvae_state(D, H, 2, 1, seed=seed).items() if not k.startswith("vq_layer.")}
    sd.update(R.vae_state(L * H, seed))
    for k, v in sd.items():
        assert hashlib.sha256(v.contiguous().numpy().tobytes()).hexdigest() == str(fx[f"{tag}/w0_sha256/{k}"]), k
    sd.update({k[len(f"{tag}/w0/"):]: torch.from_numpy(fx[k].copy()) for k in fx.files if k.startswith(f"{tag}/w0/")})
    x = torch.randn(B, T, D, generator=torch.Generator().manual_seed(1234 + seed))
    assert hashlib.sha256(x.numpy().tobytes()).hexdigest() == str(fx[f"{tag}/x_sha256"])
    return fx, (B, T, D, H, n_steps, bool(K)), args, sd, x.to(DEV)


def fixture_masks(fx, key, B, T, D, H, p):
    m = {"dec": O.unpack_mask(fx[f"{key}/mask_dec"], (T - 1, B, D)).to(DEV)}
    if p > 0 and f"{key}/mask_in" in fx.files:
        m["in"] = O.unpack_mask(fx[f"{key}/mask_in"], (T, B, D)).to(DEV)
        m["dec_l0"] = O.unpack_mask(fx[f"{key}/mask_dec_l0"], (T - 1, B, H)).to(DEV)
    return m


def ref_scale(fx, head, name):
    key = f"{head}/{name}"
    return float(np.abs(fx[key]).max()) if key in fx.files else float(fx[f"{head}_norm/{name}"])


def check_ref(got, fx, head, name, tol):
    """tests/test_gpu_plain_autoencoder.py's check: whole (max-abs error relative to the max-abs value) or, for the big tensors,
    through the float64 L2 norm + strided sample"""
    key = f"{head}/{name}"
    if key in fx.files:
        err = relerr(got, fx[key])
        assert err < tol, (key, err)
        return err
    g = got.detach().cpu().double().reshape(-1)
    ref_n = float(fx[f"{head}_norm/{name}"])
    assert abs(float(g.norm()) - ref_n) <= tol * ref_n, (key, "norm", float(g.norm()), ref_n)
    s = fx[f"{head}_sample/{name}"].astype(np.float64)
    err = float(np.abs(g.numpy()[sample_index(g.numel())] - s).max()) / max(float(np.abs(s).max()), 1e-30)
    assert err < tol, (key, "sample", err)
    return err


def eval_check(net, fx, tag, x, B, T, D, with_vq):
    net.train(False)
    state = {n: v.clone() for n, v in net.state_dict().items()}
    net.set_dropout_masks(O.unpack_mask(fx[f"{tag}/eval/mask_dec"], (T - 1, B, D)).to(DEV))
    net.set_latent_noise(torch.from_numpy(fx[f"{tag}/eval/eps"].copy()).to(DEV))       # the forward draws noise in eval mode too
    with torch.no_grad():
        res = net(x, x)
    assert isinstance(res, tuple) and len(res) == (6 if with_vq else 4)
    assert res[0].shape == (B, T, D) and res[1].shape == (2, B, net.hidden_size) and res[2].shape == res[3].shape == (B, 2 * net.hidden_size)
    for n, v in zip(("outputs", "first_hidden", "mean", "logvar"), res):
        assert relerr(v, fx[f"{tag}/eval/{n}"]) < 1e-4, n
    if with_vq:
        assert abs(float(res[4]) - float(fx[f"{tag}/eval/loss_vq"])) <= 1e-4 * abs(float(fx[f"{tag}/eval/loss_vq"]))
        assert abs(float(res[5]) - float(fx[f"{tag}/eval/perplexity"])) <= 1e-4 * float(fx[f"{tag}/eval/perplexity"])
    for n, v in net.state_dict().items():
        assert torch.equal(v, state[n]), n                      # eval mode moves no state


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_train_iterations_match_reference_golden(golden_dir, tag):
    """(a) epochs 0, 1, 2 with every dropout active, (b) one iteration at the shipped dimensions, (c) shape a behind the soft
    quantiser at the trainer's first epochs 1, 2: recorded masks and noise in, then the loss train_iter returns (no KL term at epoch 0), its return type, outputs,
    first hidden, mean, logvar, every gradient of the epoch-1 step, the state after the last step and an eval-mode forward,
    against the reference's own numbers."""
    from gesture2vec_amd.model.Autoencoder_VQVAE_model import Autoencoder_VQVAE
    from gesture2vec_amd.train_eval.train_seq2seq import FusedClipAdam, train_iter_Autoencoder_VQ_seq2seq
    fx, (B, T, D, H, n_steps, with_vq), args, sd0, x = load_fixture(golden_dir, tag)
    p, lr = args.dropout_prob, args.learning_rate
    net = Autoencoder_VQVAE(args, D, T)
    assert net.VAE is True and net.vq is with_vq
    net.load_state_dict(sd0, strict=True)
    net = net.to(DEV)
    net.train(True)
    optim = FusedClipAdam(net, lr=lr, betas=(0.5, 0.999))
    seen = {}
    hook = net.register_forward_hook(lambda m, i, out: seen.__setitem__("out", out))
    grad_step = int(fx[f"{tag}/grad_step"])
    for step in range(1, n_steps + 1):
        key = f"{tag}/s{step}"
        epoch = int(fx[f"{key}/epoch"])
        m = fixture_masks(fx, key, B, T, D, H, p)
        net.set_dropout_masks(m["dec"], m.get("in"), m.get("dec_l0"))
        net.set_latent_noise(torch.from_numpy(fx[f"{key}/eps"].copy()).to(DEV))
        ret = train_iter_Autoencoder_VQ_seq2seq(args, epoch, x, x, net, optim)
        if with_vq:
            assert isinstance(ret, tuple) and len(ret) == 2 and set(ret[0]) == {"loss"} and torch.is_tensor(ret[1]), ret
            loss = ret[0]["loss"]
            assert abs(float(ret[1]) - float(fx[f"{key}/perplexity"])) <= 1e-4 * float(fx[f"{key}/perplexity"])
        else:
            assert isinstance(ret, dict) and set(ret) == {"loss"}, ret
            loss = ret["loss"]
        out = seen["out"]
        assert len(out) == (6 if with_vq else 4)
        ref = float(fx[f"{key}/loss"])
        print(f"\n[vae {key}] epoch {epoch} loss {loss:.8f} ref {ref:.8f} rel {abs(loss - ref) / abs(ref):.2e} "
              f"kl {float(net.latent_kl.detach()):.8f} ref {float(fx[f'{key}/kld']):.8f}")
        assert abs(loss - ref) <= 2e-6 * abs(ref), (loss, ref)
        assert abs(float(net.latent_kl.detach()) - float(fx[f"{key}/kld"])) <= 1e-4 * float(fx[f"{key}/kld"])
        if epoch == 0:          # the loss at epoch 0 carries no KL term (and no loss_vq): it is custom_loss alone
            assert abs(loss - float(fx[f"{key}/custom_loss"])) <= 2e-6 * abs(ref)
        eng = net.engine()
        b = eng.buffers(B)
        assert relerr(b["enc_hidden"], fx[f"{key}/encoder_hidden"]) < 1e-4
        assert relerr(out[0], fx[f"{key}/outputs"]) < 1e-4, "reconstructed poses"
        assert relerr(out[1], fx[f"{key}/first_hidden"]) < 1e-4
        assert relerr(out[2], fx[f"{key}/mean"]) < 1e-4 and relerr(out[3], fx[f"{key}/logvar"]) < 1e-4
        for n in R.NAMES:
            check_ref(eng.view(n, True), fx, f"{key}/vae_grad", n, 1e-4)
        if step == grad_step:
            names = [k.split("/", 2)[2] for k in fx.files if k.startswith(f"{tag}/grad/") or k.startswith(f"{tag}/grad_norm/")]
            assert sorted(names) == sorted(n for n, _ in eng.layout), "the trainable set differs from the reference's"
            for n in names:
                g = eng.view(n, True)
                scale = ref_scale(fx, f"{tag}/grad", n)
                if n == PRE_B:
                    assert float(g.abs().max()) < 1e-6 and scale < 1e-5
                elif scale == 0.0:
                    assert float(g.abs().max()) == 0.0, n          # encoder GRU layer 1: dead compute, exactly zero
                else:
                    check_ref(g, fx, f"{tag}/grad", n, 1e-4)
    hook.remove()
    after = net.state_dict()
    for n, v in after.items():
        if n in (PRE_B, BN + "running_mean"):
            # Adam turns the pre-BatchNorm bias gradient's rounding noise into +-lr steps (running_mean follows that bias)
            lim = 1.01 * n_steps * lr
            if f"{tag}/wN/{n}" in fx.files:
                assert float((v.cpu() - torch.from_numpy(fx[f"{tag}/wN/{n}"])).abs().max()) <= lim, n
            else:
                s = v.detach().cpu().reshape(-1).numpy()[sample_index(v.numel())]
                assert float(np.abs(s - fx[f"{tag}/wN_sample/{n}"]).max()) <= lim, n
        elif not v.dtype.is_floating_point:
            assert np.array_equal(v.cpu().numpy(), fx[f"{tag}/wN/{n}"]), n
        else:
            check_ref(v, fx, f"{tag}/wN", n, 1e-5)
    # eval mode: BatchNorm on its running statistics, the inline Dropout(0.95) and the latent noise still on
    small = {n: torch.from_numpy(fx[f"{tag}/wN/{n}"].copy()) for n in after if f"{tag}/wN/{n}" in fx.files}
    with torch.no_grad():           # the reference's values of the tensors the steps' rounding noise moves (above)
        for n in (PRE_B, BN + "running_mean", BN + "running_var"):
            if n in small:
                after[n].copy_(small[n])
    if all(n in small for n in (PRE_B, BN + "running_mean", BN + "running_var")):
        eval_check(net, fx, tag, x, B, T, D, with_vq)


# ---------------------------------------------------------------------------------------------- 4. checkpoint and pipeline
def test_reference_checkpoint_loads_and_reproduces_eval(golden_dir):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from utils.train_utils import load_checkpoint_and_model
    fx = np.load(os.path.join(golden_dir, "vae.npz"))
    B, T, D, H, L, _, seed = [int(v) for v in fx["a/cfg"][:7]]
    args, net, _loss_fn, lang_model, pose_dim = load_checkpoint_and_model(os.path.join(golden_dir, "vae_ckpt.bin"), DEV, "autoencoder_vq")
    assert args.autoencoder_vae == "True" and net.VAE and not net.vq and pose_dim == D and not net.training and lang_model.n_words == 13
    x = torch.randn(B, T, D, generator=torch.Generator().manual_seed(1234 + seed)).to(DEV)
    eval_check(net, fx, "a", x, B, T, D, with_vq=False)


@pytest.mark.parametrize("name,vq", [("plain", "False"), ("vq", "True")])
def test_state_dict_keys_on_the_device(golden_dir, name, vq):
    """binding the engine (which re-homes every trainable tensor into the flat buffer) keeps the reference's key set"""
    from gesture2vec_amd.model.Autoencoder_VQVAE_model import Autoencoder_VQVAE
    fx = np.load(os.path.join(golden_dir, "vae.npz"))
    ref = dict(zip((str(k) for k in fx[f"d/{name}/keys"]), (str(s) for s in fx[f"d/{name}/shapes"])))
    net = Autoencoder_VQVAE(make_args(autoencoder_vq=vq, autoencoder_vq_quantizer="gssoft"), 40, 20).to(DEV)
    eng = net.engine()
    assert {k: "x".join(str(s) for s in v.shape) for k, v in net.state_dict().items()} == ref
    assert [n for n, _ in eng.layout][-6:] == list(R.NAMES), "the variational block's tensors close the flat buffer"
    for n in R.NAMES:
        assert net.get_parameter(n).data_ptr() == eng.view(n).data_ptr() and net.get_parameter(n).grad.data_ptr() == eng.view(n, True).data_ptr()


def test_chunk_latents_and_codes():
    """chunk_latents of a variational net = VAE_fc_decoder(VAE_fc_mean(hf)) (the extractors' reparameterize(train=False)), against
    the float64 restatement on the encoder state the device computed, under the kernels' bar; chunks_to_codes / KMeans run on it"""
    from gesture2vec_amd.kmeans import KMeans
    from gesture2vec_amd.model.Autoencoder_VQVAE_model import Autoencoder_VQVAE
    from gesture2vec_amd.pipeline import chunk_latents, chunks_to_codes
    torch.manual_seed(5)
    net = Autoencoder_VQVAE(make_args(), 40, 20).to(DEV)
    net.train(False)
    N = 37
    x = torch.randn(N, 20, 40, generator=torch.Generator().manual_seed(6)).to(DEV)
    with torch.no_grad():
        _, hidden = net.encoder(x.transpose(0, 1).contiguous(), None)
    h = hidden[:2].cpu()
    w = {n: v.detach().cpu() for n, v in net.state_dict().items() if n in R.NAMES}
    ref = R.latent_block(h, w, None, sample=False)["d"].transpose(1, 0).reshape(N, 400)
    f32 = R.latent_block_fp32(h, w, None, torch.zeros_like(h))["d"].transpose(1, 0).reshape(N, 400)
    lat = chunk_latents(net, x)
    assert lat.shape == (N, 400) and lat.is_contiguous()
    e, y = rel_l2(lat, ref), max(rel_l2(f32, ref), U)
    print(f"\n[vae chunk_latents] {e:.2e}/{y:.2e}")
    assert e <= 4 * y
    centers = lat[:5].clone()
    lat2, ids = chunks_to_codes(net, x, kmeans=KMeans.from_centers(centers))
    assert torch.equal(lat2, lat) and ids.dtype == torch.int64 and ids.shape == (N,)
    assert ids[:5].tolist() == [0, 1, 2, 3, 4]                        # a centre's own row is nearest to it


# ---------------------------------------------------------------------------------------------- 5. refusals
def test_data_parallel_and_fused_step_refuse_a_variational_net():
    from gesture2vec_amd.model.Autoencoder_VQVAE_model import Autoencoder_VQVAE
    from gesture2vec_amd.train_eval.train_seq2seq import (FusedClipAdam, _fused_iteration,
                                                          train_iter_Autoencoder_VQ_seq2seq_dp)
    args = make_args(rep_learning_dim=40, hidden_size=32, n_poses=12)
    net = Autoencoder_VQVAE(args, 40, 12).to(DEV)
    optim = FusedClipAdam(net, lr=5e-4)
    x = torch.randn(4, 12, 40, device=DEV)
    before = {n: v.clone() for n, v in net.state_dict().items()}
    with pytest.raises(NotImplementedError, match="variational net .* staged autograd path"):
        train_iter_Autoencoder_VQ_seq2seq_dp(args, 1, x, x, net, optim, lambda comm: None, 2)
    with pytest.raises(NotImplementedError, match="variational net"):
        _fused_iteration(args, 1, x, x, net, optim, None, 1)
    with pytest.raises(NotImplementedError, match="variational block"):
        net.engine().train_step(x, x, lr=5e-4, w_l1=5.0, w_cont=0.1, w_var=0.5)
    for n, v in net.state_dict().items():
        assert torch.equal(v, before[n]), n


# ---------------------------------------------------------------------------------------------- 6. nothing else moved
@pytest.mark.parametrize("quantizer,K", [("ema", 64), ("gssoft", 48), ("none", 0)])
def test_other_configurations_keep_their_flat_layout(quantizer, K):
    from gesture2vec_amd.engine import VQVAEEngine, latent_layout, quantizer_layout, trainable_layout
    D, H, L, T = 40, 200, 2, 20
    eng = VQVAEEngine(D, H, L, K, T, beta=0.25, dropout_prob=0.0, device=DEV, quantizer=quantizer)
    want = trainable_layout(D, H, L) + quantizer_layout(quantizer, H * L, K)
    assert eng.layout == want
    off, offsets = 0, {}
    for name, shp in want:
        n = int(np.prod(shp))
        offsets[name] = (off, n, shp)
        off += (n + 3) // 4 * 4
    assert eng.offsets == offsets and eng.n_flat == off
    n_stats = (K + K * H * L) if quantizer != "none" else 0
    assert eng.comm.numel() == off + n_stats + 4 and eng.gflat.data_ptr() == eng.comm.data_ptr()
    q = quantizer_layout(quantizer, H * L, K)
    assert eng.q_off == (offsets[q[0][0]][0] if q else off) and eng.q_end == off
    # ... and a variational engine is that layout with the six tensors appended
    vae = VQVAEEngine(D, H, L, K, T, beta=0.25, dropout_prob=0.0, device=DEV, quantizer=quantizer, latent="vae")
    assert vae.layout == want + latent_layout("vae", H * L) and vae.q_off == eng.q_off and vae.q_end == off
    assert all(vae.offsets[n] == offsets[n] for n in offsets) and vae.n_flat == off + 3 * (400 * 400 + 400)
