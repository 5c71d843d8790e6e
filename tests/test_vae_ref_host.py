"""CPU only: the float64 restatement of the variational block (tests/_vae_ref.py) against the reference's own numbers (fixture a/
of tests/golden/vae.npz, recorded by make_fixtures_vae.py from the reference on the CPU), and the host surface of a variational
net: construction, state_dict keys against the reference's, strict loading of the checkpoint the reference wrote.

Bars: the reference computed in fp32, the restatement in float64 from the same fp32 inputs; an E = 64 long fp32 dot product of
O(1) terms is good to ~64 * 6e-8 of its largest term, so 1e-5 of a tensor's largest element covers it with room.  The loss is
one fp32 scalar: 2e-6 relative, the bar tests/test_gpu_plain_autoencoder.py uses."""
import argparse
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

import _vae_ref as R
from oracle import g2v_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, ROOT)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "vae.npz"))


def relmax(got, ref):
    got, ref = torch.as_tensor(got).double().reshape(-1), torch.as_tensor(ref).double().reshape(-1)
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def block_weights(fx, tag, step, E, seed):
    """the six VAE tensors the reference's step started from: the seeded initial state, or what the fixture recorded"""
    if step == 1:
        w = R.vae_state(E, seed)
        for n, v in w.items():
            assert hashlib.sha256(v.contiguous().numpy().tobytes()).hexdigest() == str(fx[f"{tag}/w0_sha256/{n}"]), n
        return w
    return {n: torch.from_numpy(fx[f"{tag}/s{step}/vae_w/{n}"].copy()) for n in R.NAMES}


@pytest.mark.parametrize("step", [1, 2])
def test_restatement_reproduces_the_reference(fx, step):
    """mean, logvar, the decoder's initial state, the KL term, the iteration's loss and the six VAE gradients of fixture a/: step 1
    ran at epoch 0 (no KL term in loss or gradients), step 2 at epoch 1 (both carry it)."""
    B, T, D, H, L, n_steps, seed, _K, epochs = [int(v) for v in fx["a/cfg"]]
    E, key = L * H, f"a/s{step}"
    epoch = int(fx[f"{key}/epoch"])
    assert epoch == step - 1
    w = block_weights(fx, "a", step, E, seed)
    g_d = torch.from_numpy(fx[f"{key}/g_fc_decoder"].copy()).reshape(B, L, H).transpose(1, 0)
    g_kl = 0.1 * epoch / epochs if epoch > 0 else 0.0
    f, g = R.latent_block_grads(fx[f"{key}/encoder_hidden"], w, fx[f"{key}/eps"], g_d, g_kl)
    assert relmax(f["mean"], fx[f"{key}/mean"]) < 1e-5
    assert relmax(f["logvar"], fx[f"{key}/logvar"]) < 1e-5
    assert relmax(f["d"], fx[f"{key}/first_hidden"]) < 1e-5
    assert abs(float(f["kl"]) - float(fx[f"{key}/kld"])) < 1e-5 * float(fx[f"{key}/kld"])
    loss = float(fx[f"{key}/custom_loss"]) + (float(f["kl"]) * 0.1 * epoch / epochs if epoch > 0 else 0.0)
    assert abs(loss - float(fx[f"{key}/loss"])) <= 2e-6 * abs(loss)
    if epoch == 0:
        assert float(fx[f"{key}/loss"]) == float(fx[f"{key}/custom_loss"]), "no KL term at epoch 0"
    else:
        assert float(fx[f"{key}/loss"]) > float(fx[f"{key}/custom_loss"])
    for n in R.NAMES:
        head = f"{key}/vae_grad"
        if f"{head}/{n}" in fx.files:
            assert relmax(g[n], fx[f"{head}/{n}"]) < 1e-5, n
        else:
            got = g[n].reshape(-1)
            ref_n = float(fx[f"{head}_norm/{n}"])
            assert abs(float(got.norm()) - ref_n) <= 1e-5 * ref_n, n
            s = fx[f"{head}_sample/{n}"].astype(np.float64)
            assert float(np.abs(got.numpy()[R.sample_index(got.numel())] - s).max()) <= 1e-5 * float(np.abs(s).max()), n


def test_fp32_yardstick_agrees_with_autograd():
    """the analytic fp32 evaluation that sets the kernels' bar (latent_block_fp32) is the same function as the float64 autograd
    restatement: at H = 200 (the layer boundary inside a 16-wide tile of the row) they agree to fp32 rounding"""
    L, B, H = 2, 5, 200
    g = torch.Generator().manual_seed(3)
    h, eps, g_d = torch.randn(L, B, H, generator=g) * 0.5, torch.randn(B, L * H, generator=g), torch.randn(L, B, H, generator=g)
    w = R.vae_state(L * H, 1)
    f64, g64 = R.latent_block_grads(h, w, eps, g_d, g_kl=0.7)
    f32 = R.latent_block_fp32(h, w, eps, g_d, g_kl=0.7)
    for n in ("mean", "logvar", "z", "d"):
        assert relmax(f32[n], f64[n]) < 1e-5, n
    for n in ("dh", "dmean", "dlogvar"):
        assert relmax(f32[n], g64[n]) < 1e-5, n
    assert abs(float(f32["kl"]) - float(f64["kl"])) < 1e-5 * float(f64["kl"])
    # sample = False: z = mean, and the gradient of logvar keeps the KL term only
    f0, g0 = R.latent_block_grads(h, w, None, g_d, g_kl=0.7)
    assert torch.equal(f0["z"], f0["mean"])
    assert relmax(g0["dlogvar"], 0.7 * 0.5 * (torch.exp(f0["logvar"]) - 1) / (B * L * H)) < 1e-12


def _args(**kw):
    d = dict(rep_learning_dim=40, hidden_size=200, n_layers=2, dropout_prob=0.0, autoencoder_vae="True", autoencoder_vq="False",
             autoencoder_vq_components=512, autoencoder_vq_commitment_cost=0.25, n_pre_poses=1, autoencoder_conditioned="True",
             autoencoder_att="False", autoencoder_fixed_weight="False", n_poses=20, epochs=10)
    d.update(kw)
    return argparse.Namespace(**d)


@pytest.mark.parametrize("name,vq", [("plain", "False"), ("vq", "True")])
def test_state_dict_keys_match_reference(fx, name, vq):
    """VAE_fc_mean / VAE_fc_std / VAE_fc_decoder under exactly the reference's names and shapes, for both autoencoder_vq settings
    (with a quantiser: the soft one the reference ships)"""
    from model.Autoencoder_VQVAE_model import Autoencoder_VQVAE
    ref = dict(zip((str(k) for k in fx[f"d/{name}/keys"]), (str(s) for s in fx[f"d/{name}/shapes"])))
    net = Autoencoder_VQVAE(_args(autoencoder_vq=vq, autoencoder_vq_quantizer="gssoft"), 40, 20)
    assert net.VAE is True and net.vq is (vq == "True")
    mine = {k: "x".join(str(s) for s in v.shape) for k, v in net.state_dict().items()}
    assert mine == ref
    for n in R.NAMES:
        assert n in mine and net.get_parameter(n).requires_grad, n


def test_reference_checkpoint_loads_strictly(golden_dir):
    from utils.train_utils import load_checkpoint_and_model
    path = os.path.join(golden_dir, "vae_ckpt.bin")
    args, net, _, lang, pose_dim = load_checkpoint_and_model(path, "cpu", "autoencoder_vq")
    assert args.autoencoder_vae == "True" and net.VAE is True and net.vq is False and not net.training and pose_dim == 40
    raw = torch.load(path, map_location="cpu", weights_only=False)
    assert set(net.state_dict()) == set(raw["gen_dict"]) and set(R.NAMES) <= set(raw["gen_dict"])
    for k, v in raw["gen_dict"].items():
        assert torch.equal(net.state_dict()[k], v), k


def test_host_side_refusals_and_helpers():
    from model.Autoencoder_VQVAE_model import Autoencoder_VQVAE
    with pytest.raises(NotImplementedError, match="autoencoder_att"):
        Autoencoder_VQVAE(_args(autoencoder_att="True"), 40, 20)
    for bad in (None, 0, "10"):          # the KL schedule's length comes with the args; without it the mode is not built
        a = _args(epochs=bad)
        if bad is None:
            del a.epochs
        with pytest.raises(NotImplementedError, match="epochs"):
            Autoencoder_VQVAE(a, 40, 20)
    net = Autoencoder_VQVAE(_args(), 40, 20)
    assert net.kl_epochs == 10 and net.kl_weight(0) == 0.0 and net.kl_weight(3) == 0.1 * 3 / 10 and net.kl_weight(3, 20) == 0.1 * 3 / 20
    mu, lv = torch.randn(3, 400), torch.randn(3, 400)
    assert torch.equal(net.reparameterize(mu, lv, train=False), mu)
    torch.manual_seed(0)
    z = net.reparameterize(mu, lv)
    torch.manual_seed(0)
    assert torch.equal(z, mu + torch.exp(lv / 2) * torch.randn_like(lv))
    plain = Autoencoder_VQVAE(_args(autoencoder_vae="False"), 40, 20)
    assert plain.VAE is False and not hasattr(plain, "VAE_fc_mean")
    with pytest.raises(RuntimeError, match="no variational block"):
        plain.set_latent_noise(torch.zeros(2, 400))
    x = torch.zeros(2, 20, 40)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(x, x)
