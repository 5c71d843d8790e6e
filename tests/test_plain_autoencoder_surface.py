"""CPU-only tests of the quantiser-free chunk autoencoder's host surface (autoencoder_vq == "False": the reference's
config/seq2seq.yml): construction and state_dict keys against the reference's, strict loading of a checkpoint the reference wrote,
the refusals that stay.  No kernel is launched."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, ROOT)


def _args(**kw):
    d = dict(rep_learning_dim=40, hidden_size=200, n_layers=2, dropout_prob=0.0, autoencoder_vae="False",
             autoencoder_vq="False", autoencoder_vq_components=512, autoencoder_vq_commitment_cost=0.25, n_pre_poses=1,
             autoencoder_conditioned="True", autoencoder_att="False", autoencoder_fixed_weight="False", n_poses=20)
    d.update(kw)
    return argparse.Namespace(**d)


def test_state_dict_keys_match_reference(golden_dir):
    """no vq_layer; keys and shapes = the reference module's at config/seq2seq.yml's dimensions (recorded by make_fixtures_plain_ae.py)"""
    from model.Autoencoder_VQVAE_model import Autoencoder_VQVAE
    fx = np.load(os.path.join(golden_dir, "plain_ae.npz"))
    ref = dict(zip((str(k) for k in fx["c/keys"]), (str(s) for s in fx["c/shapes"])))
    net = Autoencoder_VQVAE(_args(), 40, 20)
    assert net.vq is False and not hasattr(net, "vq_layer")
    mine = {k: "x".join(str(s) for s in v.shape) for k, v in net.state_dict().items()}
    assert mine == ref


def test_reference_checkpoint_loads_strictly(golden_dir):
    """tests/golden/plain_ae_ckpt.bin was written by the reference's save path from a model with autoencoder_vq "False": it loads
    with strict=True into a model without a quantiser, and none is guessed"""
    from utils.train_utils import load_checkpoint_and_model
    path = os.path.join(golden_dir, "plain_ae_ckpt.bin")
    args, net, _, lang, pose_dim = load_checkpoint_and_model(path, "cpu", "autoencoder_vq")
    assert net.vq is False and not hasattr(net, "vq_layer") and not net.training
    assert getattr(args, "autoencoder_vq_quantizer", None) is None and pose_dim == 40 and lang.n_words == 13
    raw = torch.load(path, map_location="cpu", weights_only=False)
    assert not any(k.startswith("vq_layer.") for k in raw["gen_dict"])
    assert set(net.state_dict()) == set(raw["gen_dict"])
    for k, v in raw["gen_dict"].items():
        assert torch.equal(net.state_dict()[k], v), k


@pytest.mark.parametrize("vq", ["True", "False"])
def test_vae_is_still_refused(vq):
    from model.Autoencoder_VQVAE_model import Autoencoder_VQVAE
    with pytest.raises(NotImplementedError):
        Autoencoder_VQVAE(_args(autoencoder_vae="True", autoencoder_vq=vq), 40, 20)


def test_reference_seq2seq_yml_builds_and_its_cpu_forward_fails_loudly(golden_dir):
    from config.parse_args import parse_args
    from model.Autoencoder_VQVAE_model import Autoencoder_VQVAE
    a = parse_args(["-c", os.path.join(golden_dir, "reference_config", "seq2seq.yml")])
    assert a.autoencoder_vq == "False"
    net = Autoencoder_VQVAE(a, a.rep_learning_dim, a.n_poses)
    assert net.vq is False and net.hidden_size == 200 and net.dropout_prob == 0.0
    x = torch.zeros(2, a.n_poses, a.rep_learning_dim)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(x, x)


def test_chunks_to_codes_refuses_a_net_without_quantiser():
    from gesture2vec_amd.pipeline import chunks_to_codes
    from model.Autoencoder_VQVAE_model import Autoencoder_VQVAE
    net = Autoencoder_VQVAE(_args(), 40, 20)
    with pytest.raises(ValueError, match="no quantiser"):
        chunks_to_codes(net, torch.zeros(2, 20, 40))
