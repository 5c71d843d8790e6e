"""CPU-only checks of Part d on continuous latents (text2_embedding_discrete: False): the model's state_dict is the reference's,
the synthetic config parses, and the float64 restatement the GPU tests lean on reproduces the reference's recorded losses."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _t2e_latent_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("t2e_latent_noatt", "False"), ("t2e_latent_att", "True")]


@pytest.mark.parametrize("name,att", CASES)
def test_model_builds_with_the_reference_state_dict(golden_dir, name, att):
    from gesture2vec_amd.model.text2embedding_model import text2embedding_model
    fx = R.load_golden(golden_dir, name)
    B, Tw, S, H, L, E, NW, EMB = [int(v) for v in fx["cfg"]]
    args = argparse.Namespace(hidden_size=H, n_layers=L, dropout_prob=0.2, autoencoder_vq_components=64, autoencoder_att=att,
                              n_pre_poses=1, n_poses=20, sentence_frame_length=120, text2_embedding_discrete="False")
    net = text2embedding_model(args, 135, 20, NW, EMB, np.zeros((NW, EMB), dtype=np.float32), None)
    ref = {k[3:]: tuple(fx[k].shape) for k in fx if k.startswith("w0/")}
    got = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert got == ref
    assert net.pose_dim == E == L * H
    assert "decoder.decoder.embedding.weight" not in got
    assert got["decoder.decoder.pre_linear.0.weight"] == (H, E + (H if att == "True" else 0))
    assert got["decoder.decoder.out.weight"] == (E, H) and got["decoder.decoder.out.bias"] == (E,)
    dec = net.decoder.decoder
    assert not hasattr(dec, "embedding") and not hasattr(dec, "dropout")
    net.load_state_dict({k[3:]: torch.from_numpy(fx[k].copy()) for k in fx if k.startswith("wN/")}, strict=True)


def test_the_discrete_model_keeps_its_state_dict():
    from gesture2vec_amd.model.text2embedding_model import text2embedding_model
    args = argparse.Namespace(hidden_size=32, n_layers=2, dropout_prob=0.2, autoencoder_vq_components=64, autoencoder_att="False",
                              n_pre_poses=1, n_poses=20, sentence_frame_length=120, text2_embedding_discrete="True")
    sd = text2embedding_model(args, 135, 20, 50, 30, np.zeros((50, 30), dtype=np.float32), None).state_dict()
    assert tuple(sd["decoder.decoder.embedding.weight"].shape) == (64, 32)
    assert tuple(sd["decoder.decoder.pre_linear.0.weight"].shape) == (32, 32) and tuple(sd["decoder.decoder.out.weight"].shape) == (64, 32)


def test_latent_synthetic_config_parses():
    from config.parse_args import parse_args
    a = parse_args(["--config", os.path.join(ROOT, "config", "seq2seq_latent_synthetic.yml"), "--synthetic"])
    b = parse_args(["--config", os.path.join(ROOT, "config", "seq2seq_synthetic.yml"), "--synthetic"])
    assert a.text2_embedding_discrete == "False" and b.text2_embedding_discrete == "True"
    diff = {k for k in vars(b) if getattr(a, k, None) != getattr(b, k)}
    assert diff == {"config", "name", "model_save_path", "text2_embedding_discrete"}, diff


@pytest.mark.parametrize("name,att", CASES)
def test_restatement_reproduces_the_golden_losses(golden_dir, name, att):
    fx = R.load_golden(golden_dir, name)
    p = float(fx["cfg_f"][0])
    tgt = torch.from_numpy(fx["latents"]).transpose(0, 1).double()
    for step, w in ((1, "w0/"), (2, "w1/")):
        P = R.decoder_params({k[3:]: fx[k] for k in fx if k.startswith(w)}, requires_grad=False)
        enc = torch.from_numpy(fx[f"s{step}/enc_out"]).double() if att == "True" else None
        outs, stats = R.rollout(P, torch.from_numpy(fx[f"s{step}/hidden0"]).double(), tgt, 1, p,
                                torch.from_numpy(fx[f"s{step}/mask_dec_l0"]), enc)
        ref = float(fx[f"s{step}/loss"])
        assert abs(float(R.mse(outs, tgt)) - ref) <= 1e-6 * ref, (step, float(R.mse(outs, tgt)), ref)
        assert float((outs.transpose(0, 1) - torch.from_numpy(fx[f"s{step}/outputs"]).double()).abs().max()) < 1e-5
        assert len(stats) == tgt.shape[0] - 1


def test_restatement_feedback_gradient_is_attached():
    """the term a port of the discrete backward would drop: detaching the fed-back inputs changes d loss / d pre_linear.0.weight"""
    fx = R.load_golden(os.path.join(ROOT, "tests", "golden"), "t2e_latent_noatt")
    tgt = torch.from_numpy(fx["latents"]).transpose(0, 1).double()
    grads = []
    for detach in (False, True):
        P = R.decoder_params({k[3:]: fx[k] for k in fx if k.startswith("w0/")})
        outs, _ = R.rollout(P, torch.from_numpy(fx["s1/hidden0"]).double(), tgt, 1, 0.0, None, None, detach_feedback=detach)
        R.mse(outs, tgt).backward()
        grads.append(P["pre_linear.0.weight"].grad.clone())
    assert float((grads[0] - grads[1]).abs().max()) > 0.05 * float(grads[0].abs().max())
