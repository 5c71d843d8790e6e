"""Float64 restatement of the chunk autoencoder's variational block (autoencoder_vae == "True") in plain torch on the CPU,
written from the formulae; autograd supplies every gradient, the noise is explicit.

    hf     = h.transpose(1, 0).reshape(B, E)          h (L,B,H), E = L H: row b = [h[0, b] ; h[1, b] ; ...]
    mean   = hf W_mean^T + b_mean,   logvar = hf W_std^T + b_std
    z      = mean + exp(logvar / 2) eps               (sample=False: z = mean)
    d      = (z W_dec^T + b_dec).reshape(B, L, H).transpose(1, 0)
    kl     = 0.5 mean(exp(logvar) - logvar - 1 + mean^2)           over all B E elements

Parameters are named as the model's state_dict names them (VAE_fc_mean / VAE_fc_std / VAE_fc_decoder . weight / bias)."""
import math

import numpy as np
import torch

NAMES = ("VAE_fc_mean.weight", "VAE_fc_mean.bias", "VAE_fc_std.weight", "VAE_fc_std.bias", "VAE_fc_decoder.weight",
         "VAE_fc_decoder.bias")


def sample_index(numel: int) -> np.ndarray:
    """the strided sample of a flattened tensor that fixture and tests agree on (tests/_h200.py)"""
    stride = max(1, numel // 512)
    return np.arange(0, numel, stride)[:512]


def vae_state(E: int, seed: int) -> dict:
    """the six tensors of the block, fp32, U(-1/sqrt(E), 1/sqrt(E)) like nn.Linear's default -- from a seeded generator, so that
    the fixture script and the tests build the same bits without storing them"""
    g = torch.Generator().manual_seed(7700 + seed)
    k = 1.0 / math.sqrt(E)
    return {n: (torch.rand((E, E) if n.endswith("weight") else (E,), generator=g) * 2 - 1) * k for n in NAMES}


def _leaf(t, grad):
    t = torch.as_tensor(t).detach().clone().double()
    return t.requires_grad_(True) if grad else t


def latent_block(h, w, eps=None, sample=True, grad=False):
    """-> dict of float64 tensors hf, mean, logvar, z, d (L,B,H), kl (scalar), plus the leaves (h, w) when grad"""
    h = _leaf(h, grad)
    w = {n: _leaf(w[n], grad) for n in NAMES}
    L, B, H = h.shape
    hf = h.transpose(1, 0).reshape(B, L * H)
    mean = hf @ w["VAE_fc_mean.weight"].t() + w["VAE_fc_mean.bias"]
    logvar = hf @ w["VAE_fc_std.weight"].t() + w["VAE_fc_std.bias"]
    z = mean + torch.exp(logvar / 2) * torch.as_tensor(eps).double() if sample else mean
    d = (z @ w["VAE_fc_decoder.weight"].t() + w["VAE_fc_decoder.bias"]).reshape(B, L, H).transpose(1, 0)
    kl = 0.5 * torch.mean(torch.exp(logvar) - logvar - 1 + mean ** 2)
    return {"h": h, "w": w, "hf": hf, "mean": mean, "logvar": logvar, "z": z, "d": d, "kl": kl}


def latent_block_grads(h, w, eps, g_d, g_kl=0.0, g_mean=None, g_logvar=None):
    """Gradients of  sum(d g_d) + g_kl kl [+ sum(mean g_mean) + sum(logvar g_logvar)]  by autograd, float64.  g_d (L,B,H).
    -> (forward dict, grads dict: dh, dmean, dlogvar, and the six parameter names)"""
    f = latent_block(h, w, eps, sample=eps is not None, grad=True)
    obj = (f["d"] * torch.as_tensor(g_d).double()).sum() + float(g_kl) * f["kl"]
    if g_mean is not None:
        obj = obj + (f["mean"] * torch.as_tensor(g_mean).double()).sum()
    if g_logvar is not None:
        obj = obj + (f["logvar"] * torch.as_tensor(g_logvar).double()).sum()
    f["mean"].retain_grad()
    f["logvar"].retain_grad()
    obj.backward()
    grads = {"dh": f["h"].grad, "dmean": f["mean"].grad, "dlogvar": f["logvar"].grad}
    grads.update({n: f["w"][n].grad for n in NAMES})
    return {k: (v.detach() if torch.is_tensor(v) else v) for k, v in f.items() if k != "w"}, grads


def latent_block_fp32(h, w, eps, g_d, g_kl=0.0):
    """The same formulas evaluated in plain fp32 on the CPU (forward and the block's analytic backward): the yardstick whose own
    error against float64 sets the kernels' bar.  -> dict mean, logvar, z, d, kl, dh, dmean, dlogvar (fp32 tensors)"""
    h = torch.as_tensor(h).float()
    w = {n: torch.as_tensor(w[n]).float() for n in NAMES}
    g_d = torch.as_tensor(g_d).float()
    L, B, H = h.shape
    E = L * H
    hf = h.transpose(1, 0).reshape(B, E)
    mean = hf @ w["VAE_fc_mean.weight"].t() + w["VAE_fc_mean.bias"]
    logvar = hf @ w["VAE_fc_std.weight"].t() + w["VAE_fc_std.bias"]
    sample = eps is not None
    e = torch.as_tensor(eps).float() if sample else torch.zeros_like(mean)
    z = mean + torch.exp(logvar / 2) * e if sample else mean
    d = (z @ w["VAE_fc_decoder.weight"].t() + w["VAE_fc_decoder.bias"]).reshape(B, L, H).transpose(1, 0).contiguous()
    kl = 0.5 * torch.mean(torch.exp(logvar) - logvar - 1 + mean ** 2)
    dz = g_d.transpose(1, 0).reshape(B, E) @ w["VAE_fc_decoder.weight"]
    c = float(g_kl) / (B * E)
    dmean = dz + c * mean
    dlogvar = dz * 0.5 * torch.exp(logvar / 2) * e + c * 0.5 * (torch.exp(logvar) - 1)
    dh = (dmean @ w["VAE_fc_mean.weight"] + dlogvar @ w["VAE_fc_std.weight"]).reshape(B, L, H).transpose(1, 0).contiguous()
    return {"mean": mean, "logvar": logvar, "z": z, "d": d, "kl": kl, "dh": dh, "dmean": dmean, "dlogvar": dlogvar}
