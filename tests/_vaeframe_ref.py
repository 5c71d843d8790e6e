"""float64 restatement of the frame-level variational autoencoder of Part a (VAE_Network + train_iter_DAE with autoencoder_vq "False",
autoencoder_vae "True"), written from the definition, in numpy: forward, backward, clip_grad_norm_(5) + Adam.  It is the yardstick of
tests/test_vaeframe_host.py and tests/test_gpu_vaeframe.py and of the bars that tests/golden/make_fixtures_vaeframe.py stores.

    xm = x keep / (1 - p);  h = tanh(xm We^T + be);  mean = h Wm^T + bm;  logvar = h Ws^T + bs;  z = mean + exp(logvar / 2) eps
    c = z Wf^T + bf;  out = c Wd^T + bd
    loss = mean((out - t)^2) + 12.5 kl,  kl = mean over the B L elements of exp(logvar) - logvar - 1 + mean^2
"""
from __future__ import annotations

import numpy as np

from _vqframe_ref import SAMPLE_ABOVE, batches, batches_sha256, distance, f64, pack, stored  # noqa: F401  (shared, not copied)

STATE_KEYS = ("encoder.0.weight", "encoder.0.bias", "decoder.0.weight", "decoder.0.bias", "VAE_fc_mean.weight", "VAE_fc_mean.bias",
              "VAE_fc_std.weight", "VAE_fc_std.bias", "VAE_fc_decoder.weight", "VAE_fc_decoder.bias")
TRAINABLE = STATE_KEYS            # no buffers: every tensor of the state_dict receives a gradient
KL_WEIGHT, P_DROP = 12.5, 0.5
FORWARD = ("out", "mean", "logvar", "latent")


def forward(state, xm, eps):
    h = np.tanh(xm @ state["encoder.0.weight"].T + state["encoder.0.bias"])
    mean = h @ state["VAE_fc_mean.weight"].T + state["VAE_fc_mean.bias"]
    logvar = h @ state["VAE_fc_std.weight"].T + state["VAE_fc_std.bias"]
    z = mean + np.exp(logvar / 2.0) * eps
    c = z @ state["VAE_fc_decoder.weight"].T + state["VAE_fc_decoder.bias"]
    out = c @ state["decoder.0.weight"].T + state["decoder.0.bias"]
    return dict(latent=h, mean=mean, logvar=logvar, z=z, c=c, out=out)


def losses(f, t):
    mse = ((f["out"] - t) ** 2).mean()
    kl = (np.exp(f["logvar"]) - f["logvar"] - 1.0 + f["mean"] ** 2).mean()
    return mse, kl, mse + KL_WEIGHT * kl


def step(state, x, t, keep, eps):
    """One training forward + backward on a float64 state (a dict with the reference's state_dict keys).  x, t (B, D); keep (B, D) of
    0 / 1 or None; eps (B, L).  -> dict with every forward value (latent = h, mean, logvar, z, c, out), the three scalars (mse, kl,
    loss) and grads (the ten tensors)."""
    B, D = x.shape
    L = state["encoder.0.weight"].shape[0]
    xm = x if keep is None else x * keep / (1.0 - P_DROP)
    res = forward(state, xm, eps)
    h, mean, logvar, z, c, out = (res[k] for k in ("latent", "mean", "logvar", "z", "c", "out"))
    res["mse"], res["kl"], res["loss"] = losses(res, t)
    g = 2.0 * (out - t) / (B * D)
    kap = KL_WEIGHT / (B * L)
    dc = g @ state["decoder.0.weight"]
    dz = dc @ state["VAE_fc_decoder.weight"]
    dmean = dz + 2.0 * kap * mean
    dlogvar = dz * 0.5 * np.exp(logvar / 2.0) * eps + kap * (np.exp(logvar) - 1.0)
    dh = dmean @ state["VAE_fc_mean.weight"] + dlogvar @ state["VAE_fc_std.weight"]
    dpre = dh * (1.0 - h * h)
    res["grads"] = {"decoder.0.weight": g.T @ c, "decoder.0.bias": g.sum(0), "VAE_fc_decoder.weight": dc.T @ z,
                    "VAE_fc_decoder.bias": dc.sum(0), "VAE_fc_mean.weight": dmean.T @ h, "VAE_fc_mean.bias": dmean.sum(0),
                    "VAE_fc_std.weight": dlogvar.T @ h, "VAE_fc_std.bias": dlogvar.sum(0), "encoder.0.weight": dpre.T @ xm,
                    "encoder.0.bias": dpre.sum(0)}
    return res


def infer(state, x, eps):
    """the eval-mode forward (no dropout; the noise is still added: eps = 0 is the deterministic path) -> forward()'s dict"""
    return forward(state, x, eps)


class ClipAdam:
    """torch.nn.utils.clip_grad_norm_(params, 5) followed by torch.optim.Adam(lr, betas=(0.5, 0.999)) over every tensor of `grads`.
    (_vqframe_ref.ClipAdam walks that model's six trainable keys by name, so it does not serve a second model.)"""

    def __init__(self, lr, betas=(0.5, 0.999), eps=1e-8, max_norm=5.0):
        self.lr, self.betas, self.eps, self.max_norm, self.t = lr, betas, eps, max_norm, 0
        self.m, self.v = {}, {}

    def apply(self, state, grads):
        norm = np.sqrt(sum((g ** 2).sum() for g in grads.values()))
        coef = min(1.0, self.max_norm / (norm + 1e-6))
        self.t += 1
        b1, b2 = self.betas
        new = dict(state)
        for k, g in grads.items():
            g = g * coef
            self.m[k] = b1 * self.m.get(k, 0.0) + (1 - b1) * g
            self.v[k] = b2 * self.v.get(k, 0.0) + (1 - b2) * g * g
            denom = np.sqrt(self.v[k]) / np.sqrt(1 - b2 ** self.t) + self.eps
            new[k] = state[k] - self.lr / (1 - b1 ** self.t) * self.m[k] / denom
        return new


def iterate(state, data, lr):
    """train_iter_DAE over [(x, t, keep, eps)] from `state` -> ([result per step], final state)"""
    state, opt, results = f64(state), ClipAdam(lr), []
    for x, t, keep, eps in data:
        res = step(state, np.asarray(x, np.float64), np.asarray(t, np.float64), None if keep is None else np.asarray(keep, np.float64),
                   np.asarray(eps, np.float64))
        state = opt.apply(state, res["grads"])
        results.append(res)
    return results, state


def load_case(fx, tag):
    """-> dict(shape, lr, state0 {key: float32 array}, data [(noisy, original)], masks [uint8 (B, D)], eps [float32 (B, L)], steps)"""
    B, D, L = (int(v) for v in fx[f"{tag}/shape"])
    steps = sum(1 for k in fx.files if k.startswith(f"{tag}/s") and k.endswith("/mask"))
    data = batches(int(fx[f"{tag}/seed"]), B, D, steps)
    assert batches_sha256(data) == str(fx[f"{tag}/x_sha256"]), "the seeded inputs are not the recorded ones"
    masks = [np.unpackbits(fx[f"{tag}/s{i}/mask"])[:B * D].reshape(B, D) for i in range(1, steps + 1)]
    eps = [fx[f"{tag}/s{i}/eps"] for i in range(1, steps + 1)]
    state0 = {k[len(tag) + 4:]: fx[k] for k in fx.files if k.startswith(f"{tag}/w0/")}
    return dict(shape=(B, D, L), lr=float(fx[f"{tag}/lr"]), state0=state0, data=data, masks=masks, eps=eps, steps=steps)


def restate_case(case):
    """the float64 iterations of a loaded case -> ([result per step], final state)"""
    return iterate(case["state0"], [(n.squeeze(2).numpy(), o.squeeze(2).numpy(), m, e)
                                    for (n, o), m, e in zip(case["data"], case["masks"], case["eps"])], case["lr"])


def random_state(D, L, seed):
    """a float32 state with weights of the layers' usual scale (tests that need no reference initialisation)"""
    rng = np.random.default_rng(seed)
    f = lambda a: np.asarray(a, np.float32)      # noqa: E731
    s = {"encoder.0.weight": f(rng.standard_normal((L, D)) / np.sqrt(D)), "encoder.0.bias": f(0.1 * rng.standard_normal(L)),
         "decoder.0.weight": f(rng.standard_normal((D, L)) / np.sqrt(L)), "decoder.0.bias": f(0.1 * rng.standard_normal(D))}
    for name in ("VAE_fc_mean", "VAE_fc_std", "VAE_fc_decoder"):
        s[name + ".weight"] = f(rng.standard_normal((L, L)) / np.sqrt(L))
        s[name + ".bias"] = f(0.1 * rng.standard_normal(L))
    return {k: s[k] for k in STATE_KEYS}


def random_problem(shape, seed):
    """(state, x, t, keep, eps) float32 / uint8 for a (B, D, L) training step"""
    B, D, L = shape
    rng = np.random.default_rng(100 + seed)
    x, t = rng.standard_normal((B, D)).astype(np.float32), rng.standard_normal((B, D)).astype(np.float32)
    keep = (rng.random((B, D)) < 0.5).astype(np.uint8)
    return random_state(D, L, seed), x, t, keep, rng.standard_normal((B, L)).astype(np.float32)
