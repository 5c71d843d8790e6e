"""float64 restatement of the frame-level quantised autoencoder of Part a (VQ_Frame + its VQ_Payam_EMA + train_iter_DAE), written
from the definition, in numpy: forward, backward, the EMA update of the quantiser, clip_grad_norm_(5) + Adam.  It is the yardstick of
tests/test_vqframe_host.py and tests/test_gpu_vqframe.py and of the bars that tests/golden/make_fixtures_vqframe.py stores.

    y = (x keep / (1 - p)) We^T + be;  z = gamma (y - mean) / sqrt(var + 1e-5) + beta   (batch statistics, biased variance)
    id = argmin_k |z|^2 + |e_k|^2 - 2 z.e_k (lowest k on ties);  q = e_id (the OLD codebook);  out = q Wd^T + bd
    loss = mean((out - t)^2) + 0.25 mean((q - z)^2);  q is a constant of the backward, d out / d z = d out / d q (straight-through)
    EMA (training): cs = 0.99 cs + 0.01 counts; n = sum cs; cs = (cs + 1e-5) / (n + K 1e-5) n; ema_w = 0.99 ema_w + 0.01 onehot^T z;
    codebook = ema_w / cs[:, None]
"""
from __future__ import annotations

import hashlib

import numpy as np

TRAINABLE = ("encoder.0.weight", "encoder.0.bias", "bachnorm.weight", "bachnorm.bias", "decoder.0.weight", "decoder.0.bias")
STATE_KEYS = ("encoder.0.weight", "encoder.0.bias", "bachnorm.weight", "bachnorm.bias", "bachnorm.running_mean",
              "bachnorm.running_var", "bachnorm.num_batches_tracked", "vq_layer._ema_w", "vq_layer._ema_cluster_size",
              "vq_layer.pre_linear.weight", "vq_layer.pre_linear.bias", "vq_layer._embedding.weight", "decoder.0.weight",
              "decoder.0.bias")
BN_EPS, MOMENTUM, DECAY, VQ_EPS, COMMITMENT, P_DROP = 1e-5, 0.1, 0.99, 1e-5, 0.25, 0.5
SAMPLE_ABOVE = 1024


def f64(state):
    return {k: np.asarray(v, dtype=np.float64).copy() for k, v in state.items()}


def distances(z, E):
    return (z ** 2).sum(1, keepdims=True) + (E ** 2).sum(1)[None, :] - 2.0 * z @ E.T


def margins(z, E):
    """-> (ids, margin, bound): per row the gap between the nearest and the second-nearest code, and the gap below which an fp32
    evaluation of the distance expression may decide differently: 1e-5 (|z| + max(|e1|, |e2|))^2"""
    d = distances(z, E)
    ids = d.argmin(1)
    if E.shape[0] == 1:
        return ids, np.full(z.shape[0], np.inf), np.zeros(z.shape[0])
    part = np.argpartition(d, 1, axis=1)[:, :2]
    two = np.take_along_axis(d, part, 1)
    order = np.argsort(two, 1)
    part, two = np.take_along_axis(part, order, 1), np.take_along_axis(two, order, 1)
    en = np.sqrt((E ** 2).sum(1))
    zn = np.sqrt((z ** 2).sum(1))
    bound = 1e-5 * (zn + np.maximum(en[part[:, 0]], en[part[:, 1]])) ** 2
    return ids, two[:, 1] - two[:, 0], bound


def encode(state, x):
    """eval-mode z of (N, D) rows: the running statistics, no dropout"""
    y = x @ state["encoder.0.weight"].T + state["encoder.0.bias"]
    return ((y - state["bachnorm.running_mean"]) / np.sqrt(state["bachnorm.running_var"] + BN_EPS) * state["bachnorm.weight"]
            + state["bachnorm.bias"])


def infer(state, x):
    """-> dict(ids, latent, out, margin, bound) of the eval-mode forward"""
    z = encode(state, x)
    E = state["vq_layer._embedding.weight"]
    ids, margin, bound = margins(z, E)
    out = E[ids] @ state["decoder.0.weight"].T + state["decoder.0.bias"]
    return dict(ids=ids, latent=z, out=out, margin=margin, bound=bound)


def step(state, x, t, keep, skip_vq=False):
    """One training forward + backward on a float64 state (a dict with the reference's state_dict keys).  x, t (B, D); keep (B, D) of
    0 / 1 or None.  -> (result, new_state): result has rec, loss_vq, perplexity, ids, margin, bound, latent, out and grads (the six
    trainable tensors); new_state has the running statistics and the quantiser's state moved, the trainable tensors untouched."""
    B, D = x.shape
    We, be = state["encoder.0.weight"], state["encoder.0.bias"]
    ga, bt = state["bachnorm.weight"], state["bachnorm.bias"]
    Wd, bd = state["decoder.0.weight"], state["decoder.0.bias"]
    E = state["vq_layer._embedding.weight"]
    K, L = E.shape
    xm = x if keep is None else x * keep / (1.0 - P_DROP)
    y = xm @ We.T + be
    mean, var = y.mean(0), y.var(0)
    istd = 1.0 / np.sqrt(var + BN_EPS)
    xh = (y - mean) * istd
    z = xh * ga + bt
    new = dict(state)
    new["bachnorm.running_mean"] = (1 - MOMENTUM) * state["bachnorm.running_mean"] + MOMENTUM * mean
    new["bachnorm.running_var"] = (1 - MOMENTUM) * state["bachnorm.running_var"] + MOMENTUM * var * B / (B - 1)
    new["bachnorm.num_batches_tracked"] = state["bachnorm.num_batches_tracked"] + 1
    res = dict(latent=z)
    if skip_vq:
        q, res["loss_vq"], res["perplexity"] = z, 0.0, 0.0
    else:
        ids, res["margin"], res["bound"] = margins(z, E)
        q = E[ids]
        onehot = np.zeros((B, K))
        onehot[np.arange(B), ids] = 1.0
        counts = onehot.sum(0)
        cs = state["vq_layer._ema_cluster_size"] * DECAY + (1 - DECAY) * counts
        n = cs.sum()
        cs = (cs + VQ_EPS) / (n + K * VQ_EPS) * n
        ema_w = state["vq_layer._ema_w"] * DECAY + (1 - DECAY) * (onehot.T @ z)
        new["vq_layer._ema_cluster_size"], new["vq_layer._ema_w"] = cs, ema_w
        new["vq_layer._embedding.weight"] = ema_w / cs[:, None]
        pr = counts / B
        res.update(ids=ids, loss_vq=COMMITMENT * ((q - z) ** 2).mean(), perplexity=float(np.exp(-(pr * np.log(pr + 1e-10)).sum())))
    out = q @ Wd.T + bd
    res["out"], res["rec"] = out, ((out - t) ** 2).mean()
    g = 2.0 * (out - t) / (B * D)
    dz = g @ Wd
    if not skip_vq:
        dz = dz + 2.0 * COMMITMENT * (z - q) / (B * L)
    dy = ga * istd * (dz - dz.mean(0) - xh * (dz * xh).mean(0))
    # d loss / d be = sum_b dy = gamma istd (sum dz - B mean(dz) - mean(dz xh) sum xh) is exactly zero.  What an fp32 evaluation leaves:
    #   * the sums and the per-term roundings of dy = gamma istd (dz - mean(dz) - xh mean(dz xh)): (B - 1) eps of sum |terms| for a sum
    #     of B numbers in any order plus ~4 eps per term -> (B + 3) eps sum_b (|dz| + |mean(dz)| + |xh| |mean(dz xh)|);
    #   * sum_b xh is not zero in fp32: xh = istd (y - mean) with the mean of B numbers off by up to (B - 1) eps mean|y| and each
    #     difference rounded at eps (|y| + |mean|) -> |sum xh| <= istd (B + 3) eps sum_b (|y| + |mean|), which mean(dz xh) multiplies.
    #     This is the term that matters where a column's batch variance is small (B = 2, two close rows).
    eps32 = 2.0 ** -24
    m2 = np.abs((dz * xh).mean(0))
    res["dbe_bound"] = (B + 3) * eps32 * np.abs(ga) * istd * ((np.abs(dz) + np.abs(dz.mean(0)) + np.abs(xh) * m2).sum(0)
                                                              + m2 * istd * (np.abs(y) + np.abs(mean)).sum(0))
    res["grads"] = {"decoder.0.weight": g.T @ q, "decoder.0.bias": g.sum(0), "bachnorm.bias": dz.sum(0),
                    "bachnorm.weight": (dz * xh).sum(0), "encoder.0.weight": dy.T @ xm, "encoder.0.bias": dy.sum(0)}
    return res, new


class ClipAdam:
    """torch.nn.utils.clip_grad_norm_(params, 5) followed by torch.optim.Adam(lr, betas=(0.5, 0.999)) on the six trainable tensors"""

    def __init__(self, lr, betas=(0.5, 0.999), eps=1e-8, max_norm=5.0):
        self.lr, self.betas, self.eps, self.max_norm, self.t = lr, betas, eps, max_norm, 0
        self.m, self.v = {}, {}

    def apply(self, state, grads):
        norm = np.sqrt(sum((g ** 2).sum() for g in grads.values()))
        coef = min(1.0, self.max_norm / (norm + 1e-6))
        self.t += 1
        b1, b2 = self.betas
        new = dict(state)
        for k in TRAINABLE:
            g = grads[k] * coef
            self.m[k] = b1 * self.m.get(k, 0.0) + (1 - b1) * g
            self.v[k] = b2 * self.v.get(k, 0.0) + (1 - b2) * g * g
            denom = np.sqrt(self.v[k]) / np.sqrt(1 - b2 ** self.t) + self.eps
            new[k] = state[k] - self.lr / (1 - b1 ** self.t) * self.m[k] / denom
        return new


def iterate(state, batches, lr):
    """train_iter_DAE over [(x, t, keep)] from `state` -> ([result per step], final state)"""
    state, opt, results = f64(state), ClipAdam(lr), []
    for x, t, keep in batches:
        res, state = step(state, np.asarray(x, np.float64), np.asarray(t, np.float64), None if keep is None else np.asarray(keep, np.float64))
        state = opt.apply(state, res["grads"])
        results.append(res)
    return results, state


def batches(seed, B, D, steps):
    """The fixtures' inputs, from the seed: [(noisy, original)] torch tensors (B, D, 1); original N(0, 1), noisy = original + 0.1 N(0, 1)"""
    import torch
    g = torch.Generator().manual_seed(1000 + seed)
    out = []
    for _ in range(steps):
        original = torch.randn(B, D, 1, generator=g)
        out.append((original + 0.1 * torch.randn(B, D, 1, generator=g), original))
    return out


def batches_sha256(data):
    return hashlib.sha256(b"".join(t.numpy().tobytes() for pair in data for t in pair)).hexdigest()


def load_case(fx, tag):
    """-> dict(shape, lr, state0 {key: float32 array}, data [(noisy, original)], masks [uint8 (B, D)], steps) of a recorded case"""
    B, D, L, K = (int(v) for v in fx[f"{tag}/shape"])
    steps = sum(1 for k in fx.files if k.startswith(f"{tag}/s") and k.endswith("/mask"))
    data = batches(int(fx[f"{tag}/seed"]), B, D, steps)
    assert batches_sha256(data) == str(fx[f"{tag}/x_sha256"]), "the seeded inputs are not the recorded ones"
    masks = [np.unpackbits(fx[f"{tag}/s{i}/mask"])[:B * D].reshape(B, D) for i in range(1, steps + 1)]
    state0 = {k[len(tag) + 4:]: fx[k] for k in fx.files if k.startswith(f"{tag}/w0/")}
    return dict(shape=(B, D, L, K), lr=float(fx[f"{tag}/lr"]), state0=state0, data=data, masks=masks, steps=steps)


def restate_case(case):
    """the float64 iterations of a loaded case -> ([result per step], final state)"""
    return iterate(case["state0"], [(n.squeeze(2).numpy(), o.squeeze(2).numpy(), m) for (n, o), m in zip(case["data"], case["masks"])],
                   case["lr"])


def warm_quantiser(state, B, seed):
    """The warm state of the fixtures: codebook N(0, 1), _ema_cluster_size = B / K, _ema_w = codebook B / K"""
    K, L = state["vq_layer._embedding.weight"].shape
    E = np.random.default_rng(seed).standard_normal((K, L)).astype(np.float32)
    state = dict(state)
    state["vq_layer._embedding.weight"] = E
    state["vq_layer._ema_cluster_size"] = np.full((K,), B / K, dtype=np.float32)
    state["vq_layer._ema_w"] = (E * np.float32(B / K)).astype(np.float32)
    return state


# ---- how a quantity is stored and compared: whole up to SAMPLE_ABOVE elements, else its float64 L2 norm and a strided sample
def pack(a):
    a = np.asarray(a)
    if a.size <= SAMPLE_ABOVE:
        return {"": a}
    flat = a.reshape(-1)
    return {"_norm": np.float64(np.sqrt((flat.astype(np.float64) ** 2).sum())), "_sample": flat[::-(-a.size // SAMPLE_ABOVE)].copy()}


def distance(got, ref):
    """relative distance of two packed quantities: the largest of max |got - ref| / max |ref| over the parts"""
    worst = 0.0
    for part, r in ref.items():
        g = np.asarray(got[part], np.float64).reshape(-1)
        r = np.asarray(r, np.float64).reshape(-1)
        worst = max(worst, float(np.abs(g - r).max()) / max(float(np.abs(r).max()), 1e-30))
    return worst


def stored(fx, name):
    """the packed quantity `name` of a loaded fixture"""
    return {part: fx[name + part] for part in ("", "_norm", "_sample") if (name + part) in fx.files}
