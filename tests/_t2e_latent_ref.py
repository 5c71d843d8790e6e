"""Float64 restatement of Part d's decoder on continuous latents (text2_embedding_discrete: False) in plain torch on the CPU:
the S-1 decode steps and the MSE, written from the formulae -- autograd supplies every gradient, dropout masks are explicit,
BatchNorm runs on batch statistics in training.

    x_t = target[t-1] while t <= max(1, n_pre), else y_{t-1}            (the OUTPUT itself: its gradient flows on)
    [attention: e_s = v . tanh(W_a [h1 ; enc_s] + b_a), w = softmax_s(e), x_t = [x_t ; sum_s w_s enc_s]]
    u_t = x_t W_pre^T + b_pre;  a_t = ReLU(gamma (u_t - mean_B) / sqrt(var_B + 1e-5) + beta)
    h0, h1 = GRU cells (PyTorch gate order r, z, n; inter-layer dropout: h0 * keep / (1 - p) into layer 1)
    y_t = h1 W_out^T + b_out;  outputs[0] = target[0], outputs[t] = y_t
    loss = mean over B (S-1) E of (outputs[1:] - target[1:])^2

Parameters are named as the model's state_dict names them below `decoder.decoder.`."""
import os

import numpy as np
import torch

EPS = 1e-5


def load_golden(golden_dir, name):
    """tests/golden/<name>.npz + <name>_grads.npz + <name>_final.npz (make_fixtures_t2e_latent.py) as one {key: array}"""
    out = {}
    for suffix in ("", "_grads", "_final"):
        with np.load(os.path.join(golden_dir, name + suffix + ".npz")) as fx:
            out.update({k: fx[k] for k in fx.files})
    return out


def decoder_params(state_dict, requires_grad=True):
    """{short name: float64 leaf} from a state_dict (tensors or numpy arrays) of the whole model"""
    out = {}
    for k, v in state_dict.items():
        if not k.startswith("decoder.decoder.") or k.endswith("num_batches_tracked"):
            continue
        t = torch.as_tensor(v).detach().clone().double()
        name = k[len("decoder.decoder."):]
        if requires_grad and "running_" not in name:
            t.requires_grad_(True)
        out[name] = t
    return out


def gru_cell(x, h, w_ih, w_hh, b_ih, b_hh):
    H = h.shape[1]
    gi, gh = x @ w_ih.t() + b_ih, h @ w_hh.t() + b_hh
    r = torch.sigmoid(gi[:, :H] + gh[:, :H])
    z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    return (1 - z) * n + z * h


def rollout(P, hidden0, target, n_pre, p_drop=0.0, keep_l0=None, enc_out=None, training=True, detach_feedback=False):
    """P: decoder_params(); hidden0 (2,B,H); target (S,B,E) step-major; keep_l0 (S-1,B,H) 0/1 or None; enc_out (Tw,B,H) with
    attention.  -> (outputs (S,B,E), [(mean, biased var) per step])."""
    S = target.shape[0]
    att = "attn.v" in P
    h0, h1 = hidden0[0], hidden0[1]
    outs, stats = [target[0]], []
    x = target[0]
    for t in range(1, S):
        xin = x
        if att:
            Tw = enc_out.shape[0]
            hh = h1.unsqueeze(0).expand(Tw, -1, -1)
            energy = torch.tanh(torch.cat([hh, enc_out], 2) @ P["attn.attn.weight"].t() + P["attn.attn.bias"])      # (Tw,B,H)
            w = torch.softmax((energy * P["attn.v"]).sum(2), dim=0)                                                # (Tw,B)
            xin = torch.cat([x, (w.unsqueeze(2) * enc_out).sum(0)], 1)
        u = xin @ P["pre_linear.0.weight"].t() + P["pre_linear.0.bias"]
        if training:
            mean, var = u.mean(0), u.var(0, unbiased=False)
            stats.append((mean.detach(), var.detach()))
        else:
            mean, var = P["pre_linear.1.running_mean"], P["pre_linear.1.running_var"]
        a = torch.relu((u - mean) / torch.sqrt(var + EPS) * P["pre_linear.1.weight"] + P["pre_linear.1.bias"])
        h0 = gru_cell(a, h0, P["gru.weight_ih_l0"], P["gru.weight_hh_l0"], P["gru.bias_ih_l0"], P["gru.bias_hh_l0"])
        x1 = h0
        if training and p_drop > 0 and keep_l0 is not None:
            x1 = h0 * keep_l0[t - 1].double() / (1.0 - p_drop)
        h1 = gru_cell(x1, h1, P["gru.weight_ih_l1"], P["gru.weight_hh_l1"], P["gru.bias_ih_l1"], P["gru.bias_hh_l1"])
        y = h1 @ P["out.weight"].t() + P["out.bias"]
        outs.append(y)
        if t < max(1, n_pre):
            x = target[t]
        else:
            x = y.detach() if detach_feedback else y
    return torch.stack(outs), stats


def mse(outputs, target):
    return ((outputs[1:] - target[1:]) ** 2).mean()


def running_stats(stats, B, momentum=0.1):
    """nn.BatchNorm1d's running statistics after the steps' updates, from zeros / ones"""
    rm, rv = torch.zeros_like(stats[0][0]), torch.ones_like(stats[0][1])
    for mean, var in stats:
        rm = (1 - momentum) * rm + momentum * mean
        rv = (1 - momentum) * rv + momentum * var * (B / (B - 1) if B > 1 else 1.0)
    return rm, rv
