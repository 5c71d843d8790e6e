"""Restatement of the text -> pose baseline's decoder rollout (Seq2SeqNet) in plain torch on the CPU, written from the formulae;
autograd supplies every gradient, dropout masks are explicit, BatchNorm runs on batch statistics.  The dtype is the inputs': the
float64 run is the yardstick, the float32 run of the SAME code measures what single precision alone costs (the tests' bars).

For t = 0 .. S1-1 (h1_t = the top state in front of the step's GRU):
    x_t = target[t] while t < max(1, n_pre), else y_{t-1}                  (the OUTPUT itself: its gradient flows on)
    e_tw = v . tanh(W_a [h1_t ; enc_tw] + b_a);  w_t = softmax_tw(e) over ALL Tw positions;  c_t = sum_tw w_t[tw] enc_tw
    u_t = [x_t ; c_t] W_pre^T + b_pre;  a_t = ReLU(gamma (u_t - mean_B) / sqrt(var_B + 1e-5) + beta)
    h0, h1 = GRU cells (gate order r, z, n; inter-layer dropout: h0 * keep / (1 - p) into layer 1)
    y_t = h1 W_out^T + b_out
Parameters are named as the model's state_dict names them below `decoder.decoder.`."""
import torch

EPS = 1e-5


def decoder_params(state_dict, dtype=torch.float64, requires_grad=True):
    """{short name: leaf of `dtype`} from a state_dict (tensors or numpy arrays) of the whole model"""
    out = {}
    for k, v in state_dict.items():
        if not k.startswith("decoder.decoder.") or k.endswith("num_batches_tracked"):
            continue
        t = torch.as_tensor(v).detach().cpu().clone().to(dtype)
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


def rollout(P, hidden0, target, enc, n_pre, p_drop=0.0, keep_l0=None, training=True, detach_feedback=False):
    """P: decoder_params(); hidden0 (2,B,H); target (S1+1,B,D) step-major; enc (Tw,B,H); keep_l0 (S1,B,H) 0/1 or None.
    -> dict(y (S1,B,D), attw (S1,B,Tw), stats [(mean, biased var) per step])."""
    S1 = target.shape[0] - 1
    h0, h1 = hidden0[0], hidden0[1]
    Tw = enc.shape[0]
    ys, aws, stats = [], [], []
    x = target[0]
    for t in range(S1):
        hh = h1.unsqueeze(0).expand(Tw, -1, -1)
        energy = torch.tanh(torch.cat([hh, enc], 2) @ P["attn.attn.weight"].t() + P["attn.attn.bias"])      # (Tw,B,H)
        w = torch.softmax((energy * P["attn.v"]).sum(2), dim=0)                                                # (Tw,B)
        xin = torch.cat([x, (w.unsqueeze(2) * enc).sum(0)], 1)
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
            x1 = h0 * keep_l0[t].to(h0.dtype) / (1.0 - p_drop)
        h1 = gru_cell(x1, h1, P["gru.weight_ih_l1"], P["gru.weight_hh_l1"], P["gru.bias_ih_l1"], P["gru.bias_hh_l1"])
        y = h1 @ P["out.weight"].t() + P["out.bias"]
        ys.append(y)
        aws.append(w.t())
        if t + 1 < max(1, n_pre):
            x = target[t + 1]
        else:
            x = y.detach() if detach_feedback else y
    return dict(y=torch.stack(ys), attw=torch.stack(aws), stats=stats)


def custom_loss(outputs, target, w_l1, w_cont, w_var):
    """outputs, target (B,T,D): w_l1 mean|o - t| + w_cont sum_t |o_t - o_{t-1}| / numel - w_var sum ||o[:, :, d]||_2 (over T) / numel"""
    n = outputs.numel()
    l1 = (outputs - target).abs().mean() * w_l1
    cont = (outputs[:, 1:] - outputs[:, :-1]).abs().sum() / n * w_cont
    var = -torch.sqrt((outputs ** 2).sum(1)).sum() / n * w_var
    return l1 + cont + var


def running_stats(stats, B, momentum=0.1):
    """nn.BatchNorm1d's running statistics after the steps' updates, from zeros / ones"""
    rm, rv = torch.zeros_like(stats[0][0]), torch.ones_like(stats[0][1])
    for mean, var in stats:
        rm = (1 - momentum) * rm + momentum * mean
        rv = (1 - momentum) * rv + momentum * var * (B / (B - 1) if B > 1 else 1.0)
    return rm, rv


def kernel_case(state_dict, hidden0, target, enc, g_out, n_pre, p_drop, keep_l0, dtype=torch.float64, detach_feedback=False):
    """What the fused kernels are asked for, from the restatement in `dtype`: loss = sum(y * g_out), so that d loss / d y = g_out as
    g2v_pose_attn_rollout_bwd is handed it.  -> {name: tensor} of y, attw, the BatchNorm statistics (mean, 1 / sqrt(var + eps)),
    d_hidden0, d_enc (context AND energy paths) and every weight and bias gradient (`grad/<short name>`)."""
    P = decoder_params(state_dict, dtype)
    h0 = hidden0.detach().cpu().to(dtype).requires_grad_(True)
    en = enc.detach().cpu().to(dtype).requires_grad_(True)
    tg = target.detach().cpu().to(dtype)
    r = rollout(P, h0, tg, en, n_pre, p_drop, None if keep_l0 is None else keep_l0.detach().cpu(), detach_feedback=detach_feedback)
    (r["y"] * g_out.detach().cpu().to(dtype)).sum().backward()
    out = dict(y=r["y"].detach(), attw=r["attw"].detach(), bn_mean=torch.stack([m for m, _ in r["stats"]]),
               bn_invstd=torch.stack([1.0 / torch.sqrt(v + EPS) for _, v in r["stats"]]), d_hidden0=h0.grad, d_enc=en.grad,
               stats=r["stats"])
    for k, v in P.items():
        if v.grad is not None:
            out["grad/" + k] = v.grad
    return out
