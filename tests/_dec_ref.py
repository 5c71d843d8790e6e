"""The decoder rollout pair (g2v_dec_rollout_fwd / _bwd) restated in plain torch with the dtype as a parameter, the seeded inputs of
its float64 tests and their error bounds (tests/test_dec_ref_host.py on the host, tests/test_gpu_dec_rollout_f64.py on the GPU).
No device, no library: the recurrence is the one of include/g2v.h (the comment above g2v_dec_weights), written out once more.

In float64 a run is the reference; in float32 it is "the fp32 oracle", whose distance from float64 is the rounding noise e32 of an
array on an input.  Errors keep the project's max norm but take the scale PER TIME STEP (step_err): a BPTT gradient grows by orders
of magnitude from the last step to the first (the x20 feedback through Dropout(0.95)), and one scale for a whole (T-1, B, .) array
hides the steps whose values are small.

  bound_t = min(MARGIN * max(e32_t, 2u), cap),  MARGIN = 8 (tests/_loss_inputs.py), u = 2^-24,
  cap = what test_dec_rollout_fwd_bwd asserts (1e-4 forward arrays and running statistics, 2e-4 gradients).

The batch variance is formed the way the header states it and every route computes it: E[c^2] - E[c]^2 of c = u - b_pre, one pass
over the batch.  In float64 that is the variance to 1e-15; in float32 it loses log2(E[c^2] / var) bits to cancellation, which belongs
to the operation as the header defines it and therefore to e32.  (With the two-pass variance in its place, the first device run of
PERSIST*1-2x4x135x64-plain had e_kernel / e32 = 19 on `a`: four rows, E[c^2] / var = 25 on the worst unit, the kernels' relative
error of var 25 times that of a two-pass sum and 1 / (2 (var + eps)) of it in `a`; csrc/dec_rollout.hip, "biased batch variance".)

ReLU is the one discontinuity (the dropout masks are inputs).  tau = 8 max|a_pre32 - a_pre64| over the rollout; an element with
|a_pre64| < tau is AMBIGUOUS.  Forward arrays are compared with plain ReLU, nothing excluded (a flip moves `a` by less than tau).
The gradient reference is the float64 backward with relu_mask = (a_pre64 > 0), and on the ambiguous elements only the device's own
a > 0 (grad_reference)."""
import functools

import torch

from oracle import g2v_oracle as O

U = 2.0 ** -24
MARGIN = 8.0
CAP_FWD, CAP_GRAD = 1e-4, 2e-4
EPS = 1e-5
PRE = "decoder.decoder."
PARAMS = ("pre_linear.0.weight", "pre_linear.0.bias", "pre_linear.1.weight", "pre_linear.1.bias",
          "gru.weight_ih_l0", "gru.weight_hh_l0", "gru.bias_ih_l0", "gru.bias_hh_l0",
          "gru.weight_ih_l1", "gru.weight_hh_l1", "gru.bias_ih_l1", "gru.bias_hh_l1", "out_layer.weight", "out_layer.bias")
FWD_ARRAYS = ("y", "xin", "u", "a", "h0", "h1", "x1", "gates0", "gates1", "bn_stats", "running_mean", "running_var")
STEP_GRADS = ("du", "dgi0", "dgh0", "dgi1", "dgh1", "dy")
GRADS = STEP_GRADS + ("dh_init", "d_bn_w", "d_bn_b", "dw_hh1", "db_hh1")


def state(D, H, seed):
    """the decoder's state dict: O.init_vqvae_state plus a BatchNorm weight / bias off their initial 1 / 0"""
    sd = O.init_vqvae_state(D, H, 2, 8, seed=seed)
    g = torch.Generator().manual_seed(seed + 100)
    sd[PRE + "pre_linear.1.weight"] = 1 + 0.1 * torch.randn(H, generator=g)
    sd[PRE + "pre_linear.1.bias"] = 0.1 * torch.randn(H, generator=g)
    return sd


def inputs(T, B, D, H, p, seed, training=True):
    """float32 / uint8 CPU inputs of one case, the recipe of test_dec_rollout_fwd_bwd keyed by one seed"""
    sd = state(D, H, seed)
    g = torch.Generator().manual_seed(seed + 1000)
    inp = {"T": T, "B": B, "D": D, "H": H, "sd": sd}
    inp["target"] = torch.randn(B, T, D, generator=g)
    inp["h_init"] = torch.randn(2, B, H, generator=g) * 0.5
    inp["keep95"] = (torch.rand(T - 1, B, D, generator=g) < 0.05).to(torch.uint8)
    inp["keep_l0"] = (torch.rand(T - 1, B, H, generator=g) < (1 - p)).to(torch.uint8) if p > 0 else None
    inp["gy"] = torch.randn(T, B, D, generator=g) / (T * B * D) * 100
    if not training:
        sd[PRE + "pre_linear.1.running_mean"] = torch.randn(H, generator=g) * 0.1
        sd[PRE + "pre_linear.1.running_var"] = torch.rand(H, generator=g) + 0.5
    return inp


def _cell(x, h, w_ih, w_hh, b_ih, b_hh, keep):
    H = h.shape[1]
    gi, gh = x @ w_ih.t() + b_ih, h @ w_hh.t() + b_hh
    keep += [gi, gh]
    r = torch.sigmoid(gi[:, :H] + gh[:, :H])
    z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    return (1 - z) * n + z * h, torch.cat([r, z, n, gh[:, 2 * H:]], dim=1)


def rollout(inp, dtype, *, n_pre=1, conditioned=True, training=True, p=0.0, relu_mask=None, grad=False):
    """Every array a device call writes, in `dtype` (dict of detached tensors; keys FWD_ARRAYS + a_pre, the BatchNorm output before
    ReLU).  relu_mask (T-1,B,H): replaces ReLU by a multiplication.  grad=True: also the gradients of sum_t <y_t, gy_t> by autograd
    in the same dtype (keys GRADS, dbn = the gradient at a_pre, "params": by state-dict name)."""
    T, B, D, H, sd = inp["T"], inp["B"], inp["D"], inp["H"], inp["sd"]
    w = {k: sd[PRE + k].to(dtype).clone().requires_grad_(grad) for k in PARAMS}
    h_init = inp["h_init"].to(dtype).clone().requires_grad_(grad)
    tgt = inp["target"].to(dtype).transpose(0, 1)
    k95 = inp["keep95"].to(dtype)
    drop = training and p > 0 and inp["keep_l0"] is not None
    kl0 = inp["keep_l0"].to(dtype) if drop else None
    rm, rv = sd[PRE + "pre_linear.1.running_mean"].to(dtype), sd[PRE + "pre_linear.1.running_var"].to(dtype)
    mask = None if relu_mask is None else relu_mask.to(dtype)
    ys, out = [tgt[0]], {k: [] for k in ("xin", "u", "a_pre", "a", "x1", "gates0", "gates1", "bn_stats")}
    h0s, h1s, taps = [h_init[0]], [h_init[1]], {"u": [], "a_pre": [], "cells": []}
    with torch.set_grad_enabled(grad):
        for k in range(T - 1):                                            # step k + 1: y_{k+1} from the input drawn at y_k
            src = tgt[k] if (k == 0 or k < n_pre) else ys[k]             # next input = target[t] if t < n_pre else y_t
            xin = k95[k] * src * 20.0 if conditioned else torch.zeros_like(src)      # Dropout(0.95), always active
            u = xin @ w["pre_linear.0.weight"].t() + w["pre_linear.0.bias"]
            if training:
                c = u - w["pre_linear.0.bias"]                            # the sums the header names (g2v_dec_saved.bn_partial):
                mc = c.mean(0)                                            # of (u - b) and (u - b)^2 over the batch (module docstring)
                mean = mc + w["pre_linear.0.bias"]                        # (exactly b_pre where every row's xin is zero)
                var = torch.clamp((c * c).mean(0) - mc * mc, min=0.0)     # biased
                a_pre = (u - mean) / torch.sqrt(var + EPS) * w["pre_linear.1.weight"] + w["pre_linear.1.bias"]
                rm = 0.9 * rm + 0.1 * mean.detach()
                rv = 0.9 * rv + 0.1 * (var.detach() * (B / max(B - 1, 1)))
                out["bn_stats"].append(torch.stack([mean, var]))
            else:
                a_pre = (u - rm) / torch.sqrt(rv + EPS) * w["pre_linear.1.weight"] + w["pre_linear.1.bias"]
            a = torch.relu(a_pre) if mask is None else a_pre * mask[k]
            cells = []
            h0, g0 = _cell(a, h0s[k], w["gru.weight_ih_l0"], w["gru.weight_hh_l0"], w["gru.bias_ih_l0"], w["gru.bias_hh_l0"], cells)
            x1 = kl0[k] * h0 / (1.0 - p) if drop else h0                  # nn.GRU's inter-layer dropout, training only
            h1, g1 = _cell(x1, h1s[k], w["gru.weight_ih_l1"], w["gru.weight_hh_l1"], w["gru.bias_ih_l1"], w["gru.bias_hh_l1"], cells)
            y = h1 @ w["out_layer.weight"].t() + w["out_layer.bias"]
            ys.append(y); h0s.append(h0); h1s.append(h1)
            taps["u"].append(u); taps["a_pre"].append(a_pre); taps["cells"].append(cells)
            for name, v in (("xin", xin), ("u", u), ("a_pre", a_pre), ("a", a), ("x1", x1), ("gates0", g0), ("gates1", g1)):
                out[name].append(v)
        res = {k: torch.stack([t.detach() for t in v]) for k, v in out.items() if v}
        res.update(y=torch.stack([t.detach() for t in ys]), h0=torch.stack([t.detach() for t in h0s]),
                   h1=torch.stack([t.detach() for t in h1s]), running_mean=rm.detach(), running_var=rv.detach())
        if not grad:
            return res
        kept = taps["u"] + taps["a_pre"] + [c for cs in taps["cells"] for c in cs] + ys[1:]
        for t in kept:
            t.retain_grad()
        gy = inp["gy"].to(dtype)
        sum((ys[t] * gy[t]).sum() for t in range(1, T)).backward()
    zg = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    res["du"] = torch.stack([zg(t) for t in taps["u"]])
    res["dbn"] = torch.stack([zg(t) for t in taps["a_pre"]])
    for j, name in enumerate(("dgi0", "dgh0", "dgi1", "dgh1")):
        res[name] = torch.stack([zg(cs[j]) for cs in taps["cells"]])
    res["dy"] = torch.stack([gy[0]] + [zg(t) for t in ys[1:]])            # the total dL/dy_t, feedback included; row 0 is not compared
    res["dh_init"] = zg(h_init)
    res["params"] = {PRE + k: zg(v) for k, v in w.items()}
    res["d_bn_w"], res["d_bn_b"] = res["params"][PRE + "pre_linear.1.weight"], res["params"][PRE + "pre_linear.1.bias"]
    res["dw_hh1"], res["db_hh1"] = res["params"][PRE + "gru.weight_hh_l1"], res["params"][PRE + "gru.bias_hh_l1"]
    return res


# ---------------------------------------------------------------------------------------------------------------- error measure
def _steps(name, t):
    """(steps, ...) view of an array: its own leading axis where that is time, one step for the rest"""
    t = torch.as_tensor(t).detach().cpu().double()
    timed = name in ("xin", "u", "a", "a_pre", "x1", "gates0", "gates1", "bn_stats", "y", "h0", "h1", "dbn") + STEP_GRADS
    return t.reshape(t.shape[0], -1) if timed else t.reshape(1, -1)


def step_err(got, ref, name="y"):
    """max|got_t - ref_t| / max|ref_t| for every time step t (tensor of float64).  A reference slice that is exactly zero has no
    scale of its own: 0 where the other slice is exactly zero too, inf where it is not."""
    g, r = _steps(name, got), _steps(name, ref)
    assert g.shape == r.shape, (name, g.shape, r.shape)
    diff, scale = (g - r).abs().amax(1), r.abs().amax(1)
    inf = torch.full_like(diff, float("inf"))
    return torch.where(scale > 0, diff / scale.clamp_min(1e-300), torch.where(g.abs().amax(1) == 0, torch.zeros_like(diff), inf))


def bound(e32, cap):
    return torch.clamp(MARGIN * torch.clamp(e32, min=2 * U), max=cap)


def cap_of(name):
    return CAP_FWD if name in FWD_ARRAYS else CAP_GRAD


def check(label, name, got, ref, e32, skip_first=False, cap=None, steps_of=None):
    """print the worst step's e_kernel, e32, their ratio and the bound; return (ok, line, ratio).  The ratio is e_kernel over
    max(e32, 2u), the quantity the margin multiplies.  skip_first: step 0 is not compared (dy: the header calls that row ignored).
    cap, steps_of: another operation's cap for `name` and the array of this file whose time axis it has (tests/_gru_ref.py)."""
    ek, bd = step_err(got, ref, steps_of or name), bound(e32, cap_of(name) if cap is None else cap)
    if skip_first:
        ek, bd, e32 = ek[1:], bd[1:], e32[1:]
    k = int(torch.argmax(ek / bd))
    ratio = float(ek[k] / max(float(e32[k]), 2 * U))
    line = (f"{label} {name}: step {k + (1 if skip_first else 0)} of {len(ek)}  e_kernel {float(ek[k]):.3e}  e32 {float(e32[k]):.3e}  "
            f"ratio {ratio:.2f}  bound {float(bd[k]):.3e}")
    print(line)
    return bool((ek <= bd).all()), line, ratio


# --------------------------------------------------------------------------------------------------------------- a case's reference
def mode_of(case):
    return dict(n_pre=case["n_pre"], conditioned=bool(case["conditioned"]), training=bool(case["training"]), p=case["p"])


def case_key(case):
    return (case["T"], case["B"], case["D"], case["H"], case["p"], case["n_pre"], int(case["conditioned"]), int(case["training"]),
            case["seed"])


@functools.lru_cache(maxsize=2)
def _reference(key):
    T, B, D, H, p, n_pre, conditioned, training, seed = key
    mode = dict(n_pre=n_pre, conditioned=bool(conditioned), training=bool(training), p=p)
    inp = inputs(T, B, D, H, p, seed, training=bool(training))
    f64, f32 = rollout(inp, torch.float64, **mode), rollout(inp, torch.float32, **mode)
    ref = {"inp": inp, "mode": mode, "f64": f64}
    ref["tau"] = 8.0 * float((f32["a_pre"].double() - f64["a_pre"]).abs().max())
    ref["ambiguous"] = f64["a_pre"].abs() < ref["tau"]
    ref["pattern"] = f64["a_pre"] > 0
    ref["pattern32_differs"] = int((((f32["a_pre"] > 0) != ref["pattern"]) & ~ref["ambiguous"]).sum())
    ref["e32"] = {k: step_err(f32[k], f64[k], k) for k in FWD_ARRAYS if k in f64 and (training or k in ("y", "u", "h0", "h1"))}
    if training:      # the gradient noise: both dtypes under the float64 ReLU pattern, so that no flip enters it
        g64 = rollout(inp, torch.float64, relu_mask=ref["pattern"], grad=True, **mode)
        g32 = rollout(inp, torch.float32, relu_mask=ref["pattern"], grad=True, **mode)
        ref["g64"] = {k: g64[k] for k in GRADS + ("dbn",)}
        ref["e32"].update({k: step_err(g32[k], g64[k], k) for k in GRADS})
    return ref


def reference(case):
    """inputs, the float64 forward (and backward under its own ReLU pattern), tau, the ambiguous elements and e32 per array and
    step of one case of DEC_F64_CASES; the last two cases stay cached"""
    return _reference(case_key(case))


def grad_reference(case, device_a):
    """The float64 gradients the device's backward is held to: relu_mask = (a_pre64 > 0), on the ambiguous elements the device's
    own a > 0.  Also returns how many non-ambiguous elements of the device's pattern differ from the float64 one (must be 0)."""
    ref = reference(case)
    dev = torch.as_tensor(device_a).detach().cpu() > 0
    differs = int(((dev != ref["pattern"]) & ~ref["ambiguous"]).sum())
    flips = ref["ambiguous"] & (dev != ref["pattern"])
    if not bool(flips.any()):
        return ref["g64"], differs
    g = rollout(ref["inp"], torch.float64, relu_mask=torch.where(ref["ambiguous"], dev, ref["pattern"]), grad=True, **ref["mode"])
    return {k: g[k] for k in GRADS + ("dbn",)}, differs
