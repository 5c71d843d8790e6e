"""The greedy gesture-code decoder of part d (g2v_attn_code_rollout_fwd / _bwd, g2v_code_cluster_bptt; csrc/t2e_rollout.hip)
restated in plain torch with the dtype as a parameter, the seeded inputs of its float64 tests and what a case must meet before a
kernel is held to it (tests/test_code_ref_host.py on the host, tests/test_gpu_code_rollout_f64.py on the GPU).  No device, no
library: the recurrence is the one of include/g2v.h (the comment above g2v_code_dec_weights), written out once more.  The error
measure, the margin and the bound are tests/_dec_ref.py's (step_err, bound, check): max norm per time step,
bound_t = min(8 max(e32_t, 2u), cap).

The batch variance is formed the way the kernels form it, in one pass: E[c^2] - E[c]^2 of c = u - b_pre (the per-workgroup partial
sums of csrc/t2e_rollout.hip), so that the cancellation is part of e32 (tests/_dec_ref.py, lines 13-17).  bn_stats holds the mean
and 1 / sqrt(var + eps).

Two discontinuities.  ReLU is handled as in tests/_dec_ref.py: tau = 8 max|a_pre32 - a_pre64|, the gradient reference takes the
float64 pattern a_pre64 > 0 and, on the elements within tau of zero only, the device's own a > 0.  The greedy feedback must not
hide anything, so it is made a condition on the INPUTS: a case is admissible only if at every free-running step and row the gap
between the two largest float64 logits exceeds tau_arg = 8 max|logits32 - logits64|, logits32 being the float32 restatement fed
the float64 run's ids (reference()["gap_min"] > reference()["tau_arg"]; the seeds of CODE_F64_CASES are chosen for it).  The
device's ids must then equal the float64 ids exactly, every row, and everything else is compared along that one trajectory.
The argmax takes the lowest index among equal maxima by an explicit rule (argmax_lowest).  A tie case plants two codes k1 < k2 with
identical rows of w_out, b_out and emb: their logits are one and the same dot product (rollout copies column k1 into column k2),
the gap condition applies to the pair against the rest, and k1 must be fed."""
import functools

import torch

import _dec_ref as R
from _dec_ref import EPS, MARGIN, U, bound, check, step_err      # noqa: F401  (the tests take them from here)

CAP_FWD, CAP_RUNNING, CAP_GRAD = 3e-5, 1e-5, 2e-4      # what tests/test_gpu_text2embedding.py asserts of the code rollout
WEIGHTS = ("emb", "w_pre", "b_pre", "bn_w", "bn_b", "w_ih0", "w_hh0", "b_ih0", "b_hh0", "w_ih1", "w_hh1", "b_ih1", "b_hh1",
           "w_out", "b_out")
ATT_WEIGHTS = ("w_attn", "b_attn", "v_attn")
SAVED = ("ec", "u", "a", "bn_stats", "h0", "h1", "x1", "gates0", "gates1", "logits", "hp", "attw")      # + ids, compared exactly
STEP_GRADS = ("du", "dgi0", "dgh0", "dgi1", "dgh1", "da")      # per step; the cluster BPTT writes the last five
_TIMED = SAVED + STEP_GRADS + ("a_pre", "dbn")


def cap_of(name):
    return CAP_RUNNING if name.startswith("running_") else (CAP_FWD if name in SAVED else CAP_GRAD)


def steps_of(name):
    """the array of tests/_dec_ref.py whose time axis `name` has (check(..., steps_of=))"""
    return "y" if name in _TIMED else "dh_init"


def argmax_lowest(logits):
    """row argmax, the LOWEST index among equal maxima, by an explicit rule"""
    K = logits.shape[1]
    at_max = logits == logits.max(dim=1, keepdim=True).values
    return torch.where(at_max, torch.arange(K).expand_as(logits), torch.full_like(logits, K, dtype=torch.int64)).min(dim=1).values


# --------------------------------------------------------------------------------------------------------------------- inputs
def make_inputs(S1, B, H, K, Tw, att, p, seed, tie=None):
    """float32 / uint8 / int64 CPU inputs keyed by one seed.  Weights are named as the fields of g2v_code_dec_weights; BatchNorm's
    weight / bias are off 1 / 0 and its running statistics off 0 / 1.  tie = (k1, k2, gain, lift): codes k1 < k2 share one row of
    w_out (scaled by gain), of b_out (raised by lift) and of emb."""
    g = torch.Generator().manual_seed(seed)
    Hin = 2 * H if att else H
    uni = lambda *s, fan: (torch.rand(*s, generator=g) * 2 - 1) / fan ** 0.5
    w = {"emb": torch.randn(K, H, generator=g), "w_pre": uni(H, Hin, fan=Hin), "b_pre": uni(H, fan=Hin),
         "bn_w": 1 + 0.1 * torch.randn(H, generator=g), "bn_b": 0.1 * torch.randn(H, generator=g)}
    for l in (0, 1):
        w.update({f"w_ih{l}": uni(3 * H, H, fan=H), f"w_hh{l}": uni(3 * H, H, fan=H), f"b_ih{l}": uni(3 * H, fan=H),
                  f"b_hh{l}": uni(3 * H, fan=H)})
    w.update(w_out=uni(K, H, fan=H), b_out=uni(K, fan=H))
    if att:
        w.update(w_attn=uni(H, 2 * H, fan=2 * H), b_attn=uni(H, fan=2 * H), v_attn=torch.randn(H, generator=g) / H ** 0.5)
    if tie is not None:
        k1, k2, gain, lift = tie
        w["w_out"][k1] *= gain
        w["b_out"][k1] += lift
        for name in ("w_out", "b_out", "emb"):
            w[name][k2] = w[name][k1]
    inp = {"S1": S1, "B": B, "H": H, "K": K, "Tw": Tw, "att": att, "p": p, "w": w, "tie": tie}
    inp["running_mean"], inp["running_var"] = 0.1 * torch.randn(H, generator=g), 0.5 + torch.rand(H, generator=g)
    inp["codes"] = torch.randint(0, K, (S1 + 1, B), generator=g)
    inp["h_init"] = 0.5 * torch.randn(2, B, H, generator=g)
    inp["keep_emb"] = (torch.rand(S1, B, H, generator=g) < 0.5).to(torch.uint8)
    inp["keep_l0"] = (torch.rand(S1, B, H, generator=g) < (1 - p)).to(torch.uint8) if p > 0 else None
    inp["d_logits"] = torch.randn(S1, B, K, generator=g) * (10.0 / (B * K ** 0.5))      # gradients of order 1 at every B and K
    inp["enc"] = inp["enc_proj"] = None
    if att:
        inp["enc"] = torch.randn(Tw, B, H, generator=g)
        inp["enc_proj"] = (inp["enc"].double() @ w["w_attn"][:, H:].double().t()).float()      # formed in float64, rounded once
    inp["dh_top"] = (inp["d_logits"].double() @ w["w_out"].double()).float()      # the cluster BPTT's input, free of kernel error
    return inp


def inputs(case):
    return make_inputs(case["S1"], case["B"], case["H"], case["K"], case["Tw"], case["att"], case["p"], case["seed"], case["tie"])


# ------------------------------------------------------------------------------------------------------------------ the rollout
def rollout(inp, dtype, *, n_pre=1, training=True, emb_drop=True, ids=None, relu_mask=None, grad=False):
    """Every member of g2v_code_dec_saved and the running statistics, in `dtype` (dict of detached tensors; also a_pre, the
    BatchNorm output in front of ReLU, and free, the (S1,) flags of the steps whose fed code is an argmax).  ids (S1,B): the codes
    to feed instead of the run's own (the float32 restatement along the float64 trajectory).  relu_mask (S1,B,H): replaces ReLU by
    a multiplication.  grad=True: also the gradients of sum <logits, d_logits> by autograd in the same dtype -- every member of
    g2v_code_dec_grads under its field name, STEP_GRADS per step, dbn (the gradient at a_pre)."""
    S1, B, H, K, att, p = inp["S1"], inp["B"], inp["H"], inp["K"], inp["att"], inp["p"]
    names = WEIGHTS + (ATT_WEIGHTS if att else ())
    w = {k: inp["w"][k].to(dtype).clone().requires_grad_(grad) for k in names}
    h_init = inp["h_init"].to(dtype).clone().requires_grad_(grad)
    enc = inp["enc"].to(dtype).clone().requires_grad_(grad) if att else None
    ke = inp["keep_emb"].to(dtype) if (training and emb_drop) else None
    drop = training and p > 0 and inp["keep_l0"] is not None
    kl0 = inp["keep_l0"].to(dtype) if drop else None
    rm, rv = inp["running_mean"].to(dtype), inp["running_var"].to(dtype)
    mask = None if relu_mask is None else relu_mask.to(dtype)
    npre = max(1, min(n_pre, S1))
    out = {k: [] for k in ("ids", "ec", "u", "a_pre", "a", "bn_stats", "x1", "gates0", "gates1", "logits", "hp", "attw")}
    h0s, h1s, taps = [h_init[0]], [h_init[1]], {"u": [], "a_pre": [], "a": [], "cells": [], "logits": []}
    with torch.set_grad_enabled(grad):
        if att:      # the energies' encoder half is an INPUT (enc_proj); its value is kept, its dependence on enc and W_attn restored
            ep_graph = enc @ w["w_attn"][:, H:].t()
            ep = inp["enc_proj"].to(dtype) + (ep_graph - ep_graph.detach())
        for t in range(S1):
            if ids is not None:
                idt = ids[t]
            elif t < npre:
                idt = inp["codes"][t].clamp(0, K - 1)
            else:
                idt = argmax_lowest(out["logits"][t - 1])
            e = w["emb"][idt]
            if ke is not None:
                e = e * ke[t] * 2.0                                           # Dropout(0.5)
            x = e
            if att:
                hp = h1s[t] @ w["w_attn"][:, :H].t() + w["b_attn"]            # (B,H)
                score = (torch.tanh(hp.unsqueeze(0) + ep) * w["v_attn"]).sum(2)      # (Tw,B)
                aw = torch.softmax(score.t(), dim=1)                          # (B,Tw), over ALL Tw positions
                x = torch.cat([e, torch.einsum("bt,tbh->bh", aw, enc)], 1)
                out["hp"].append(hp); out["attw"].append(aw)
            c = x @ w["w_pre"].t()
            u = c + w["b_pre"]
            if training:
                mc = c.mean(0)                                                # the sums the kernels form: of c and of c^2
                var = torch.clamp((c * c).mean(0) - mc * mc, min=0.0)         # biased, one pass
                mean, invstd = mc + w["b_pre"], 1.0 / torch.sqrt(var + EPS)
                rm = 0.9 * rm + 0.1 * mean.detach()
                rv = 0.9 * rv + 0.1 * (var.detach() * (B / (B - 1)) if B > 1 else var.detach())
                out["bn_stats"].append(torch.stack([mean, invstd]))
            else:
                mean, invstd = rm, 1.0 / torch.sqrt(rv + EPS)
            a_pre = (u - mean) * invstd * w["bn_w"] + w["bn_b"]
            a = torch.relu(a_pre) if mask is None else a_pre * mask[t]
            cells = []
            h0, g0 = R._cell(a, h0s[t], w["w_ih0"], w["w_hh0"], w["b_ih0"], w["b_hh0"], cells)
            x1 = kl0[t] * h0 / (1.0 - p) if drop else h0                      # nn.GRU's inter-layer dropout, training only
            h1, g1 = R._cell(x1, h1s[t], w["w_ih1"], w["w_hh1"], w["b_ih1"], w["b_hh1"], cells)
            logits = h1 @ w["w_out"].t() + w["b_out"]
            if inp["tie"] is not None:      # rows k1 and k2 of w_out and b_out are identical: one dot product, not two
                k1, k2 = inp["tie"][:2]
                col = logits[:, k1:k1 + 1].detach() + (logits[:, k2:k2 + 1] - logits[:, k2:k2 + 1].detach())      # (k1's value, k2's graph)
                logits = torch.cat([logits[:, :k2], col, logits[:, k2 + 1:]], 1)
            h0s.append(h0); h1s.append(h1)
            taps["u"].append(u); taps["a_pre"].append(a_pre); taps["a"].append(a); taps["cells"].append(cells); taps["logits"].append(logits)
            for name, v in (("ids", idt), ("ec", x), ("u", u), ("a_pre", a_pre), ("a", a), ("x1", x1), ("gates0", g0), ("gates1", g1),
                            ("logits", logits.detach())):
                out[name].append(v)
        res = {k: torch.stack([t.detach() for t in v]) for k, v in out.items() if v}
        res.update(h0=torch.stack([t.detach() for t in h0s]), h1=torch.stack([t.detach() for t in h1s]),
                   running_mean=rm.detach(), running_var=rv.detach(), free=torch.arange(S1) >= npre)
        if not grad:
            return res
        kept = taps["u"] + taps["a_pre"] + taps["a"] + [c for cs in taps["cells"] for c in cs]
        for t in kept:
            t.retain_grad()
        dl = inp["d_logits"].to(dtype)
        sum((taps["logits"][t] * dl[t]).sum() for t in range(S1)).backward()
    zg = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    res["du"] = torch.stack([zg(t) for t in taps["u"]])
    res["dbn"] = torch.stack([zg(t) for t in taps["a_pre"]])
    res["da"] = torch.stack([zg(t) for t in taps["a"]])
    for j, name in enumerate(("dgi0", "dgh0", "dgi1", "dgh1")):
        res[name] = torch.stack([zg(cs[j]) for cs in taps["cells"]])
    res["d_hidden0"] = zg(h_init)
    for k in names:
        res["d_" + k] = zg(w[k])
    if att:
        res["d_enc"] = zg(enc)
    return res


def grad_names(att):
    return ("d_hidden0",) + tuple("d_" + k for k in WEIGHTS + (ATT_WEIGHTS if att else ())) + (("d_enc",) if att else ())


# --------------------------------------------------------------------------------------------------------------- a case's reference
def mode_of(case):
    return dict(n_pre=case["n_pre"], training=bool(case["training"]), emb_drop=bool(case["emb_drop"]))


def case_key(case):
    return (case["S1"], case["B"], case["H"], case["K"], case["Tw"], bool(case["att"]), case["p"], case["n_pre"], bool(case["training"]),
            bool(case["emb_drop"]), case["seed"], case["tie"])


def fwd_names(case):
    """the saved arrays a call of the case writes"""
    names = ["ec", "u", "h0", "h1", "logits"] + (["hp", "attw"] if case["att"] else [])
    if case["training"]:
        names += ["a", "bn_stats", "gates0", "gates1"] + (["x1"] if case["p"] > 0 else [])
    return names


def gap(logits, free, tie):
    """smallest distance between the two largest logits of a row over the steps whose argmax is fed (t + 1 free-running, t + 1 <
    S1); the planted pair counts as one code.  inf where nothing is fed back."""
    S1 = logits.shape[0]
    rows = [logits[t] for t in range(S1 - 1) if bool(free[t + 1])]
    if not rows:
        return float("inf")
    lg = torch.stack(rows).double()
    if tie is not None:
        lg = torch.cat([lg[..., :tie[1]], lg[..., tie[1] + 1:]], -1)
    top = lg.topk(2, dim=-1).values
    return float((top[..., 0] - top[..., 1]).min())


@functools.lru_cache(maxsize=2)
def _reference(key):
    S1, B, H, K, Tw, att, p, n_pre, training, emb_drop, seed, tie = key
    inp = make_inputs(S1, B, H, K, Tw, att, p, seed, tie)
    mode = dict(n_pre=n_pre, training=training, emb_drop=emb_drop)
    f64 = rollout(inp, torch.float64, **mode)
    f32 = rollout(inp, torch.float32, ids=f64["ids"], **mode)       # along the float64 trajectory
    ref = {"inp": inp, "mode": mode, "f64": f64}
    ref["tau_arg"] = 8.0 * float((f32["logits"].double() - f64["logits"]).abs().max())
    ref["gap_min"] = gap(f64["logits"], f64["free"], tie)
    ref["ids32_differ"] = int((rollout(inp, torch.float32, **mode)["ids"] != f64["ids"]).sum())      # the float32 run left to itself
    ref["tau"] = 8.0 * float((f32["a_pre"].double() - f64["a_pre"]).abs().max())
    ref["ambiguous"] = f64["a_pre"].abs() < ref["tau"]
    ref["pattern"] = f64["a_pre"] > 0
    ref["pattern32_differs"] = int((((f32["a_pre"] > 0) != ref["pattern"]) & ~ref["ambiguous"]).sum())
    ref["e32"] = {k: step_err(f32[k], f64[k], steps_of(k)) for k in SAVED + ("running_mean", "running_var") if k in f64}
    if training:      # the gradient noise: both dtypes under the float64 ReLU pattern and the float64 ids
        g64 = rollout(inp, torch.float64, ids=f64["ids"], relu_mask=ref["pattern"], grad=True, **mode)
        g32 = rollout(inp, torch.float32, ids=f64["ids"], relu_mask=ref["pattern"], grad=True, **mode)
        names = STEP_GRADS + ("dbn",) + grad_names(att)
        ref["g64"] = {k: g64[k] for k in names}
        ref["g32_d_b_pre"] = float(g32["d_b_pre"].abs().max())
        ref["e32"].update({k: step_err(g32[k], g64[k], steps_of(k)) for k in names if float(g64[k].abs().max()) > 0})
    return ref


def reference(case):
    """inputs, the float64 forward (and backward under its own ReLU pattern), e32 per array and step, tau and the ambiguous ReLU
    elements, tau_arg and the smallest argmax gap of one case of CODE_F64_CASES; the last two cases stay cached"""
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
    g = rollout(ref["inp"], torch.float64, ids=ref["f64"]["ids"], relu_mask=torch.where(ref["ambiguous"], dev, ref["pattern"]), grad=True,
                **ref["mode"])
    return {k: g[k] for k in ref["g64"]}, differs


def admissible(case):
    """(ok, why) of the conditions on a case's inputs: the argmax gap at every free-running step and row, no ReLU decision of the
    float32 restatement differing away from zero"""
    ref = reference(case)
    if not ref["gap_min"] > ref["tau_arg"]:
        return False, f"argmax gap {ref['gap_min']:.2e} <= tau_arg {ref['tau_arg']:.2e}"
    if ref["pattern32_differs"]:
        return False, f"{ref['pattern32_differs']} float32 ReLU decisions differ away from zero"
    return True, ""
