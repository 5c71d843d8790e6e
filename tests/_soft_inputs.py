"""Seeded inputs, the staged reference and the error bound of the soft quantiser tests (tests/test_soft_quantiser_reference.py on the
host, tests/test_gpu_soft_quantiser.py on the GPU).  Plain torch on the CPU, no GPU, no fixture file.

staged(): oracle.g2v_oracle.vq_gssoft_forward restated with flat, logvar and dist as autograd LEAVES, so the gradient arriving at each
of them (dflat, dlogvar, dd: arrays the kernels write) has a counterpart; evaluated in float64 it is the reference, in float32 "the
fp32 oracle" whose distance from float64 is the rounding noise floor e32 of an output on an input."""
import functools
from collections import namedtuple

import torch

from oracle import g2v_oracle as O

BETA, G_SCALE, G_LOSS = 0.25, 0.7, 0.4      # commitment cost; d L / d q_latent (the factor inside dq); d L / d loss at the input gradient
Case = namedtuple("Case", "N E K scale lv_w lv_b")
FLAT = (0.3, 0.1)                            # logvar_layer weight scale (x 1/sqrt(E)) and bias scale: s = exp(-2 logvar) ~ 1
PEAKED = (1.0, 1.25)                         # s spreads over orders of magnitude: the s-dependent factors of dd / dlogvar matter


def _c(N, E, K, scale, regime=FLAT):
    return Case(N, E, K, scale, *regime)


# the separate kernels (csrc/vq.hip + dense products), every shape
SEPARATE_CASES = {
    "4096x400x512": _c(4096, 400, 512, 0.3),           # shipped width; > 2048*256 elements: the grid-stride loops wrap
    "517x400x512": _c(517, 400, 512, 0.3),             # N % 4 == 1
    "1x400x512": _c(1, 400, 512, 0.3),
    "257x100x70": _c(257, 100, 70, 0.5),               # E % 64 != 0, K % 64 != 0
    "33x64x48": _c(33, 64, 48, 0.5),                   # K < 64: idle lanes
    "130x128x1100": _c(130, 128, 1100, 0.3),           # K > 1024
    "2051x128x512": _c(2051, 128, 512, 0.3),           # a shape the fused kernels also serve
    "517x400x512-peaked": _c(517, 400, 512, 1.0, PEAKED),
}
# the fused kernels (csrc/vq_soft.hip): E = 128, K % 128 == 0, K <= 1024
FUSED_CASES = {
    "1x128x128": _c(1, 128, 128, 0.5),
    "15x128x384": _c(15, 128, 384, 0.3),
    "16x128x512": _c(16, 128, 512, 1.0),
    "17x128x1024": _c(17, 128, 1024, 0.3),
    "1030x128x512": _c(1030, 128, 512, 0.3),
    "4101x128x512": _c(4101, 128, 512, 0.3),
    "1030x128x512-peaked": _c(1030, 128, 512, 1.0, PEAKED),
    "4096x128x512-peaked3": _c(4096, 128, 512, 3.0, PEAKED),
}
# VQ_Payam_GSSoft as a module (inputs (2, B, E / 2), B = 1024 = N): shipped shape and E = 128, both regimes.  The module takes the
# separate launches at both widths (only the engine calls the fused pair), so E = 128 is a second shape of that route
MODULE_CASES = {
    "1024x400x512": _c(1024, 400, 512, 0.3),
    "1024x400x512-peaked": _c(1024, 400, 512, 1.0, PEAKED),
    "1024x128x512": _c(1024, 128, 512, 0.3),
    "1024x128x512-peaked": _c(1024, 128, 512, 1.0, PEAKED),
}
ALL_CASES = {**{"sep-" + k: v for k, v in SEPARATE_CASES.items()}, **{"fused-" + k: v for k, v in FUSED_CASES.items()},
             **{"module-" + k: v for k, v in MODULE_CASES.items()}}

FORWARD = ("flat", "logvar", "dist", "probs", "q", "mse", "loss_vq", "quant", "perplexity", "dq")
BACKWARD = ("dd", "dlogvar", "rowsum", "dflat", "gz", "g_mean_w", "g_mean_b", "g_logvar_w", "g_logvar_b", "g_embedding")
OUTPUTS = FORWARD + BACKWARD
# No bound is looser than what tests/test_gpu_thin_models.py::test_fused_soft_quantiser_kernels_equal_the_separate_kernels allows
# between the two routes for the same quantity (3e-4, its gradient tolerance, for what it does not compare).
CAP = {"flat": 1e-5, "logvar": 1e-5, "dist": 2e-5, "probs": 5e-5, "q": 2e-5, "dq": 1e-4, "quant": 2e-5, "mse": 1e-5, "loss_vq": 1e-5,
       "perplexity": 1e-5, "dd": 3e-4, "dlogvar": 3e-4, "rowsum": 3e-4, "dflat": 3e-4, "gz": 3e-4, "g_mean_w": 3e-4, "g_mean_b": 3e-4,
       "g_logvar_w": 3e-4, "g_logvar_b": 3e-4, "g_embedding": 3e-4}
MARGIN = 8.0
# assign(): a row whose two largest float64 probabilities are closer than this (relative to the larger) may go either way in fp32;
# 50 x the largest fp32 noise floor of probs (2e-6)
ASSIGN_BAND = 1e-4


def make_inputs(case: Case, seed: int = 0):
    """float32 CPU tensors of one case: x (N,E) rows, the three layers' parameters, dh (N,E) the gradient at the quantised value"""
    N, E, K, scale, lv_w, lv_b = case
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * N + 31 * E + K)
    r = lambda *s, m=1.0: torch.randn(*s, generator=g) * m
    return {"x": r(N, E, m=scale), "w_mean": r(E, E, m=E ** -0.5), "b_mean": r(E, m=0.1), "w_logvar": r(K, E, m=lv_w * E ** -0.5),
            "b_logvar": r(K, m=lv_b), "codebook": r(K, E, m=scale), "dh": r(N, E, m=1e-3)}


def state_dict(inp, prefix=""):
    E = inp["x"].shape[1]
    return {prefix + "mean_layer.weight": inp["w_mean"], prefix + "mean_layer.bias": inp["b_mean"],
            prefix + "logvar_layer.weight": inp["w_logvar"], prefix + "logvar_layer.bias": inp["b_logvar"],
            prefix + "_embedding.weight": inp["codebook"], prefix + "pre_linear.weight": torch.eye(E, dtype=inp["x"].dtype),
            prefix + "pre_linear.bias": torch.zeros(E, dtype=inp["x"].dtype)}


def staged(inp, dtype=torch.float64, beta=BETA, g_scale=G_SCALE, g_loss=G_LOSS):
    """Forward of vq_gssoft_forward and the backward of L = sum(quant dh) + g_scale q_latent + g_loss beta e_latent (g_scale == g_loss:
    L = sum(quant dh) + g_loss loss) in `dtype`; every name of OUTPUTS."""
    t = {k: v.detach().to(dtype) for k, v in inp.items()}
    N, E = t["x"].shape
    leaf = lambda v: v.detach().clone().requires_grad_(True)
    x, Wm, bm, Wl, bl, W = (leaf(t[k]) for k in ("x", "w_mean", "b_mean", "w_logvar", "b_logvar", "codebook"))
    flat0 = O.linear(x, Wm, bm)                                              # :1391
    flat = leaf(flat0)
    logvar0 = O.linear(flat, Wl, bl)                                         # :1392
    dist0 = O.vq_distances(flat, W)                                          # :1396-1400
    logvar, dist = leaf(logvar0), leaf(dist0)
    smooth = 1.0 / torch.exp(logvar) ** 2                                    # :1411
    prob = torch.exp(-((dist / 400) * (0.5 * smooth))) / torch.sqrt(smooth)  # :1351,1361
    probs = prob / prob.sum(1, keepdim=True)                                 # :1368
    q = probs @ W                                                            # :1417-1421
    e_latent = ((q.detach() - x) ** 2).mean()                                # :1424
    q_latent = ((q - x.detach()) ** 2).mean()                                # :1425
    quant = x + (q - x).detach()                                             # :1431
    avg = probs.mean(0)
    perplexity = torch.exp(-(avg * torch.log(avg + 1e-10)).sum())            # :1432-1433
    mse = q_latent.detach()
    out = {"flat": flat0, "logvar": logvar0, "dist": dist0, "probs": probs, "q": q, "mse": mse, "loss_vq": (1 + beta) * mse,
           "quant": quant, "perplexity": perplexity, "dq": g_scale * 2 * (q - x) / (N * E)}
    ((quant * t["dh"]).sum() + g_scale * q_latent + g_loss * beta * e_latent).backward()
    out.update(dd=dist.grad, dlogvar=logvar.grad, rowsum=dist.grad.sum(1))
    torch.autograd.backward([dist0, logvar0], [dist.grad, logvar.grad])
    out["dflat"] = flat.grad
    flat0.backward(flat.grad)
    out.update(gz=x.grad, g_mean_w=Wm.grad, g_mean_b=bm.grad, g_logvar_w=Wl.grad, g_logvar_b=bl.grad, g_embedding=W.grad)
    return {k: v.detach() for k, v in out.items()}


def relerr(got, ref, scale=None) -> float:
    """max-norm error relative to the reference's max-norm (or to `scale`)"""
    got = torch.as_tensor(got).detach().cpu().double().reshape(-1)
    ref = torch.as_tensor(ref).detach().cpu().double().reshape(-1)
    return float((got - ref).abs().max()) / max(float(ref.abs().max()) if scale is None else scale, 1e-300)


def err(got: dict, ref: dict, k: str) -> float:
    """relerr of output k.  rowsum_n = sum_k dd_nk cancels (sum_k g_k = 0, and s ~ 1 in the flat regime), so its own max-norm is no
    measure of the rounding of that sum: it is taken relative to max_n sum_k |dd_nk|, the size of what was added.  Measured on the
    float64 reference, max_n |rowsum_n| / max_n sum_k |dd_nk| is 9.2e-5 at (1, 400, 512), where no second row sets the scale, 2.3e-2
    to 1.3e-1 in the other flat cases and 1.0 in the peaked one.  With the fp32 oracle's error put on rowsum's own max-norm, the single
    row would get e32 = 9.1e-5 (the others 6e-7 to 1.6e-6), that figure would be the floor of every case, and the bound would be
    2.1e-6 to 9e-5 of the summed magnitudes wherever N > 1, against about 1.3e-6 to 7.7e-6 here; at N = 1 it would ask for 2.8e-8 of the
    summed magnitudes, under the fp32 unit roundoff (6e-8) of a single term.
    tests/test_gpu_soft_quantiser.py also checks rowsum against the sum of the kernel's own dd."""
    return relerr(got[k], ref[k], float(ref["dd"].abs().sum(1).max()) if k == "rowsum" else None)


def g_scale_of(name: str) -> float:
    """the module takes one factor for the whole loss (L = sum(quant dh) + g_loss loss); the kernel-level cases keep the two apart"""
    return G_LOSS if name.startswith("module-") else G_SCALE


@functools.lru_cache(maxsize=None)
def reference(name: str):
    """(inputs, float64 staged reference) of ALL_CASES[name]"""
    inp = make_inputs(ALL_CASES[name])
    return inp, staged(inp, torch.float64, g_scale=g_scale_of(name))


@functools.lru_cache(maxsize=None)
def noise(name: str):
    """e32 of every output of ALL_CASES[name]: the fp32 oracle against float64"""
    inp, ref = reference(name)
    o32 = staged(inp, torch.float32, g_scale=g_scale_of(name))
    return {k: err(o32, ref, k) for k in OUTPUTS}


@functools.lru_cache(maxsize=None)
def floors():
    """per output, the largest e32 over every case.  It evaluates the float64 and the fp32 reference of all 20 cases, (4096, 400, 512)
    included, once per process on first use, even when one test is selected: about 10 s on the CPU."""
    return {k: max(noise(n)[k] for n in ALL_CASES) for k in OUTPUTS}


def bound(name: str, output: str) -> float:
    """e_kernel <= max(8 e32, floor), and never looser than CAP.  The margin of 8 covers another fixed summation order (MFMA four-wide
    chains, wave reductions) and a device expf / division a couple of ulp looser than the host's."""
    return min(max(MARGIN * noise(name)[output], floors()[output]), CAP[output])


def check_outputs(name: str, got: dict, label: str, only=None):
    """print e_kernel, e32 and their ratio per output, then assert the bound on all of them; returns {output: ratio}"""
    _, ref = reference(name)
    rows, bad = {}, []
    for k in (only or OUTPUTS):
        if k not in got:
            continue
        ek, e32, b = err(got, ref, k), noise(name)[k], bound(name, k)
        finite = bool(torch.isfinite(torch.as_tensor(got[k]).detach().float()).all())
        rows[k] = ek / max(e32, 1e-300)
        print(f"{label} {name} {k}: e_kernel {ek:.3e} e32 {e32:.3e} ratio {rows[k]:.2f} bound {b:.3e}")
        if not finite or not ek <= b:
            bad.append((k, ek, e32, b))
    assert not bad, (label, name, bad)
    return rows


def near_tie_rows(probs64):
    """rows whose two largest probabilities differ by less than ASSIGN_BAND of the larger"""
    top2 = probs64.topk(2, dim=1).values
    return (top2[:, 0] - top2[:, 1]) < ASSIGN_BAND * top2[:, 0]
