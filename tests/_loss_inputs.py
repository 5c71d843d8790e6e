"""Seeded inputs, float64 references and error bounds of the loss / optimiser kernel tests (tests/test_loss_reference.py on the host,
tests/test_gpu_loss_path.py on the GPU): custom_loss + finalize, the MSE pair, sumsq + clip_adam (csrc/misc.hip) and the
cross-entropy pair (csrc/seq2seq.hip).  Plain torch on the CPU, no GPU code, no fixture file.

Every reference is a callable in a dtype: in float64 it is the reference, in float32 "the fp32 oracle" whose distance from float64
is the rounding noise floor e32 of an output on an input.

ARRAY outputs (custom_loss dy, cross-entropy gradient, Adam p / m / v) follow tests/_soft_inputs.py: e_kernel <= min(max(8 e32,
floor), cap), floor the largest e32 of that output over all cases of its op, cap the tolerance of the op's existing test.

SCALAR outputs are sums of non-negative terms (l1, cont, -var, mse of custom_loss; the MSE loss; gnorm^2; the mean of the
cross-entropy row losses lse - z_t >= 0), for which e32 can be luckily tiny; their bound is a priori.  In a fixed-order fp32 sum of
non-negative terms every addition rounds a partial sum that is no larger than the total, and every rounding of a term is relative
to that term, so the result is within (1 + u)^(depth + c) - 1 ~ (depth + c) u of the exact sum, u = 2^-24, depth the longest chain
of additions one term passes through, c the roundings applied to one term and to the final scaling.  depth and c are counted from
the kernels below, next to each formula; nothing here comes from what the kernels return."""
import functools
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

U = 2.0 ** -24                 # fp32 unit roundoff (round to nearest)
MARGIN = 8.0
CAP = {"dy": 1e-5, "ce_grad": 2e-5, "p": 1e-5, "m": 1e-5, "v": 1e-5}


def gamma(k: float) -> float:
    """(1 + u)^k - 1: the relative error k roundings can compound to"""
    return math.expm1(k * math.log1p(U))


def relerr(got, ref, scale=None) -> float:
    """max-norm error relative to the reference's max-norm (or to `scale`); 0 when both are identically zero"""
    got = torch.as_tensor(got).detach().cpu().double().reshape(-1)
    ref = torch.as_tensor(ref).detach().cpu().double().reshape(-1)
    return float((got - ref).abs().max()) / max(float(ref.abs().max()) if scale is None else scale, 1e-300)


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


# ================================================================================================ custom_loss
CLCase = namedtuple("CLCase", "B T D weights scale g_scale")
W_SHIPPED = (5.0, 0.1, 0.5)


def _cl(B, T, D, weights=W_SHIPPED, scale=1.0):
    return {f"{B}x{T}x{D}" + ("" if weights == W_SHIPPED else "-w123") + ("" if scale == 1.0 else f"-s{scale:g}"):
            (B, T, D, weights, scale)}


_CL_SHAPES = {
    **_cl(1, 1, 1),                      # T = 1: no cont term, first and last frame coincide, generic kernel
    **_cl(1, 2, 3),                      # every frame is a boundary frame
    **_cl(3, 34, 85),                    # reg<34>, 255 columns: one partial workgroup
    **_cl(2, 34, 128),                   # exactly 256 columns
    **_cl(1, 34, 257),                   # a second workgroup holding one column
    **_cl(5, 20, 135),                   # reg<20>, 3 workgroups
    **_cl(7, 9, 40),                     # generic, 2 workgroups
    **_cl(3, 33, 135),                   # generic kernel on one side of a compile-time T
    **_cl(3, 35, 135),                   # generic kernel on the other side
    **_cl(300, 34, 1),                   # D = 1
    **_cl(490, 34, 135),                 # 259 workgroups: reg<34>, the finalize's second pass with a ragged tail
    **_cl(600, 20, 135),                 # 317 workgroups: reg<20>, the same
    **_cl(4096, 6, 135),                 # 2160 workgroups: generic kernel at the shipped B D
    **_cl(2, 34, 128, weights=(1.0, 2.0, 3.0)),
    **_cl(5, 20, 135, scale=1e3),
    **_cl(3, 33, 135, scale=1e-3),
}
# every shape at both gradient scales (1/3 is not a power of two: the product g_scale * grad rounds)
G_SCALES = {"": 1.0, "-g3": 1.0 / 3.0}
CL_CASES = {name + tag: CLCase(*c, g) for name, c in _CL_SHAPES.items() for tag, g in G_SCALES.items()}


def cl_planted(case: CLCase):
    """where the edge values sit ((b, d) columns, (b, t) frames, (b, t, d) elements); None for T == 1, where nothing is planted.
    With B == 1 the repeated frame covers the first half of D only, so that the other columns keep a cont term."""
    B, T, D = case[:3]
    if T == 1:
        return None
    return {"zero_col": (B - 1, D - 1),                      # the last column: the tail of the last workgroup
            "const_col": (0, 0),
            "repeat": (B // 2, T // 2, D if B > 1 else max(1, D // 2)),      # y[b, t, :nd] = y[b, t - 1, :nd]
            "equal": (B // 2, 0, D // 2)}                    # y == target


def cl_inputs(name: str):
    """float32 CPU (output (B,T,D), target (B,T,D)) of CL_CASES[name], edge values planted"""
    case = CL_CASES[name]
    B, T, D, _, scale, _ = case
    g = _gen(11, B, T, D, round(math.log10(scale)) + 7)
    tgt = torch.randn(B, T, D, generator=g) * scale
    out = 0.7 * tgt + torch.randn(B, T, D, generator=g) * (0.5 * scale)
    pl = cl_planted(case)
    if pl:
        b, d = pl["const_col"]
        out[b, :, d] = out[b, 0, d]
        b, t, nd = pl["repeat"]
        out[b, t, :nd] = out[b, t - 1, :nd]
        b, d = pl["zero_col"]
        out[b, :, d] = 0.0
        b, t, d = pl["equal"]
        tgt[b, t, d] = out[b, t, d]
    return out, tgt


def custom_loss(output, target, weights, g_scale=1.0, dtype=torch.float64):
    """train_eval/train_seq2seq.py:40-88 on (B,T,D), restated: -> dict total, l1, cont, var, mse (0-d) and dy = g_scale dL/d output.
    The time norm is torch.norm(o, 2, 1) as the reference has it: its subgradient at an all-zero column is 0 (the kernels'
    loss_col_coef: cn = 0), where sqrt(sum(o^2)) would give NaN."""
    w_l1, w_cont, w_var = weights
    o = output.detach().to(dtype).clone().requires_grad_(True)
    t = target.detach().to(dtype)
    n = o.numel()
    l1 = F.l1_loss(o, t) * w_l1                                                           # :61-62
    if o.shape[1] > 1:
        diff = [abs(o[:, k, :] - o[:, k - 1, :]) for k in range(1, o.shape[1])]           # :65-67
        cont = torch.sum(torch.stack(diff)) / n * w_cont                                  # :68-69
    else:
        cont = o.sum() * 0.0                                                              # (torch.stack of nothing raises)
    var = -torch.sum(torch.norm(o, 2, 1)) / n * w_var                                     # :72-74
    total = l1 + cont + var                                                               # :76
    (g,) = torch.autograd.grad(total, o)
    return {"total": total.detach(), "l1": l1.detach(), "cont": cont.detach(), "var": var.detach(),
            "mse": ((o.detach() - t) ** 2).mean(), "dy": g * g_scale}


@functools.lru_cache(maxsize=None)
def cl_reference(name: str):
    out, tgt = cl_inputs(name)
    c = CL_CASES[name]
    return custom_loss(out, tgt, c.weights, c.g_scale, torch.float64)


@functools.lru_cache(maxsize=None)
def cl_noise(name: str):
    """e32 of dy and of the five scalars (the latter only printed: their bound is a priori)"""
    out, tgt = cl_inputs(name)
    c = CL_CASES[name]
    ref, o32 = cl_reference(name), custom_loss(out, tgt, c.weights, c.g_scale, torch.float32)
    e = {"dy": relerr(o32["dy"], ref["dy"])}
    for k in ("l1", "cont", "var", "mse"):
        e[k] = relerr(o32[k], ref[k])
    e["total"] = relerr(o32["total"], ref["total"], cl_total_scale(ref))
    return e


def cl_total_scale(ref) -> float:
    """terms[0] = l1 + cont + var cancels (var < 0): its error is measured against |l1| + |cont| + |var|"""
    return float(ref["l1"].abs() + ref["cont"].abs() + ref["var"].abs())


def cl_blocks(B, D) -> int:
    return -(-(B * D) // 256)


def cl_scalar_bounds(case: CLCase):
    """relative bounds of terms[1..4] and of terms[0] against cl_total_scale, counted from custom_loss_kernel /
    custom_loss_reg_kernel<T> / custom_loss_finalize_kernel / loss_terms_write (csrc/misc.hip, csrc/common.hpp).
    The chain of additions shared by all four sums, after the per-column value exists:
        6   wave_sum: six xor-shuffle levels
        2   (red[0] + red[1]) + (red[2] + red[3]) over the workgroup's four waves
        ceil(nblk / 256)   the finalize's strided pass: one thread adds that many partials
        6 + 2   the finalize's wave_sum and four-wave sum
    l1, cont and mse also walk the column: T additions into the running sum (T - 1 for cont).
    Roundings of one term, and of the final scaling:
        l1    1 (v - tv) + 3 (c1 = float(w) / float(n): the cast of w, the division; the product s_l1 * c1)        c = 4
        cont  1 (v - prev) + 3 (the same with c2)                                                                    c = 4
        mse   3 ((v - tv) rounds once, its square carries that twice and rounds again; an fma contraction only
              removes one) + 2 (inv_n = 1.0f / n, the product)                                                       c = 5
        var   the term is the column norm sqrt(ss): ss is a chain of T fmaf, each one rounding of a partial sum of
              non-negative squares, so ss is within T u; the square root halves that and rounds (counted as 2: one
              ulp, should sqrtf not be correctly rounded): T / 2 + 2.  Plus 3 for c3 and the product.               c = T / 2 + 5
    n = T B D is exact in fp32 for every case here (< 2^24), its three-factor product float(T) * float(B) * float(D) too.
    terms[0]: two more additions, each rounding a partial sum no larger than |l1| + |cont| + |var|, on top of the terms' own
    errors (each relative to its own magnitude): max of the three bounds + 2 u, against |l1| + |cont| + |var|."""
    B, T, D = case[:3]
    tail = 6 + 2 + -(-cl_blocks(B, D) // 256) + 6 + 2
    b = {"l1": gamma(T + tail + 4), "cont": gamma(max(T - 1, 0) + tail + 4), "mse": gamma(T + tail + 5),
         "var": gamma(tail + T / 2 + 5)}
    b["total"] = max(b["l1"], b["cont"], b["var"]) + gamma(2)
    return b


# ================================================================================================ MSE
MSE_SIZES = (1, 63, 255, 256, 257, 1023, 1025, 2 ** 20 + 3, 3 * 2 ** 20 + 5)
MSE_G_SCALES = (1.0, 0.25)
MSE_CASES = {f"{n}-g{g:g}": (n, g) for n in MSE_SIZES for g in MSE_G_SCALES}
# dy[e] = (2 g_scale / n) (y - t): the cast of g_scale to float, the division by float(n) (n < 2^24: exact; 2 g exact), the
# subtraction, the product: four roundings, each relative to the value itself, so the bound holds per element
MSE_DY_ROUNDINGS = 4


def mse_inputs(name: str):
    n, _ = MSE_CASES[name]
    g = _gen(23, n)
    t = torch.randn(n, generator=g)
    return t + 0.3 * torch.randn(n, generator=g), t


def mse(y, t, g_scale=1.0, dtype=torch.float64):
    y, t = y.detach().to(dtype), t.detach().to(dtype)
    n = y.numel()
    return {"loss": ((y - t) ** 2).mean(), "dy": g_scale * 2 * (y - t) / n}


@functools.lru_cache(maxsize=None)
def mse_reference(name: str):
    return mse(*mse_inputs(name), MSE_CASES[name][1], torch.float64)


def mse_blocks(n: int) -> int:
    return min(-(-n // 1024), 1024)


def mse_loss_bound(n: int) -> float:
    """mse_kernel / mse_finalize_kernel.  The term d * d: d = y - t rounds once, the square carries that twice and rounds: 3.
    depth: ceil(n / (256 nblk)) additions of the thread's grid-stride loop, 6 (wave_sum), 2 (four waves), ceil(nblk / 256) in the
    finalize's strided pass, 6 + 2 again.  Final scaling: float(n), 1.0f / that, the product: 3."""
    nblk = mse_blocks(n)
    return gamma(-(-n // (256 * nblk)) + 6 + 2 + -(-nblk // 256) + 6 + 2 + 3 + 3)


# ================================================================================================ clip + Adam
ADAM_SIZES = (1, 63, 257, 1025, 100003, 2 ** 21 + 3)
ADAM_GRAD_SCALES = (1.0, 0.125)
ADAM_STEPS = 4
MAX_NORM, LR, BETAS, EPS = 5.0, 5e-4, (0.5, 0.999), 1e-8
# The C ABI takes the betas as float (include/g2v.h: g2v_clip_adam_step), so the operation under test is Adam at the fp32 values
# of (0.5, 0.999), as custom_loss is evaluated at the fp32 inputs: converted to float64 unchanged.  fl32(0.999) = 0.99900001287...
# and 1 - beta2 amplifies that thousandfold: with beta2 = 0.999 as a double the reference's v would sit 1.29e-5 (relative) from the
# v of any implementation that is handed the float, a distance that says nothing about the kernel (measured so on the MI355X:
# 1.26e-5 to 1.30e-5 in all 48 cases).  p never shows it: v / (1 - beta2^t) is a weighted mean of g^2 under either value.
BETAS_ABI = tuple(float(torch.tensor(b, dtype=torch.float32)) for b in BETAS)
# ||g grad_scale|| / max_norm of the four steps: never within 1e-3 of 1, so that rounding cannot change the clip decision
ADAM_REGIMES = {
    "unclipped": (0.2, 0.5, 0.1, 0.8),
    "clipped": (3.0, 0.4, 10.0, 1.7),          # clipped, not, clipped, clipped
    "zero-first": (0.0, 0.6, 2.0, 0.3),        # step 1 has an all-zero gradient: m = v = 0, denom = eps, the update must be 0
    "zero-init": (0.5, 2.5, 0.7, 0.2),         # p0 = 0: p is the accumulated update, the bias corrections at full relative precision
}
AdamCase = namedtuple("AdamCase", "n grad_scale regime")
ADAM_CASES = {f"{n}-gs{gs:g}-{r}": AdamCase(n, gs, r) for n in ADAM_SIZES for gs in ADAM_GRAD_SCALES for r in ADAM_REGIMES}
CLIP_BAND = (0.999, 1.001)


def adam_inputs(name: str):
    """float32 CPU p0 (n) and the steps' gradients (ADAM_STEPS, n): direction random, norm set so that ||g grad_scale|| is the
    regime's multiple of max_norm"""
    n, gs, regime = ADAM_CASES[name]
    g = _gen(37, n, list(ADAM_REGIMES).index(regime))
    p0 = torch.zeros(n) if regime == "zero-init" else torch.randn(n, generator=g)
    grads = []
    for ratio in ADAM_REGIMES[regime]:
        d = torch.randn(n, generator=g).double()
        grads.append((d / d.norm() * (ratio * MAX_NORM / gs)).float())
    return p0, torch.stack(grads)


def clip_adam(p0, grads, grad_scale, dtype=torch.float64, max_norm=MAX_NORM, lr=LR, betas=BETAS_ABI, eps=EPS):
    """torch.nn.utils.clip_grad_norm_ (coef = min(1, max_norm / (||g grad_scale|| + 1e-6))) on the scaled gradient, then
    torch.optim.Adam's arithmetic at the betas the ABI carries; -> p, m, v after the last step, gnorm of every step, step"""
    b1, b2 = betas
    p = p0.detach().to(dtype).clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    gnorm = []
    for t, g in enumerate(grads, start=1):
        g = g.detach().to(dtype) * grad_scale
        total = torch.sqrt((g * g).sum())              # (torch.sum is pairwise: in fp32 it keeps the oracle's own error near u)
        gnorm.append(total)
        g = g * torch.clamp(max_norm / (total + 1e-6), max=1.0)
        m = m * b1 + (1 - b1) * g
        v = v * b2 + (1 - b2) * g * g
        denom = v.sqrt() / math.sqrt(1 - b2 ** t) + eps
        p = p - (lr / (1 - b1 ** t)) * (m / denom)
    return {"p": p, "m": m, "v": v, "gnorm": torch.stack(gnorm), "step": len(grads)}


def clip_ratios(name: str):
    """||g grad_scale|| / max_norm per step on the float64 reference"""
    return [float(x) / MAX_NORM for x in adam_reference(name)["gnorm"]]


@functools.lru_cache(maxsize=None)
def adam_reference(name: str):
    p0, grads = adam_inputs(name)
    ref = clip_adam(p0, grads, ADAM_CASES[name].grad_scale, torch.float64)
    lo, hi = CLIP_BAND
    for r in (float(x) / MAX_NORM for x in ref["gnorm"]):
        assert not lo <= r <= hi, f"{name}: clip ratio {r} is within rounding reach of 1"     # a condition on the inputs
    return ref


@functools.lru_cache(maxsize=None)
def adam_noise(name: str):
    p0, grads = adam_inputs(name)
    ref, o32 = adam_reference(name), clip_adam(p0, grads, ADAM_CASES[name].grad_scale, torch.float32)
    return {k: relerr(o32[k], ref[k]) for k in ("p", "m", "v", "gnorm")}


def adam_blocks(n: int) -> int:
    return min(-(-n // 1024), 1024)


def gnorm_bound(n: int) -> float:
    """sumsq_kernel + the head of clip_adam_kernel.  gnorm^2 is a sum of non-negative terms g * g (1 rounding): depth =
    ceil(n / (256 nblk)) in the grid-stride loop + 6 + 2, then ceil(nblk / 256) + 6 + 2 over the partials.  The square root halves
    the relative error of the sum and rounds (counted as 2, one ulp); total = bc * grad_scale: the cast of grad_scale and the product."""
    nblk = adam_blocks(n)
    sumsq = -(-n // (256 * nblk)) + 6 + 2 + -(-nblk // 256) + 6 + 2 + 1
    return gamma(sumsq / 2 + 2 + 2)


# ================================================================================================ cross entropy
CE_SHAPES = ((1, 1), (1, 7), (5, 63), (4, 64), (6, 65), (3, 512), (257, 400), (4099, 512))
CE_CASES = {f"{M}x{K}": (M, K) for M, K in CE_SHAPES}


def ce_planted(M: int, K: int):
    """rows of the three special regimes (M >= 4 and K >= 2; the smaller cases are logits at scale 3 only)"""
    return {"pm80": M - 1, "far_target": M - 2, "equal": M - 3} if M >= 4 and K >= 2 else None


def ce_inputs(name: str):
    """float32 logits (M,K) at scale 3 and int64 targets; targets hold 0 and K - 1.  Planted rows: entries at +-80 (+ unit noise);
    a row around +5000 whose target logit lies 1e4 below its maximum (loss 1e4, gradient -1/M at the target, and exp(z) without the
    maximum subtracted overflows); a row of all-equal logits."""
    M, K = CE_CASES[name]
    g = _gen(41, M, K)
    z = torch.randn(M, K, generator=g) * 3
    t = torch.randint(0, K, (M,), generator=g)
    t[0] = 0 if M > 1 else K - 1
    t[-1] = K - 1
    pl = ce_planted(M, K)
    if pl:
        r = pl["pm80"]
        z[r] = 80.0 * (2.0 * torch.randint(0, 2, (K,), generator=g) - 1.0) + torch.randn(K, generator=g)
        r = pl["far_target"]
        z[r] += 5000.0
        t[r] = (int(z[r].argmax()) + 1) % K
        z[r, t[r]] = z[r].max() - 1e4
        z[pl["equal"]] = 1.25
    return z, t


def cross_entropy(z, t, dtype=torch.float64):
    zl = z.detach().to(dtype).clone().requires_grad_(True)
    loss = F.cross_entropy(zl, t)
    (g,) = torch.autograd.grad(loss, zl)
    return {"loss": loss.detach(), "grad": g}


@functools.lru_cache(maxsize=None)
def ce_reference(name: str):
    return cross_entropy(*ce_inputs(name), torch.float64)


@functools.lru_cache(maxsize=None)
def ce_noise(name: str):
    ref, o32 = ce_reference(name), cross_entropy(*ce_inputs(name), torch.float32)
    return {"ce_grad": relerr(o32["grad"], ref["grad"]), "loss": abs(float(o32["loss"]) - float(ref["loss"]))}     # loss: ABSOLUTE


def ce_loss_bound(name: str) -> float:
    """ABSOLUTE bound of the mean loss, from ce_kernel + mean_kernel (csrc/seq2seq.hip).  A row: mx is exact; z_k - mx rounds once,
    which moves exp by the factor exp(+-u |z_k - mx|); over the row that is a relative error of s = sum exp(z_k - mx) of at most
    u sum_k p_k (mx - z_k) = u (H(p) - ln s) <= u ln K.  expf: 2 (one ulp).  The sum: ceil(K / 64) additions per lane + 6 levels.
    So s is within (ln K + 2 + ceil(K / 64) + 6) u, and that relative error is the absolute error of ln s.  logf rounds to one ulp
    of |ln s| (2 u |ln s|), lse = mx + ln s rounds (u |lse|), row = lse - z_t rounds (u |row|):
        |row error| <= u (ln K + ceil(K / 64) + 8 + 2 |ln s| + |lse| + |row|).
    The mean is a sum of the non-negative rows: ceil(M / 256) per thread + 6 + 2, the cast of M and the division: relative
    (ceil(M / 256) + 10) u of the mean.  lse, ln s and row are taken from the float64 reference."""
    M, K = CE_CASES[name]
    z, t = ce_inputs(name)
    z = z.double()
    mx = z.max(1).values
    lns = torch.log(torch.exp(z - mx[:, None]).sum(1))
    lse = mx + lns
    row = lse - z[torch.arange(M), t]
    per_row = math.log(K) + -(-K // 64) + 8 + 2 * lns.abs() + lse.abs() + row.abs()
    return gamma(1) * float(per_row.mean()) * (1 + gamma(-(-M // 256) + 10)) + gamma(-(-M // 256) + 10) * float(row.mean())


# ================================================================================================ the array bound
_OP = {"cl": (CL_CASES, cl_noise, ("dy",)), "ce": (CE_CASES, ce_noise, ("ce_grad",)), "adam": (ADAM_CASES, adam_noise, ("p", "m", "v"))}
_OP_OF = {out: op for op, (_, _, outs) in _OP.items() for out in outs}


@functools.lru_cache(maxsize=None)
def _floors_of(op: str):
    cases, noise, outs = _OP[op]
    return {k: max(noise(n)[k] for n in cases) for k in outs}


def floors():
    """per array output, the largest e32 over every case of its op.  Evaluates the float64 and the fp32 reference of every case of
    an op once per process, on first use of a bound of that op: a few seconds on the CPU."""
    return {k: v for op in _OP for k, v in _floors_of(op).items()}


def noise_of(name: str, output: str) -> float:
    return _OP[_OP_OF[output]][1](name)[output]


def bound(name: str, output: str) -> float:
    """e_kernel <= max(8 e32, floor), and never looser than CAP.  The margin of 8 covers another fixed order of the same roundings
    (fma contraction, one rounded reciprocal instead of a division) and a device expf / sqrtf / division an ulp looser than the host's."""
    return min(max(MARGIN * noise_of(name, output), _floors_of(_OP_OF[output])[output]), CAP[output])


def check_array(label, name, output, got, ref, ref_scale=None):
    """print e_kernel, e32, their ratio and the bound; assert finite and within the bound; -> ratio"""
    ek, e32, b = relerr(got, ref, ref_scale), noise_of(name, output), bound(name, output)
    print(f"{label} {name} {output}: e_kernel {ek:.3e} e32 {e32:.3e} ratio {ek / max(e32, 1e-300):.2f} bound {b:.3e}")
    assert bool(torch.isfinite(torch.as_tensor(got).detach().float()).all()), (label, name, output, "not finite")
    assert ek <= b, (label, name, output, ek, e32, b)
    return ek / max(e32, 1e-300)


def check_scalar(label, name, output, got, ref, rel_bound, e32, scale=None):
    """the same for a scalar with an a-priori bound, relative to |ref| (or to `scale`)"""
    got, ref = float(got), float(ref)
    s = abs(ref) if scale is None else scale
    ek = abs(got - ref) / max(s, 1e-300) if got != ref else 0.0
    print(f"{label} {name} {output}: e_kernel {ek:.3e} e32 {e32:.3e} ratio {ek / max(e32, 1e-300):.2f} bound {rel_bound:.3e}"
          f" (e_kernel / bound {ek / rel_bound:.3f})")
    assert math.isfinite(got), (label, name, output, got)
    assert ek <= rel_bound, (label, name, output, got, ref, ek, rel_bound)
    return ek / rel_bound
