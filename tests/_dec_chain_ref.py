"""The generation chain (g2v_dec_chain_fwd, include/g2v.h) and the tail of a generated clip (g2v_clip_finish) restated in plain
torch with the dtype as a parameter, the seeded inputs of their tests and the error bound (tests/test_dec_chain_host.py on the
host, tests/test_gpu_dec_chain.py on the GPU).  No device, no library.

The step is the eval-mode step of tests/_dec_ref.py: its GRU cell (_cell), its BatchNorm on the running statistics, its
Dropout(0.95) as keep * x * 20.  In float64 a run is the reference; in float32 it is the fp32 oracle whose distance from float64
is the rounding noise e32.  Errors are taken per chunk and step with tests/_dec_ref.py's step_err, and the bound is its rule:

  bound = min(MARGIN * max(e32, 2u), cap),  MARGIN = 8, u = 2^-24, cap = 1e-4 (a forward array).

The masks are drawn with keep probability 0.5, not 0.05 (the kernel takes any mask; the scale stays 20): at 0.05 and small D most
steps would drop the whole input, and a broken carry or feedback would pass.  `inputs` asserts that the first step of every chunk
and at least one fed-back step of every chunk keep at least one column for every clip."""
import functools

import numpy as np
import torch

import _dec_ref as R

U, MARGIN, CAP = R.U, R.MARGIN, R.CAP_FWD
KEEP_PROB = 0.5
SAVGOL_WINDOW, SAVGOL_ORDER = 25, 5


def case(C, T, W, B, D, H, *, seed, ids="none", start=True, teacher=False, n_pre=1, conditioned=True, unaligned=False, tag=""):
    """ids: "none" (row b C + c), "edge" (rows 0 and R - 1 are hit and a row repeats; R = B C + 3) or "random" """
    name = f"{C}x{T}x{W}x{B}x{D}x{H}" + (f"-{tag}" if tag else "")
    return dict(id=name, C=C, T=T, W=W, B=B, D=D, H=H, seed=seed, ids=ids, start=start, teacher=teacher, n_pre=n_pre,
                conditioned=conditioned, unaligned=unaligned)


# (C, T, W, B, D, H): the smallest shapes at which the kernel can still go wrong
CASES = [
    case(2, 3, 0, 1, 5, 8, seed=21, ids="none", tag="noids"),
    case(3, 3, 1, 4, 135, 64, seed=12, ids="edge", tag="edgeids"),
    case(2, 4, 5, 17, 40, 200, seed=13, ids="random", tag="ragged"),            # two workgroups, the second ragged
    case(2, 3, 1, 16, 65, 200, seed=14, ids="none", tag="oddD"),                # D off every vector width
    case(2, 4, 1, 3, 5, 8, seed=15, ids="random", teacher=True, n_pre=2, tag="teacher"),
    case(2, 3, 1, 4, 5, 8, seed=26, ids="random", conditioned=False, tag="unconditioned"),
    case(2, 3, 1, 5, 7, 8, seed=17, ids="edge", unaligned=True, tag="unaligned"),
    case(1, 3, 2, 2, 6, 8, seed=18, ids="none", start=False, tag="nostart"),
    case(2, 3, 1, 17, 135, 64, seed=19, ids="random", tag="resident-ragged"),   # the register-resident kernel, two workgroups
]
STEP_API_CASES = CASES[:2]


def fed_back_steps(c):
    """the steps s of a chunk whose input is an output of the same chunk (not the carried frame, not the teacher)"""
    return [c["W"] + t - 1 for t in range(2, c["T"]) if not (c["teacher"] and t - 1 < c["n_pre"])]


def inputs(c):
    """float32 / uint8 / int64 CPU inputs of one case, keyed by its seed"""
    C, T, W, B, D, H = (c[k] for k in ("C", "T", "W", "B", "D", "H"))
    sd = R.inputs(2, 1, D, H, 0.0, c["seed"], training=False)["sd"]          # weights + running statistics off their initial values
    g = torch.Generator().manual_seed(c["seed"] + 5000)
    S = W + T - 1
    inp = dict(c)
    inp["sd"] = sd
    if c["ids"] == "none":
        Rr, ids = B * C, None
    else:
        Rr = B * C + 3
        ids = torch.randint(0, Rr, (B, C), generator=g)
        if c["ids"] == "edge":
            flat = ids.view(-1)
            flat[0], flat[1], flat[-1] = 0, Rr - 1, Rr - 1                       # rows 0 and R - 1, and R - 1 twice
            assert B * C >= 3
    inp["R"], inp["ids"] = Rr, ids
    inp["rows"] = torch.randn(Rr, 2 * H, generator=g) * 0.5
    inp["start_t"] = torch.randn(B, D, generator=g) if c["start"] else None
    inp["teacher_t"] = torch.randn(B, C, T, D, generator=g) if c["teacher"] else None
    k = (torch.rand(C, S, B, D, generator=g) < KEEP_PROB).to(torch.uint8)
    inp["keep95"] = k
    # a condition of the test, from the inputs alone: the carry and the feedback reach the arithmetic for every clip
    kept = k.sum(3) > 0                                                          # (C, S, B)
    assert bool(kept[:, 0].all()), f"{c['id']}: the first step of some chunk drops every column of some clip"
    fb = fed_back_steps(c)
    if fb:
        assert bool(kept[:, fb].any(1).all()), f"{c['id']}: no fed-back step of some chunk keeps a column for some clip"
    else:      # T too short for a fed-back step inside a chunk: the carry into the next chunk is the feedback
        assert C >= 2 and T - 1 >= (c["n_pre"] if c["teacher"] else 1), f"{c['id']}: nothing is ever fed back"
    return inp


def _weights(sd, dtype):
    return {k: sd[R.PRE + k].to(dtype) for k in R.PARAMS}, sd[R.PRE + "pre_linear.1.running_mean"].to(dtype), \
        sd[R.PRE + "pre_linear.1.running_var"].to(dtype)


def step(x, h0, h1, keep, w, rm, rv, conditioned):
    """BahdanauAttnDecoderRNN.forward in eval mode, the arithmetic of tests/_dec_ref.py's rollout(training=False) -> (y, h0, h1)"""
    xin = keep * x * 20.0 if conditioned else torch.zeros_like(x)
    u = xin @ w["pre_linear.0.weight"].t() + w["pre_linear.0.bias"]
    a = torch.relu((u - rm) / torch.sqrt(rv + R.EPS) * w["pre_linear.1.weight"] + w["pre_linear.1.bias"])
    h0, _ = R._cell(a, h0, w["gru.weight_ih_l0"], w["gru.weight_hh_l0"], w["gru.bias_ih_l0"], w["gru.bias_hh_l0"], [])
    h1, _ = R._cell(h0, h1, w["gru.weight_ih_l1"], w["gru.weight_hh_l1"], w["gru.bias_ih_l1"], w["gru.bias_hh_l1"], [])
    return h1 @ w["out_layer.weight"].t() + w["out_layer.bias"], h0, h1


def chain(inp, dtype, clips=None):
    """-> {"out": (B, C T, D), "h_last": (2, B, H)} in `dtype`; clips: a slice of the batch to decode alone"""
    C, T, W, B, D, H = (inp[k] for k in ("C", "T", "W", "B", "D", "H"))
    sl = slice(0, B) if clips is None else clips
    w, rm, rv = _weights(inp["sd"], dtype)
    rows = inp["rows"].to(dtype)
    ids = inp["ids"][sl] if inp["ids"] is not None else torch.arange(B * C).view(B, C)[sl]
    nb = ids.shape[0]
    k95 = inp["keep95"][:, :, sl].to(dtype)
    teacher = None if inp["teacher_t"] is None else inp["teacher_t"][sl].to(dtype)
    carry = torch.zeros(nb, D, dtype=dtype) if inp["start_t"] is None else inp["start_t"][sl].to(dtype)
    out = torch.zeros(nb, C, T, D, dtype=dtype)
    h0 = h1 = None
    for c in range(C):
        h = rows[ids[:, c]]
        h0, h1 = h[:, :H], h[:, H:]
        x = carry
        out[:, c, 0] = x
        for s in range(W):
            _, h0, h1 = step(x, h0, h1, k95[c, s], w, rm, rv, inp["conditioned"])
        for t in range(1, T):
            y, h0, h1 = step(x, h0, h1, k95[c, W + t - 1], w, rm, rv, inp["conditioned"])
            out[:, c, t] = y
            x = teacher[:, c, t] if (teacher is not None and t < inp["n_pre"]) else y
        carry = x if inp["conditioned"] else torch.zeros_like(x)
    return {"out": out.view(nb, C * T, D), "h_last": torch.stack([h0, h1])}


def by_step(out):
    """(B, F, D) -> (F, B, D): step_err's time axis first"""
    return torch.as_tensor(out).detach().cpu().transpose(0, 1)


@functools.lru_cache(maxsize=None)
def _reference(cid):
    c = next(k for k in CASES if k["id"] == cid)
    inp = inputs(c)
    f64, f32 = chain(inp, torch.float64), chain(inp, torch.float32)
    e32 = {"out": R.step_err(by_step(f32["out"]), by_step(f64["out"]), "y"), "h_last": R.step_err(f32["h_last"], f64["h_last"], "h_last")}
    return {"inp": inp, "f64": f64, "e32": e32}


def reference(c):
    """inputs, the float64 chain and e32 per frame of one case; computed once and shared, never modified"""
    return _reference(c["id"])


def check(label, name, got, ref, e32):
    """tests/_dec_ref.py's check on `out` (per chunk and step) or `h_last` under the forward cap -> (ok, line, ratio)"""
    got, ref = (by_step(got), by_step(ref)) if name == "out" else (got, ref)
    ek, bd = R.step_err(got, ref, "y" if name == "out" else name), R.bound(e32, CAP)
    k = int(torch.argmax(ek / bd))
    ratio = float(ek[k] / max(float(e32[k]), 2 * U))
    line = (f"{label} {name}: frame {k} of {len(ek)}  e_kernel {float(ek[k]):.3e}  e32 {float(e32[k]):.3e}  ratio {ratio:.2f}  "
            f"bound {float(bd[k]):.3e}")
    print(line)
    return bool((ek <= bd).all()), line, ratio


# ---------------------------------------------------------------------------------------------------------------- the clip's tail
def savgol_table(window=SAVGOL_WINDOW, order=SAVGOL_ORDER):
    """float64: `window` interior taps, then the two (window // 2, window) edge matrices (first frames, last frames) of
    scipy.signal.savgol_filter(mode="interp"): rows of the least-squares projection onto polynomials over the window"""
    half = window // 2
    A = np.vander(np.arange(window, dtype=np.float64) - half, order + 1, increasing=True)
    P = A @ np.linalg.pinv(A)
    return np.concatenate([P[half], P[:half].reshape(-1), P[window - half:].reshape(-1)])


def blend_inplace(r, T, n=10):
    """the reference's loop (inference_Autoencoder.py:388-395, its 30 as T) on one clip (F, Dr), in place, in r's dtype"""
    r = r.clone()
    for offset in range(T, len(r), T):
        for index in range(n):
            prev, nxt = r[offset - index].clone(), r[offset + index].clone()
            r[offset + index] = prev * (n - index) / (n + 1) + nxt * (index + 1) / (n + 1)
    return r


def clip_finish(r, mean, std, T, n, table, dtype):
    """g2v_clip_finish on (B, F, Dr): blend from the un-blended frames, * clip(std, 0.01) + mean (None: not), filter (table None: not)"""
    r = r.to(dtype)
    B, F, Dr = r.shape
    out = r.clone()
    for o in range(T, F, T):
        for i in range(n):
            out[:, o + i] = r[:, o - i] * (n - i) / (n + 1) + r[:, o + i] * (i + 1) / (n + 1)
    if std is not None:
        out = out * torch.clamp(std.to(dtype), min=0.01) + mean.to(dtype)
    if table is None:
        return out
    W_, half = SAVGOL_WINDOW, SAVGOL_WINDOW // 2
    tb = torch.as_tensor(table).to(dtype)
    taps, first, last = tb[:W_], tb[W_:W_ + half * W_].view(half, W_), tb[W_ + half * W_:].view(half, W_)
    res = torch.empty_like(out)
    res[:, half:F - half] = torch.einsum("bfdk,k->bfd", out.unfold(1, W_, 1), taps)
    res[:, :half] = torch.einsum("jk,bkd->bjd", first, out[:, :W_])
    res[:, F - half:] = torch.einsum("jk,bkd->bjd", last, out[:, F - W_:])
    return res


FINISH_SHAPES = [(2, 3, 20, 135), (1, 2, 19, 7)]          # (B, C, T, Dr)
FINISH_MODES = ["blend", "blend+unnorm", "blend+unnorm+savgol"]


def finish_inputs(B, C, T, Dr, seed=31):
    g = torch.Generator().manual_seed(seed + B + 10 * C + 100 * T)
    r = torch.randn(B, C * T, Dr, generator=g)
    mean, std = torch.randn(Dr, generator=g), torch.rand(Dr, generator=g) + 0.1
    std[Dr // 2] = 0.004                                      # below the clip at 0.01
    return r, mean, std
