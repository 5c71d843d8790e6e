"""This project's own numpy restatement of placing new rows into a fitted t-SNE map (csrc/tsne_place.hip): exact
neighbours among the fitted rows, their conditionals, the start, and the per-row descent against the fixed map.  float64 unless a
dtype is given (then the state and the pair arithmetic run in it, as `_tsne_ref.kl_grad` / `descend` do); nothing here imports
openTSNE or sklearn."""
import numpy as np

import _tsne_ref as TR

DEFAULTS = dict(perplexity=5.0, k=25, learning_rate=0.1, exaggeration=1.5, n_iter=250, momentum=0.8, max_grad_norm=0.25)


def k_aff(N, perplexity):
    return min(N - 1, int(3.0 * perplexity))


def sqdist(Z, X):
    """float64 squared Euclidean distances (M, N) of the rows of Z to the rows of X, from differences"""
    both = np.concatenate([np.asarray(X, np.float64), np.asarray(Z, np.float64)])
    return TR.sqdist(both, np.arange(len(X), len(both)))[:, :len(X)]


def neighbors(D, kk):
    """-> (idx (M, kk), d2 (M, kk)): the kk smallest of each row of D in ascending (d^2, index) order"""
    idx = np.argsort(D, axis=1, kind="stable")[:, :kk]
    return idx, np.take_along_axis(D, idx, 1)


def conditionals(d2, perplexity):
    """sklearn's bisection of the precision over the rows of d2 (M, k_aff), nothing left out -> p (M, k_aff) float64"""
    d2 = np.asarray(d2, np.float64)
    m = d2.shape[0]
    target = np.log(perplexity)
    beta, lo, hi = np.ones(m), np.full(m, -np.inf), np.full(m, np.inf)
    P = np.zeros_like(d2)
    live = np.arange(m)
    for _ in range(TR.N_STEPS):
        e = np.exp(-d2[live] * beta[live, None])
        s = e.sum(1)
        s[s == 0.0] = TR.ROW_FLOOR
        p = e / s[:, None]
        P[live] = p
        diff = np.log(s) + beta[live] * (d2[live] * p).sum(1) - target
        go = np.abs(diff) > TR.TOL
        live, diff = live[go], diff[go]
        if live.size == 0:
            break
        up = diff > 0.0
        b = beta[live]
        lo[live] = np.where(up, b, lo[live])
        hi[live] = np.where(up, hi[live], b)
        beta[live] = np.where(up, np.where(np.isinf(hi[live]), b * 2.0, (b + hi[live]) / 2.0),
                              np.where(np.isinf(lo[live]), b / 2.0, (b + lo[live]) / 2.0))
    return P


def start(Y, idx, p=None, mode="median", k_use=None):
    """the start (M, 2) fp32: numpy's fp32 median of Y over the first k_use neighbours, or sum p Y in float64 rounded once"""
    Y = np.asarray(Y, np.float32)
    if mode == "median":
        return np.median(Y[idx[:, :k_use]], axis=1).astype(np.float32)
    k_use = p.shape[1] if k_use is None else k_use
    return (np.asarray(p, np.float64)[:, :k_use, None] * Y[idx[:, :k_use]].astype(np.float64)).sum(1).astype(np.float32)


def kl_grad(Y, idx, p, y, exaggeration=1.0, dtype=np.float64):
    """-> (kl (M,), grad (M, 2), Z (M,)) of the placement objective at y, per row, evaluated in `dtype`:
    w_ij = 1 / (1 + |y_i - Y_j|^2), Z_i = sum_j w_ij over all N fitted points,
    grad_i = 2 [exaggeration sum_nbr p_ij w_ij (y_i - Y_j) - (1 / Z_i) sum_j w_ij^2 (y_i - Y_j)],
    kl_i = sum_nbr p_ij log(p_ij / (w_ij / Z_i)) at exaggeration 1 (a p of exactly 0 adds nothing)"""
    Y, y, p = np.asarray(Y, dtype), np.asarray(y, dtype), np.asarray(p, dtype)
    one = dtype(1.0)
    diff = y[:, None, :] - Y[None, :, :]
    w = one / (one + (diff * diff).sum(2))
    Z = w.sum(1, dtype=dtype)
    rep = ((w * w)[:, :, None] * diff).sum(1, dtype=dtype)
    dn = y[:, None, :] - Y[idx[:, :p.shape[1]]]
    wn = one / (one + (dn * dn).sum(2))
    att = ((p * wn)[:, :, None] * dn).sum(1, dtype=dtype)
    grad = dtype(2.0) * (dtype(exaggeration) * att - rep / Z[:, None])
    with np.errstate(divide="ignore", invalid="ignore"):
        terms = np.where(p > 0, p * np.log(np.where(p > 0, p, one) / (wn / Z[:, None])), dtype(0.0))
    return terms.sum(1, dtype=dtype), grad, Z


def step(y, velocity, gains, grad, momentum, lr, max_grad_norm):
    """one step in the arrays' dtype: clip by the norm, the gains rule of `_tsne_ref.update`, velocity, y"""
    dt = y.dtype.type
    g = grad.astype(y.dtype)
    n = np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1])
    if max_grad_norm > 0:
        with np.errstate(divide="ignore", invalid="ignore"):
            scale = np.where(n > dt(max_grad_norm), dt(max_grad_norm) / n, dt(1.0)).astype(y.dtype)
        g = np.where((n > dt(max_grad_norm))[:, None], g * scale[:, None], g)
    inc = velocity * g < 0.0
    gains = np.maximum(np.where(inc, gains + dt(0.2), gains * dt(0.8)), dt(0.01))
    velocity = dt(momentum) * velocity - dt(lr) * (g * gains)
    return y + velocity, velocity, gains


def descend(Y, idx, p, y0, n_iter=250, exaggeration=1.5, momentum=0.8, learning_rate=0.1, max_grad_norm=0.25, dtype=np.float64):
    """n_iter steps from y0 with velocity 0 and gains 1, then the closing sweep at exaggeration 1 -> (y, kl, grad, Z)"""
    y = np.asarray(y0, dtype).copy()
    vel, gains = np.zeros_like(y), np.ones_like(y)
    for _ in range(n_iter):
        _, g, _ = kl_grad(Y, idx, p, y, exaggeration, dtype)
        y, vel, gains = step(y, vel, gains, g, momentum, learning_rate, max_grad_norm)
    kl, g, Z = kl_grad(Y, idx, p, y, 1.0, dtype)
    return y, kl, g, Z


def place(X, Y, Z, perplexity=5.0, k=25, initialization="median", dtype=np.float64, **descent_kw):
    """steps 1-4 end to end -> dict(idx, d2, p, y0, y, kl, grad, Z)"""
    ka = k_aff(len(X), perplexity)
    idx, d2 = neighbors(sqdist(Z, X), max(ka, k))
    p = conditionals(d2[:, :ka], perplexity).astype(np.float32)
    y0 = start(Y, idx, p, initialization, k if initialization == "median" else ka)
    y, kl, g, Zs = descend(Y, idx, p, y0, dtype=dtype, **descent_kw)
    return dict(idx=idx, d2=d2, p=p, y0=y0, y=y, kl=kl, grad=g, Z=Zs)
