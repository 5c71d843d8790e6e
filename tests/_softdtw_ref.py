"""The numpy restatement of the soft-DTW block of include/g2v.h, vectorised over pairs (the loops run over cells): the cost, the
forward tile R, the backward tile E, value and gradient of a barycentre objective, the barycentre (scipy's L-BFGS-B, the call the
header names) and the k-means loop of gesture2vec_amd/timeseries.SoftDTWKMeans.  `dtype` is float64 or np.longdouble.  Not
tslearn: the definitions are tslearn's as read from its source.  The first index i is the centre's (S), the second j the series' (T)."""
import numpy as np
from scipy.optimize import minimize

import _dtw_ref as DR

EPS = 2.0 ** -52


def cost_tiles(z, x, dtype=np.float64):
    """z (P, S, F), x (P, T, F) -> (P, S, T): sum_f (z_if - x_jf)^2 from the differences"""
    if dtype == np.float64:
        return DR.cost_tiles(np.asarray(z, dtype=np.float64), np.asarray(x, dtype=np.float64))
    z, x = np.asarray(z, dtype=dtype), np.asarray(x, dtype=dtype)
    out = np.zeros((z.shape[0], z.shape[1], x.shape[1]), dtype=dtype)
    for f in range(z.shape[2]):
        d = z[:, :, None, f] - x[:, None, :, f]
        out += d * d
    return out


def softmin(a, b, c, gamma):
    """the header's softmin; an absent predecessor is +inf and contributes exp(-inf) = 0.  At least one of a, b, c is finite."""
    ap, bp, cp = -a / gamma, -b / gamma, -c / gamma
    m = np.maximum(ap, np.maximum(bp, cp))
    return -gamma * (np.log(np.exp(ap - m) + np.exp(bp - m) + np.exp(cp - m)) + m)


def forward(cost, gamma):
    """(P, S, T) costs -> (P, S, T) R; R[:, -1, -1] is the soft-DTW value"""
    P, S, T = cost.shape
    gamma = cost.dtype.type(gamma)
    R = np.full((P, S + 1, T + 1), np.inf, dtype=cost.dtype)
    for i in range(S):
        for j in range(T):
            if i == 0 and j == 0:
                R[:, 1, 1] = cost[:, 0, 0]
            else:
                R[:, i + 1, j + 1] = cost[:, i, j] + softmin(R[:, i, j + 1], R[:, i, j], R[:, i + 1, j], gamma)
    return R[:, 1:, 1:]


def backward(cost, R, gamma):
    """-> (P, S, T) E, the header's backward recursion"""
    P, S, T = cost.shape
    gamma = cost.dtype.type(gamma)
    E = np.zeros((P, S + 1, T + 1), dtype=cost.dtype)
    for i in range(S - 1, -1, -1):
        for j in range(T - 1, -1, -1):
            if i == S - 1 and j == T - 1:
                E[:, i, j] = 1
                continue
            e = np.zeros(P, dtype=cost.dtype)
            if i + 1 < S:
                e = E[:, i + 1, j] * np.exp((R[:, i + 1, j] - R[:, i, j] - cost[:, i + 1, j]) / gamma)
            if j + 1 < T:
                e = e + E[:, i, j + 1] * np.exp((R[:, i, j + 1] - R[:, i, j] - cost[:, i, j + 1]) / gamma)
            if i + 1 < S and j + 1 < T:
                e = e + E[:, i + 1, j + 1] * np.exp((R[:, i + 1, j + 1] - R[:, i, j] - cost[:, i + 1, j + 1]) / gamma)
            E[:, i, j] = e
    return E[:, :S, :T]


def pair_costs(x, y, dtype=np.float64):
    """every series of x (N, T, F) against every centre of y (M, S, F) -> (N M, S, T), pair n M + m; blocks of series on
    _dtw_ref's threads (the sums of one block do not depend on the cut)"""
    N, M = x.shape[0], y.shape[0]
    rows = max(1, -(-N // DR._THREADS))
    cuts = list(range(0, N, rows)) + [N]
    block = lambda c: cost_tiles(np.tile(y, (c[1] - c[0], 1, 1)), np.repeat(x[c[0]:c[1]], M, axis=0), dtype)      # noqa: E731
    return np.concatenate(list(DR._POOL.map(block, zip(cuts[:-1], cuts[1:]))), axis=0)


def tiles(x, y, gamma, dtype=np.float64):
    """-> R (N, M, S, T)"""
    x, y = np.asarray(x), np.asarray(y)
    R = forward(pair_costs(x, y, dtype), gamma)
    return R.reshape(x.shape[0], y.shape[0], R.shape[1], R.shape[2])


def cdist(x, y, gamma, dtype=np.float64):
    """-> (values (N, M), max |R| over each pair's tile (N, M): the scale of the value's tolerance)"""
    R = tiles(x, y, gamma, dtype)
    return R[:, :, -1, -1], np.abs(R).max(axis=(2, 3))


def alignment(x, z, gamma, dtype=np.float64):
    """rows x (P, T, F) against one centre z (S, F) -> dict cost, R, E (P, S, T), value (P)"""
    x = np.asarray(x)
    cost = cost_tiles(np.broadcast_to(np.asarray(z), (x.shape[0],) + np.shape(z)), x, dtype)
    R = forward(cost, gamma)
    return {"cost": cost, "R": R, "E": backward(cost, R, gamma), "value": R[:, -1, -1]}


def tol_R(T, S, maxR, gamma):
    """eight roundings per cell, each at most an ulp of max(|R|, gamma), along T + S diagonals"""
    return 8 * (T + S) * EPS * np.maximum(maxR, gamma)


def tol_E(T, S, maxR, gamma):
    return 2 * (T + S) * tol_R(T, S, maxR, gamma) / gamma


def objective(x, z, gamma, weights=None, dtype=np.float64):
    """value and gradient of obj(z) = sum_n w_n sdtw(z, x_n) over the rows x (P, T, F) -> dict value, grad (S, F), and the two scales
    of the gradient's tolerance: lever (S, F) = sum_n w_n sum_j 2 |z_if - x_njf| (what an error of E is multiplied with) and terms
    (S, F) = the sum of the absolute values of the gradient's terms; maxR = max |R| over all tiles"""
    x = np.asarray(x).astype(dtype)
    z = np.asarray(z).astype(dtype)
    w = np.ones(x.shape[0], dtype=dtype) if weights is None else np.asarray(weights).astype(dtype)
    a = alignment(x, z, gamma, dtype)
    wE = a["E"] * w[:, None, None]
    rows = wE.sum(axis=(0, 2))
    grad = 2 * (z * rows[:, None] - np.einsum("pst,ptf->sf", wE, x))
    lever = 2 * (np.abs(z[None, :, None, :] - x[:, None, :, :]) * w[:, None, None, None]).sum(axis=(0, 2))
    terms = 2 * (np.abs(z) * np.abs(wE).sum(axis=(0, 2))[:, None] + np.einsum("pst,ptf->sf", np.abs(wE), np.abs(x)))
    return {"value": (w * a["value"]).sum(), "grad": grad, "lever": lever, "terms": terms, "maxR": float(np.abs(a["R"]).max()),
            "abs_value": float((np.abs(w) * np.abs(a["value"])).sum())}


def barycenter(x, gamma, weights=None, max_iter=50, tol=1e-3, init=None):
    """the header's softdtw_barycenter -> (z (S, F), function evaluations)"""
    x = np.asarray(x)
    if init is None:
        w = np.ones(x.shape[0]) if weights is None else np.asarray(weights, dtype=np.float64)
        init = (x.astype(np.float64) * w[:, None, None]).sum(axis=0) / w.sum()
    init = np.array(init, dtype=np.float64)
    if max_iter == 0:
        return init, 0

    def f(flat):
        o = objective(x, flat.reshape(init.shape), gamma, weights)
        return float(o["value"]), o["grad"].ravel()

    res = minimize(f, init.ravel(), method="L-BFGS-B", jac=True, tol=tol, options=dict(maxiter=max_iter, disp=False))
    return res.x.reshape(init.shape), int(res.nfev)


def centre_gap(v):
    """the smallest gap between the best and the second-best centre over the rows of v (N, M), relative to the larger magnitude"""
    if v.shape[1] < 2:
        return np.inf
    s = np.sort(v, axis=1)
    return float(np.min((s[:, 1] - s[:, 0]) / np.maximum(np.maximum(np.abs(s[:, 0]), np.abs(s[:, 1])), 1e-300)))


def fit(x, init, gamma, max_iter=5, max_iter_barycenter=5, tol=1e-6):
    """The loop of timeseries.SoftDTWKMeans from given init centres (K, S, F) -> dict centers, labels, inertia, n_iter, centre_gap,
    nfev (per iteration, per cluster), empty, maxR (the largest |R| of the last assignment's tiles)"""
    x = np.asarray(x)
    centers = np.array(init, dtype=np.float64)
    K = centers.shape[0]
    old, gap, nfev, empty, maxR = np.inf, np.inf, [], False, 0.0
    for it in range(max_iter):
        v, mr = cdist(x, centers, gamma)
        labels = np.argmin(v, axis=1)
        inertia = float(v[np.arange(len(labels)), labels].mean())
        gap, maxR = min(gap, centre_gap(v)), float(mr.max())
        if np.bincount(labels, minlength=K).min() == 0:
            empty = True
            break
        evals = np.zeros(K, dtype=np.int64)
        for k in range(K):
            centers[k], evals[k] = barycenter(x[labels == k], gamma, max_iter=max_iter_barycenter, init=centers[k])
        nfev.append(evals)
        if abs(old - inertia) < tol:
            break
        old = inertia
    return {"centers": centers, "labels": labels, "inertia": inertia, "n_iter": it + 1, "centre_gap": gap, "nfev": nfev,
            "empty": empty, "maxR": maxR}


# ---- the cases the host and the device tests share: built once per session ----------------------------------------------------------
import functools  # noqa: E402

import _dtw_inputs as DI  # noqa: E402

SHAPES_TS = [(1, 1), (1, 7), (7, 1), (2, 2), (15, 17), (16, 16), (17, 33), (34, 34), (63, 64), (64, 64)]
WIDTHS = [1, 3, 40, 135, 512]
SHAPES_NM = [(1, 1), (5, 3), (67, 41)]
GAMMAS = [0.5, 1.0, 0.01]
FIT_GAMMA = 0.5


def case_gamma(T, S, F):
    """every (T, S) meets every gamma, and so does every F: the three rotate over the grid"""
    return GAMMAS[(SHAPES_TS.index((T, S)) + WIDTHS.index(F)) % len(GAMMAS)]


def inputs(N, M, T, S, F, scale=None):
    """DI.random_pair scaled by 1 / sqrt(2 F) (costs of order one), or by `scale`; x stays fp32"""
    x, y = DI.random_pair(N, M, T, S, F, 100 * T + S + F)
    k = 1.0 / np.sqrt(2.0 * F) if scale is None else scale
    return (x * np.float32(k)).astype(np.float32), y * k


@functools.lru_cache(maxsize=None)
def cdist_case(T, S, F):
    """-> (x, y, gamma, values (N, M), max|R| (N, M)) at the largest (N, M); the smaller ones are its leading blocks"""
    N, M = SHAPES_NM[-1]
    x, y = inputs(N, M, T, S, F)
    g = case_gamma(T, S, F)
    return (x, y, g) + cdist(x, y, g)


@functools.lru_cache(maxsize=None)
def scaled_case():
    """the series scaled by 100 at gamma = 0.01: exponents down to -1e6"""
    x, y = inputs(67, 41, 17, 33, 40, scale=100.0)
    return (x, y, 0.01) + cdist(x, y, 0.01)


@functools.lru_cache(maxsize=None)
def fit_case(name):
    x, init, K = DI.planted(name)
    return fit(x, init, FIT_GAMMA, max_iter=5, max_iter_barycenter=5)
