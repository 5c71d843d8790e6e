"""This project's own numpy restatement of exact t-SNE as sklearn 1.7 defines it (sklearn.manifold._t_sne, _utils.pyx): squared
distances, the per-row bisection of the precision, the joint P, KL divergence + gradient, the update rule, and the two quality
measures the tests use.  float64 unless a dtype is given; nothing here imports sklearn (tests/golden/make_fixtures_tsne.py checks
it against sklearn and records the results)."""
import numpy as np

EPS = float(np.finfo(np.float64).eps)           # sklearn's MACHINE_EPSILON
N_STEPS, TOL, ROW_FLOOR = 100, 1e-5, 1e-8


def sqdist(X, rows=None):
    """float64 squared Euclidean distances of `rows` (default: all) to every row, from differences; the pair (i, i) is exactly 0"""
    X = np.asarray(X, np.float64)
    rows = np.arange(X.shape[0]) if rows is None else np.asarray(rows)
    D = np.empty((len(rows), X.shape[0]))
    for a in range(0, len(rows), 16):
        diff = X[rows[a:a + 16], None, :] - X[None, :, :]
        D[a:a + 16] = np.einsum("ijk,ijk->ij", diff, diff)
    return D


def conditionals(D, perplexity, rows=None):
    """sklearn's _binary_search_perplexity over the distance rows D (m, N) of `rows` (default: m = N, all rows): beta = 1, doubled /
    halved while a bound is infinite, <= 100 steps, stop at |H - log(perplexity)| <= 1e-5, a row sum of 0 becomes 1e-8, j = i left
    out.  -> (C (m, N) with C[r, rows[r]] = 0, beta (m,))"""
    D = np.asarray(D, np.float64)
    m, N = D.shape
    rows = np.arange(m) if rows is None else np.asarray(rows)
    keep = np.ones((m, N), bool)
    keep[np.arange(m), rows] = False
    target = np.log(perplexity)
    beta, lo, hi = np.ones(m), np.full(m, -np.inf), np.full(m, np.inf)
    C = np.zeros((m, N))
    live = np.arange(m)
    for _ in range(N_STEPS):
        e = np.where(keep[live], np.exp(-D[live] * beta[live, None]), 0.0)
        s = e.sum(1)
        s[s == 0.0] = ROW_FLOOR
        p = e / s[:, None]
        C[live] = p
        diff = np.log(s) + beta[live] * (D[live] * p).sum(1) - target
        go = np.abs(diff) > TOL
        live, diff = live[go], diff[go]
        if live.size == 0:
            break
        up = diff > 0.0
        b = beta[live]
        lo[live] = np.where(up, b, lo[live])
        hi[live] = np.where(up, hi[live], b)
        beta[live] = np.where(up, np.where(np.isinf(hi[live]), b * 2.0, (b + hi[live]) / 2.0),
                              np.where(np.isinf(lo[live]), b / 2.0, (b + lo[live]) / 2.0))
    return C, beta


def joint(X, perplexity):
    """the dense joint P (N, N) float64: max((C + C^T) / sum(C + C^T), eps) off the diagonal, 0 on it"""
    C, _ = conditionals(sqdist(X), perplexity)
    S = C + C.T
    P = np.maximum(S / max(S.sum(), EPS), EPS)
    np.fill_diagonal(P, 0.0)
    return P


def kl_grad(P, Y, exaggeration=1.0, dtype=np.float64, rows=None, Z=None):
    """sklearn's _kl_divergence called with P * exaggeration, dense, evaluated in `dtype` -> (KL, grad (N, 2), Z).  With `rows`, P
    holds those rows only, Z must be given, the gradient rows are returned and KL is None."""
    Y = np.asarray(Y, dtype)
    P = np.asarray(P, dtype) * dtype(exaggeration)
    rows_ = np.arange(Y.shape[0]) if rows is None else np.asarray(rows)
    diff = Y[rows_, None, :] - Y[None, :, :]
    q = dtype(1.0) / (dtype(1.0) + (diff * diff).sum(2))
    q[np.arange(len(rows_)), rows_] = 0.0
    if rows is None:
        Z = q.sum(dtype=dtype)
    Q = np.maximum(q / dtype(Z), dtype(EPS))
    grad = dtype(4.0) * (((P - Q) * q)[:, :, None] * diff).sum(1)
    if rows is not None:
        return None, grad, Z
    off = ~np.eye(Y.shape[0], dtype=bool)
    kl = (P[off] * np.log(np.maximum(P[off], dtype(EPS)) / Q[off])).sum(dtype=dtype)
    return float(kl), grad, float(Z)


def update(y, velocity, gains, grad, momentum, lr):
    """sklearn's _gradient_descent step, in the arrays' dtype -> (y, velocity, gains, sum (gains grad)^2)"""
    dt = y.dtype.type
    inc = velocity * grad < 0.0
    gains = np.maximum(np.where(inc, gains + dt(0.2), gains * dt(0.8)), dt(0.01))
    g = grad * gains
    velocity = dt(momentum) * velocity - dt(lr) * g
    return y + velocity, velocity, gains, float((g.astype(np.float64) ** 2).sum())


def descend(P, y0, n_iter, exaggeration, momentum, lr, dtype=np.float64):
    """n_iter steps from y0 with fresh velocity and gains -> y"""
    y = np.asarray(y0, dtype).copy()
    vel, gains = np.zeros_like(y), np.ones_like(y)
    for _ in range(n_iter):
        _, g, _ = kl_grad(P, y, exaggeration, dtype)
        y, vel, gains, _ = update(y, vel, gains, g.astype(dtype), momentum, lr)
    return y


def knn_accuracy(Y, labels, k=5):
    """share of rows whose label is the majority label of their k nearest other rows in Y (lowest label on a tied vote)"""
    D = sqdist(Y)
    np.fill_diagonal(D, np.inf)
    nn = np.argsort(D, axis=1, kind="stable")[:, :k]
    votes = np.stack([np.bincount(labels[r], minlength=int(labels.max()) + 1) for r in nn])
    return float((votes.argmax(1) == labels).mean())


def trustworthiness(X, Y, k=5):
    """sklearn.manifold.trustworthiness(X, Y, n_neighbors=k), Euclidean"""
    n = X.shape[0]
    DX, DY = sqdist(X), sqdist(Y)
    np.fill_diagonal(DX, np.inf)
    np.fill_diagonal(DY, np.inf)
    order_x = np.argsort(DX, axis=1, kind="stable")
    rank_x = np.empty_like(order_x)
    rank_x[np.arange(n)[:, None], order_x] = np.arange(1, n + 1)[None, :]          # the nearest other row has rank 1, self rank n
    nn_y = np.argsort(DY, axis=1, kind="stable")[:, :k]
    r = rank_x[np.arange(n)[:, None], nn_y] - k
    return float(1.0 - 2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0)) * r[r > 0].sum())
