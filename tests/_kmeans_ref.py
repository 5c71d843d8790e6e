"""Float64 numpy restatement of what gesture2vec_amd/kmeans.py and kmeans.hip compute: Lloyd iterations with sklearn's two stop
rules and its empty-cluster relocation in a fixed order, and greedy k-means++ consuming given uniform draws.  Test code only."""
import numpy as np


def sq_dists(X, C):
    """(N,K) float64 |x - c|^2, formed directly (no expansion): the yardstick for argmin margins."""
    X, C = np.asarray(X, np.float64), np.asarray(C, np.float64)
    out = np.empty((X.shape[0], C.shape[0]))
    for k in range(C.shape[0]):
        d = X - C[k]
        out[:, k] = np.einsum("ne,ne->n", d, d)
    return out


def assign(X, C):
    """labels (lowest index on ties) and the relative top-2 gap (d2 - d1) / (|x|^2 + |c1|^2 + tiny) per row"""
    D = sq_dists(X, C)
    lab = D.argmin(axis=1)
    if C.shape[0] == 1:
        return lab, np.full(X.shape[0], np.inf)
    part = np.partition(D, 1, axis=1)
    x2 = np.einsum("ne,ne->n", np.asarray(X, np.float64), np.asarray(X, np.float64))
    c2 = np.einsum("ke,ke->k", np.asarray(C, np.float64), np.asarray(C, np.float64))[lab]
    return lab, (part[:, 1] - part[:, 0]) / (x2 + c2 + 1e-300)


def update(X, labels, C_old, prev=None, relocate=True):
    """One update step.  -> dict(counts, sums, centers (fp32: the float64 quotient rounded once), inertia, shift, n_changed,
    relocated_rows).  Labels outside [0, K) are ignored.  Relocation: the empty clusters in ascending id take the n_empty rows with
    the largest |x - c_old[label]|^2, farthest first, lowest row among equals; a cluster left without rows keeps its old centre."""
    X64, C64 = np.asarray(X, np.float64), np.asarray(C_old, np.float64)
    labels = np.asarray(labels, np.int64)
    N, E = X64.shape
    K = C64.shape[0]
    ok = (labels >= 0) & (labels < K)
    counts = np.bincount(labels[ok], minlength=K).astype(np.int64)
    sums = np.zeros((K, E))
    order = np.argsort(labels[ok], kind="stable")              # rows of a cluster in ascending row order
    starts = np.cumsum(counts) - counts
    if order.size:
        sums[counts > 0] = np.add.reduceat(X64[ok][order], starts[counts > 0], axis=0)
    d = X64[ok] - C64[labels[ok]]
    rowd = np.full(N, -1.0)
    rowd[ok] = np.einsum("ne,ne->n", d, d)
    inertia = float(rowd[ok].sum())
    rows = []
    if relocate:
        empty = np.flatnonzero(counts == 0)
        n_rel = min(len(empty), int(ok.sum()))
        order = np.lexsort((np.arange(N), -rowd))[:n_rel]          # farthest first, lowest row among equals
        for new_k, row in zip(empty[:n_rel], order):
            old_k = labels[row]
            sums[old_k] -= X64[row]
            counts[old_k] -= 1
            sums[new_k] = X64[row]
            counts[new_k] = 1
            rows.append(int(row))
    centers = np.asarray(C_old, np.float32).copy()
    has = counts > 0
    centers[has] = (sums[has] / counts[has, None]).astype(np.float32)
    diff = centers.astype(np.float64) - C64
    return {"counts": counts, "sums": sums, "centers": centers, "inertia": inertia, "shift": float((diff * diff).sum()),
            "n_changed": int(N if prev is None else (np.asarray(prev) != labels).sum()), "relocated_rows": rows}


def tolerance(X, tol):
    return float(tol * np.mean(np.var(np.asarray(X, np.float64), axis=0)))


def lloyd(X, init, max_iter=2500, tol=1e-4, track_gap=False):
    """sklearn's _kmeans_single_lloyd: assign, update, swap, stop when no label changed (strict) or shift <= tol * mean Var; after a
    stop by tol / max_iter the labels are those of the final centres.  The fp32 centres carry the trajectory, as on the device.
    track_gap: `min_gap` = the smallest relative top-2 gap any assignment of the loop saw, `min_pos_gap` = the same over the rows whose
    two nearest centres are not exactly equidistant (duplicated centres: the lower index wins everywhere)."""
    C = np.asarray(init, np.float32).copy()
    tol_abs = tolerance(X, tol)
    prev = np.full(X.shape[0], -1, np.int64)
    strict, n_iter, min_gap, min_pos_gap, relocated = False, 0, np.inf, np.inf, 0
    for it in range(max_iter):
        lab, gap = assign(X, C)
        if track_gap:
            min_gap = min(min_gap, float(gap.min()))
            min_pos_gap = min(min_pos_gap, float(gap[gap > 0].min()))
        u = update(X, lab, C, prev)
        relocated += len(u["relocated_rows"])
        C = u["centers"]
        n_iter = it + 1
        if u["n_changed"] == 0:
            strict = True
            break
        if u["shift"] <= tol_abs:
            break
        prev = lab
    if not strict:
        lab, gap = assign(X, C)
        if track_gap:
            min_gap = min(min_gap, float(gap.min()))
    inertia = update(X, lab, C, relocate=False)["inertia"]
    return {"centers": C, "labels": lab, "inertia": inertia, "n_iter": n_iter, "min_gap": min_gap, "min_pos_gap": min_pos_gap,
            "relocated": relocated}


def kmeans_pp(X, K, rs, max_trials=8):
    """sklearn's greedy _kmeans_plusplus on float64 distances, drawing from `rs` (numpy RandomState) in sklearn's order: one
    random_sample() for the first centre (row floor(u N)), uniform(size=min(2 + int(log K), max_trials)) per further centre;
    candidates = searchsorted(cumsum(closest), u * potential) clipped to N - 1.  -> rows, and per step the smallest relative
    distance of a search target to the cumulative sum (`target_sep`) and of the best potential to the runner-up (`pot_sep`)."""
    X64 = np.asarray(X, np.float64)
    N = X64.shape[0]
    trials = min(2 + int(np.log(K)), max_trials)
    first = min(int(rs.random_sample() * N), N - 1)
    rows = [first]
    closest = sq_dists(X64, X64[first:first + 1])[:, 0]
    pot = closest.sum()
    target_sep, pot_sep = np.inf, np.inf
    for _ in range(1, K):
        vals = rs.uniform(size=trials) * pot
        cum = np.cumsum(closest)
        cand = np.minimum(np.searchsorted(cum, vals), N - 1)
        target_sep = min(target_sep, float(np.abs(cum[None, :] - vals[:, None]).min() / pot))
        D = np.minimum(closest[None, :], sq_dists(X64, X64[cand]).T)
        pots = D.sum(axis=1)
        best = int(np.argmin(pots))
        others = np.delete(pots, np.flatnonzero(cand == cand[best]))
        if len(others):
            pot_sep = min(pot_sep, float((others.min() - pots[best]) / pots[best]))
        closest, pot = D[best], pots[best]
        rows.append(int(cand[best]))
    return {"rows": rows, "target_sep": target_sep, "pot_sep": pot_sep}
