#!/usr/bin/env python
"""Writes tests/golden/mapquality.npz: sklearn.manifold.trustworthiness of the generic inputs of _mapq_ref.SHAPES, both ways round,
with the inputs themselves.

    python tests/golden/make_fixtures_mapquality.py          (needs scikit-learn; the tests do not)

Per shape (N, d, k, c), under `<name>` = _mapq_ref.name_of(shape): `<name>_x` fp32 (N, d), `<name>_y` fp32 (N, c), `<name>_k`,
`<name>_seed`, `<name>_trust` = trustworthiness(x, y, n_neighbors=k) and `<name>_cont` = trustworthiness(y, x, n_neighbors=k),
float64.  `placed_x`, `placed_y`, `placed_z`, `placed_yz`, `placed_k`, `placed_seed`: a fitted set and M rows placed against it
(no sklearn value exists for those).  `exact_x`, `exact_y`: the integer grid of _mapq_ref.exact_grid (sklearn's unstable argsort
does not fix the order of its ties, so no sklearn value is recorded for it either).

Every generic input is drawn with the first seed from 0 on that meets both preconditions of _mapq_ref in both spaces, asserted
here and again by the tests, and (c) on which sklearn's fp32 distances order every compared pair as the float64 ones do:
  (a) selection_margin > 1: no row's k-th and (k + 1)-th neighbour are closer in d^2 than the selection's documented margin;
  (b) closest_compared > 1e-12: no two compared float64 distances of a row differ by less than the order of a sum can move them.
The restatement reproduces sklearn to 1e-12 on every one."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _mapq_ref as MR  # noqa: E402
from _tsne_ref import sqdist  # noqa: E402

MAX_SEEDS = 20000


def meets(X, Y, k):
    if not (MR.selection_margin(X, k) > 1.0 and MR.selection_margin(Y, k) > 1.0):
        return False
    me = np.arange(X.shape[0])
    DX, DY = sqdist(X), sqdist(Y)
    return (MR.closest_compared(DX, MR.nearest(DY, k, True), me) > MR.REL_SEP and
            MR.closest_compared(DY, MR.nearest(DX, k, True), me) > MR.REL_SEP)


def sklearn_agrees(X, Y, k):
    """(c) sklearn's own rounding swaps no rank: it keeps the distances of fp32 rows as fp32 (Gram form), which at some seeds puts
    two nearly equal distances in the other order and moves its number by one step of 2 / (N k (2 N - 3 k - 1))"""
    from sklearn.manifold import trustworthiness
    ref = MR.map_quality(X, Y, k)
    return (abs(ref["trustworthiness"] - float(trustworthiness(X, Y, n_neighbors=k))) <= 1e-12 and
            abs(ref["continuity"] - float(trustworthiness(Y, X, n_neighbors=k))) <= 1e-12)


def meets_placed(X, Y, Z, y, k):
    if not (MR.selection_margin(X, k, Z) > 1.0 and MR.selection_margin(Y, k, y) > 1.0):
        return False
    DX, DY = MR.cross_sqdist(Z, X), MR.cross_sqdist(y, Y)
    return (MR.closest_compared(DX, MR.nearest(DY, k, False)) > MR.REL_SEP and
            MR.closest_compared(DY, MR.nearest(DX, k, False)) > MR.REL_SEP)


def main():
    import sklearn
    from sklearn.manifold import trustworthiness
    out = {"sklearn_version": np.array(sklearn.__version__), "numpy_version": np.array(np.__version__)}
    for shape in MR.SHAPES:
        N, d, k, c = shape
        name = MR.name_of(shape)
        for seed in range(MAX_SEEDS):
            X, Y = MR.generic(N, d, c, seed)
            if meets(X, Y, k) and sklearn_agrees(X, Y, k):
                break
        else:
            raise SystemExit(f"no seed below {MAX_SEEDS} meets the preconditions at {shape}")
        ref = MR.map_quality(X, Y, k)
        trust, cont = float(trustworthiness(X, Y, n_neighbors=k)), float(trustworthiness(Y, X, n_neighbors=k))
        me = np.arange(N)
        bt, bc = MR.band_pairs(X, X, ref["nn_y"], me), MR.band_pairs(Y, Y, ref["nn_x"], me)
        print(f"{name}: seed {seed}, trustworthiness {trust:.6f}, continuity {cont:.6f}, rows without a penalty "
              f"{int((ref['penalty_t'] == 0).sum())} / {int((ref['penalty_c'] == 0).sum())}, pairs inside the band (sure, may) "
              f"{bt} / {bc}, margins {MR.selection_margin(X, k):.2f} / {MR.selection_margin(Y, k):.2f}")
        assert abs(ref["trustworthiness"] - trust) <= 1e-12 and abs(ref["continuity"] - cont) <= 1e-12, \
            f"the restatement does not reproduce sklearn ({ref['trustworthiness'] - trust:.3e}, {ref['continuity'] - cont:.3e})"
        out[f"{name}_x"], out[f"{name}_y"] = X, Y
        out[f"{name}_k"], out[f"{name}_seed"] = np.int64(k), np.int64(seed)
        out[f"{name}_trust"], out[f"{name}_cont"] = np.float64(trust), np.float64(cont)
    N, d, k, c, M = MR.PLACED
    for seed in range(MAX_SEEDS):
        X, Y, Z, y = MR.generic(N, d, c, seed, M)
        if meets(X, Y, k) and meets_placed(X, Y, Z, y, k):
            break
    else:
        raise SystemExit(f"no seed below {MAX_SEEDS} meets the preconditions at {MR.PLACED}")
    ref = MR.placement_quality(X, Y, Z, y, k)
    print(f"placed: seed {seed}, trustworthiness {ref['trustworthiness']:.6f}, continuity {ref['continuity']:.6f}")
    out.update(placed_x=X, placed_y=Y, placed_z=Z, placed_yz=y, placed_k=np.int64(k), placed_seed=np.int64(seed))
    X, Y = MR.exact_grid()
    assert MR.exact_in_fp32(X) and MR.exact_in_fp32(Y)
    ref = MR.map_quality(X, Y, MR.EXACT_K)
    print(f"exact: trustworthiness {ref['trustworthiness']:.6f}, continuity {ref['continuity']:.6f}")
    out.update(exact_x=X, exact_y=Y)
    path = os.path.join(HERE, "mapquality.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
