#!/usr/bin/env python
"""Writes tests/golden/kmeans.npz: sklearn's own fits of the seeded inputs of tests/_kmeans_inputs.py, and the recorded k-means++ picks.

    python tests/golden/make_fixtures_kmeans.py          (needs scikit-learn; the tests do not)

Per case of _kmeans_inputs.CASES: sklearn.cluster.KMeans(n_clusters=K, init=init, n_init=1, max_iter=2500, tol=1e-4,
algorithm="lloyd").fit(X) -> labels, inertia, n_iter_, the centres (whole for the small case; otherwise their float64 Frobenius norm
and every 7th element), sha256 of X and init.  Asserted here, so that the tests may demand equality on EVERY row:
  * the float64 restatement (tests/_kmeans_ref.py) reproduces sklearn: no label differs, equal n_iter_, centres within 1e-6;
  * the smallest relative top-2 distance gap over the whole trajectory exceeds 1e-5 (the fp32 assignment kernel's distance error is
    2 * 2^-20 of |x|^2 + |c|^2 at the most: no device rounding can turn the trajectory), and no cluster is ever empty.
The k-means++ record (PP_CASE): the rows tests/_kmeans_ref.kmeans_pp picks with numpy.random.RandomState(seed); asserted: every search
target is further than 1e-6 (relative to the potential) from the cumulative sum it is searched in, and every best candidate's
potential is more than 1e-6 (relative) below the runner-up's."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _kmeans_inputs as KI  # noqa: E402
import _kmeans_ref as KR  # noqa: E402

STRIDE = 7


def main():
    import sklearn
    from sklearn.cluster import KMeans
    out = {"sklearn_version": np.array(sklearn.__version__), "numpy_version": np.array(np.__version__), "stride": np.int64(STRIDE)}
    for name, (N, E, K, seed) in KI.CASES.items():
        X, init = KI.make(N, E, K, seed)
        sk = KMeans(n_clusters=K, init=init, n_init=1, max_iter=2500, tol=1e-4, algorithm="lloyd").fit(X)
        ref = KR.lloyd(X, init, track_gap=True)
        mism = int((ref["labels"] != sk.labels_).sum())
        cerr = float(np.abs(ref["centers"].astype(np.float64) - sk.cluster_centers_).max())
        print(f"{name}: N={N} E={E} K={K} seed={seed} n_iter sklearn {sk.n_iter_} restatement {ref['n_iter']}, label mismatches {mism}, "
              f"centres within {cerr:.2e}, smallest gap {ref['min_gap']:.2e}, relocated {ref['relocated']}, inertia {sk.inertia_:.6f} "
              f"vs {ref['inertia']:.6f}")
        assert mism == 0 and ref["n_iter"] == sk.n_iter_ and cerr <= 1e-6, "the restatement does not reproduce sklearn"
        assert ref["min_gap"] > 1e-5 and ref["relocated"] == 0, "pick the next seed: a near-tie or an empty cluster on the trajectory"
        assert len(np.unique(sk.labels_)) == K
        C = np.asarray(sk.cluster_centers_, np.float32)
        out[f"{name}_labels"] = sk.labels_.astype(np.int16)
        out[f"{name}_inertia"] = np.float64(sk.inertia_)
        out[f"{name}_n_iter"] = np.int64(sk.n_iter_)
        out[f"{name}_centers_norm"] = np.float64(np.sqrt((C.astype(np.float64) ** 2).sum()))
        out[f"{name}_centers"] = C if name == "small" else C.reshape(-1)[::STRIDE].copy()
        out[f"{name}_sha_x"] = np.array(KI.sha(X))
        out[f"{name}_sha_init"] = np.array(KI.sha(init))
    N, E, K, seed, rs_seed = KI.PP_CASE
    X, _ = KI.make(N, E, K, seed)
    pp = KR.kmeans_pp(X, K, np.random.RandomState(rs_seed))
    print(f"k-means++: rows {pp['rows']}, target separation {pp['target_sep']:.2e}, potential separation {pp['pot_sep']:.2e}")
    assert pp["target_sep"] > 1e-6 and pp["pot_sep"] > 1e-6, "pick another RandomState seed"
    out["pp_rows"] = np.asarray(pp["rows"], np.int64)
    out["pp_sha_x"] = np.array(KI.sha(X))
    out["pp_random_rows"] = np.random.RandomState(rs_seed).permutation(N)[:K].astype(np.int64)
    path = os.path.join(HERE, "kmeans.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
