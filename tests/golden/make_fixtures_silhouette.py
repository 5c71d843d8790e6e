#!/usr/bin/env python
"""Writes tests/golden/silhouette.npz: sklearn's own silhouette coefficients of the seeded inputs of tests/_silhouette_inputs.py.

    python tests/golden/make_fixtures_silhouette.py          (needs scikit-learn and scipy; the tests do not)

Per case of _silhouette_inputs.CASES and per recorded label set: sklearn.metrics.silhouette_samples(D, labels, metric="precomputed") as
float64 with D = scipy.spatial.distance.cdist(X, X) in float64, the labels as int16, sha256 of X and of the labels; for
_silhouette_inputs.SAMPLE sklearn.metrics.silhouette_score(D, labels, metric="precomputed", sample_size, random_state).
Why precomputed distances: sklearn's own Euclidean path forms |x|^2 + |y|^2 - 2 x.y, in float64 for float64 rows, which leaves ~1e-7
on the distance of a bitwise duplicate pair and 1e-10 .. 1e-9 on the coefficients of these inputs (printed below for the record);
cdist sums (x - y)^2.  Asserted here: the numpy restatement (tests/_silhouette_ref.py) reproduces the recorded values to 1e-12."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _kmeans_inputs as KI  # noqa: E402
import _silhouette_inputs as SI  # noqa: E402
import _silhouette_ref as SR  # noqa: E402

RECORDED = {"shipped": ("nearest",), "small": ("nearest", "skewed"), "mid": ("nearest",)}


def main():
    import sklearn
    from scipy.spatial.distance import cdist
    from sklearn.metrics import silhouette_samples, silhouette_score
    out = {"sklearn_version": np.array(sklearn.__version__), "numpy_version": np.array(np.__version__)}
    for name in SI.CASES:
        X, sets, _ = SI.case(name)
        out[f"{name}_sha_x"] = np.array(KI.sha(X))
        X64 = X.astype(np.float64)
        Dsk = cdist(X64, X64)
        D = SR.distances(X)
        for which in RECORDED[name]:
            lab = sets[which]
            sk = np.asarray(silhouette_samples(Dsk, lab, metric="precomputed"), np.float64)
            ref = SR.terms(D, lab)[2]
            err = float(np.abs(sk - ref).max())
            gram = float(np.abs(np.asarray(silhouette_samples(X64, lab), np.float64) - sk).max())
            print(f"{name}/{which}: N={len(lab)} clusters {len(np.unique(lab))}, mean {sk.mean():.9f}, restatement within {err:.2e} "
                  f"(sklearn's Euclidean path: {gram:.2e})")
            assert err <= 1e-12, "the restatement does not reproduce sklearn"
            out[f"{name}_{which}_s"] = sk
            out[f"{name}_{which}_labels"] = lab.astype(np.int16)
            out[f"{name}_{which}_sha_labels"] = np.array(KI.sha(lab))
    name, seed, size = SI.SAMPLE
    X, sets, _ = SI.case(name)
    X64 = X.astype(np.float64)
    out["sample_score"] = np.float64(silhouette_score(cdist(X64, X64), sets["nearest"], metric="precomputed", sample_size=size,
                                                      random_state=seed))
    path = os.path.join(HERE, "silhouette.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
