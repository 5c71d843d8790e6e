#!/usr/bin/env python
"""Writes tests/golden/dbscan.npz: sklearn.cluster.DBSCAN's own labels and core indices of five inputs, with the rows themselves.

    python tests/golden/make_fixtures_dbscan.py          (needs scikit-learn; the tests do not)

Per input of _dbscan_inputs.FIXTURES: `<name>_x` fp32 (N, E), `<name>_eps`, `<name>_min_samples`, `<name>_labels` int16 (N) =
DBSCAN(eps, min_samples).fit(x).labels_, `<name>_core` int32 = core_sample_indices_; `contested_between` = the contested row.
Blob inputs are drawn with the first seed from `seed0` on that meets every condition below; the other two are fixed.

Conditions, asserted here and again by tests/test_dbscan_host.py:
  * no pair's float64 distance lies within a relative 1e-4 of eps (then sklearn's own rounding decides no pair differently);
  * at least two clusters and at least one noise row per blob input;
  * in `contested`, a row that is not core lies within eps of core rows of two clusters;
  * the float64 rule of tests/_dbscan_ref.py reproduces sklearn's labels and core indices on every row."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _dbscan_inputs as DI  # noqa: E402
import _dbscan_ref as DR  # noqa: E402

BLOBS = {"blobs_193x37": (193, 37, 100), "blobs_257x3": (257, 3, 200), "blobs_300x400": (300, 400, 300)}      # N, E, seed0


def draw_blobs(N, E, seed0):
    for seed in range(seed0, seed0 + 100):
        X, eps, ms = DI.blobs(N, E, seed)
        ref = DR.fit(X, eps, ms)
        if DR.closest_to_eps(X, eps) > DI.REL_GAP and ref["labels"].max() >= 1 and (ref["labels"] < 0).any():
            return X, eps, ms, seed
    raise SystemExit(f"no seed in {seed0} .. {seed0 + 99} meets the conditions at ({N}, {E})")


def main():
    import sklearn
    from sklearn.cluster import DBSCAN
    out = {"sklearn_version": np.array(sklearn.__version__), "numpy_version": np.array(np.__version__)}
    for name in DI.FIXTURES:
        if name in BLOBS:
            X, eps, ms, seed = draw_blobs(*BLOBS[name])
            note = f"seed {seed}"
        elif name == "chains":
            X, eps, ms = DI.chains()
            note = "fixed"
        else:
            X, eps, ms, between = DI.contested()
            out["contested_between"] = np.int64(between)
            note = f"the row between is {between}"
        sk = DBSCAN(eps=eps, min_samples=ms).fit(X)
        labels, core = np.asarray(sk.labels_, np.int64), np.asarray(sk.core_sample_indices_, np.int64)
        gap = DR.closest_to_eps(X, eps)
        ref = DR.fit(X, eps, ms)
        print(f"{name}: {X.shape}, eps {eps}, min_samples {ms}, {note}: {labels.max() + 1} clusters, {len(core)} core, "
              f"{int((labels < 0).sum())} noise, closest pair to eps {gap:.2e} (relative), {ref['rounds']} rounds")
        assert gap > DI.REL_GAP, "a pair lies within 1e-4 of eps"
        assert np.array_equal(ref["labels"], labels) and np.array_equal(np.nonzero(ref["core"])[0], core), \
            "the rule does not reproduce sklearn"
        if name in BLOBS:
            assert labels.max() >= 1 and (labels < 0).any()
        if name == "contested":
            adj = DR.adjacency(X, eps)[between]
            assert not ref["core"][between] and len(set(labels[adj & ref["core"]])) == 2
            assert labels[between] == labels[adj & ref["core"]].min()
        out[f"{name}_x"] = X
        out[f"{name}_eps"] = np.float64(eps)
        out[f"{name}_min_samples"] = np.int64(ms)
        out[f"{name}_labels"] = labels.astype(np.int16)
        out[f"{name}_core"] = core.astype(np.int32)
    path = os.path.join(HERE, "dbscan.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
