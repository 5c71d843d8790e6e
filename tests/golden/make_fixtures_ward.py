#!/usr/bin/env python
"""Writes tests/golden/ward.npz: sklearn.cluster.AgglomerativeClustering(linkage="ward")'s own tree and labels of five inputs, with
the rows themselves.

    python tests/golden/make_fixtures_ward.py          (needs scikit-learn; the tests do not)

Per input of _ward_inputs.FIXTURES: `<name>_x` fp32 (N, E), `<name>_children` int32 (N - 1, 2) = children_, `<name>_distances`
float64 (N - 1) = distances_, `<name>_ks` the three n_clusters of _ward_inputs.KS and `<name>_labels` int16 (3, N) = labels_ of a fit
at each.  `threshold_t`, `threshold_n_clusters`, `threshold_labels`: the fit of _ward_inputs.THRESHOLD_ON with distance_threshold = t,
the midpoint of two consecutive heights.  Every input is drawn with the first seed from `seed0` on that meets the conditions.

Conditions, asserted here and again by tests/test_ward_host.py:
  * in the float64 restatement of tests/_ward_ref.py, the runner-up of every row's nearest neighbour, in every round, lies more than
    1e-7 (relative) above the best;
  * consecutive sorted heights differ by more than 1e-7 relative;
  * the chain takes more than 8 rounds (check_every = 4 is outrun several times);
  * the restatement reproduces sklearn's children_ on every row, distances_ to 1e-12, and every label."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _ward_inputs as WI  # noqa: E402
import _ward_ref as WR  # noqa: E402

DRAW = {"blobs_193x37": (lambda s: WI.blobs(193, 37, s), 100), "blobs_257x3": (lambda s: WI.blobs(257, 3, s), 200),
        "blobs_300x400": (lambda s: WI.blobs(300, 400, s), 300), "chain": (lambda s: WI.chain(s), 0),
        "noise_65x3": (lambda s: WI.noise(65, 3, s), 400)}                                         # generator, seed0


def draw(name):
    gen, seed0 = DRAW[name]
    for seed in range(seed0, seed0 + 100):
        X = gen(seed)
        ref = WR.fit(X)
        if ref["nn_gap"] > WI.REL_GAP and ref["height_gap"] > WI.REL_GAP and (name != "chain" or ref["rounds"] > 8):
            return X, ref, seed
    raise SystemExit(f"no seed in {seed0} .. {seed0 + 99} meets the conditions for {name}")


def main():
    import sklearn
    from sklearn.cluster import AgglomerativeClustering
    out = {"sklearn_version": np.array(sklearn.__version__), "numpy_version": np.array(np.__version__)}
    for name in WI.FIXTURES:
        X, ref, seed = draw(name)
        N = len(X)
        sk = AgglomerativeClustering(n_clusters=WI.KS[name][0], linkage="ward", compute_full_tree=True, compute_distances=True).fit(X)
        children, dist = np.asarray(sk.children_, np.int64), np.asarray(sk.distances_, np.float64)
        err = float(np.max(np.abs(ref["distances"] - dist) / dist))
        print(f"{name}: {X.shape}, seed {seed}: {ref['rounds']} rounds, nn gap {ref['nn_gap']:.2e}, height gap {ref['height_gap']:.2e}, "
              f"sklearn's own height gap {WR.height_gap(dist):.2e}, heights off by {err:.1e} (relative)")
        assert np.array_equal(ref["children"], children), "the restatement does not reproduce sklearn's children_"
        assert err < 1e-12 and WR.height_gap(dist) > WI.REL_GAP
        labels = []
        for k in WI.KS[name]:
            lk = np.asarray(AgglomerativeClustering(n_clusters=k, linkage="ward").fit(X).labels_, np.int64)
            assert np.array_equal(WR.cut(k, children, N), lk), f"the cut restatement does not reproduce sklearn's labels at k = {k}"
            labels.append(lk)
        out[f"{name}_x"] = X
        out[f"{name}_children"] = children.astype(np.int32)
        out[f"{name}_distances"] = dist
        out[f"{name}_ks"] = np.array(WI.KS[name], dtype=np.int64)
        out[f"{name}_labels"] = np.stack(labels).astype(np.int16)
        if name == WI.THRESHOLD_ON:
            t = float(0.5 * (dist[-7] + dist[-6]))                # six heights lie above it: seven clusters
            th = AgglomerativeClustering(n_clusters=None, distance_threshold=t, linkage="ward").fit(X)
            assert th.n_clusters_ == 7 and np.array_equal(WR.cut(7, children, N), th.labels_)
            out["threshold_t"] = np.float64(t)
            out["threshold_n_clusters"] = np.int64(th.n_clusters_)
            out["threshold_labels"] = np.asarray(th.labels_, np.int16)
    path = os.path.join(HERE, "ward.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
