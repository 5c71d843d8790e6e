#!/usr/bin/env python
"""Writes tests/golden/tsne.npz: what sklearn 1.7 computes on the seeded inputs of tests/_tsne_inputs.py.

    python tests/golden/make_fixtures_tsne.py          (needs scikit-learn and scipy; the tests do not)

* sklearn.decomposition.PCA(50, svd_solver="full") of the base case (720 x 400): mean, components, variances, the transform.
* sklearn.manifold._t_sne._joint_probabilities (perplexity 30) on the first 97 rows (the whole P) and on the base case (16 rows of
  P), with max |P - restatement| / max P for both and for every input of the GPU test's P cases (`gap_<case>`): sklearn rounds its
  squared distances to fp32, the restatement (tests/_tsne_ref.py) keeps float64, and that gap is what the GPU test's bound is 4 x of.
* sklearn's _kl_divergence (value and gradient) on the restatement's P of the base case at the fixed init (std 1e-4) and at the
  spread Y that sklearn's float64 run ends in, with and without exaggeration.
* kl_divergence_, trustworthiness and 5-NN label accuracy of full exact runs (sklearn's schedule driven through its own
  _gradient_descent and _kl_divergence from the fixed init) with float64 and with float32 parameters.
* sha256 of the inputs.
Asserted here: the restatement reproduces sklearn's _kl_divergence to 1e-12 and its trustworthiness exactly."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _tsne_inputs as TI  # noqa: E402
import _tsne_ref as TR  # noqa: E402

P_CASES = {"n97": (TI.SMALL_N, 400), "n1000": (1000, 400), "n1037": (1037, 48), "ld52": (300, 50)}     # rows(N, d) of the GPU test
P_ROWS_720 = np.arange(0, 720, 45)


def sk_joint(X, perplexity):
    from scipy.spatial.distance import squareform
    from sklearn.manifold import _t_sne as T
    from sklearn.metrics import pairwise_distances
    return squareform(T._joint_probabilities(pairwise_distances(X, metric="euclidean", squared=True), perplexity, 0))


def sk_run(Psk, y0, dtype, lr, max_iter=1000, exaggeration=12.0):
    """TSNE._tsne's two calls of _gradient_descent, on the condensed P"""
    from sklearn.manifold import _t_sne as T
    n = y0.shape[0]
    P = Psk.copy()
    args = dict(it=0, n_iter_check=50, min_grad_norm=1e-7, learning_rate=lr, verbose=0, kwargs={}, args=[P, 1, n, 2],
                n_iter_without_progress=250, max_iter=250, momentum=0.5)
    P *= exaggeration
    params, kl, it = T._gradient_descent(T._kl_divergence, y0.astype(dtype).ravel(), **args)
    P /= exaggeration
    args.update(max_iter=max_iter, it=it + 1, momentum=0.8, n_iter_without_progress=300)
    params, kl, it = T._gradient_descent(T._kl_divergence, params, **args)
    return params.reshape(n, 2), float(kl), it


def main():
    import sklearn
    from scipy.spatial.distance import squareform
    from sklearn.decomposition import PCA
    from sklearn.manifold import _t_sne as T, trustworthiness
    out = {"sklearn_version": np.array(sklearn.__version__), "numpy_version": np.array(np.__version__)}
    X, lab = TI.base()
    Xs, _ = TI.small()
    out["base_sha_x"], out["base_sha_labels"], out["small_sha_x"] = np.array(TI.sha(X)), np.array(TI.sha(lab)), np.array(TI.sha(Xs))

    pca = PCA(50, svd_solver="full").fit(X.astype(np.float64))
    out.update(pca_mean=pca.mean_, pca_components=pca.components_, pca_explained_variance=pca.explained_variance_,
               pca_explained_variance_ratio=pca.explained_variance_ratio_, pca_transform=pca.transform(X.astype(np.float64)))

    Psk_small, Psk = sk_joint(Xs, TI.PERPLEXITY), sk_joint(X, TI.PERPLEXITY)
    P_small, P = TR.joint(Xs, TI.PERPLEXITY), TR.joint(X, TI.PERPLEXITY)
    out.update(small_P=squareform(Psk_small, checks=False), base_P_rows=P_ROWS_720, base_P=Psk[P_ROWS_720],
               gap_small=np.float64(np.abs(P_small - Psk_small).max() / Psk_small.max()),
               gap_base=np.float64(np.abs(P - Psk).max() / Psk.max()))
    print(f"restatement vs sklearn's P: small {float(out['gap_small']):.2e}, base {float(out['gap_base']):.2e} of max P")
    for name, (N, d) in P_CASES.items():
        Xc = Xs if name == "n97" else TI.rows(N, d)
        Pr, Pk = (P_small, Psk_small) if name == "n97" else (TR.joint(Xc, TI.PERPLEXITY), sk_joint(Xc, TI.PERPLEXITY))
        out[f"gap_{name}"] = np.float64(np.abs(Pr - Pk).max() / Pk.max())
        out[f"sha_{name}"] = np.array(TI.sha(Xc))
        print(f"  {name}: N = {N}, d = {d}: gap {float(out[f'gap_{name}']):.2e}")

    y0 = TI.init_y(X.shape[0])
    lr = max(X.shape[0] / 12.0 / 4.0, 50.0)
    cond = squareform(Psk, checks=False)
    runs = {}
    for tag, dt in (("f64", np.float64), ("f32", np.float32)):
        Y, kl, it = sk_run(cond, y0, dt, lr)
        tw = float(trustworthiness(X, Y, n_neighbors=5))
        assert abs(tw - TR.trustworthiness(X, Y, 5)) <= 1e-12, "the restatement's trustworthiness is not sklearn's"
        runs[tag] = (Y, kl)
        out.update({f"run_{tag}_kl": np.float64(kl), f"run_{tag}_n_iter": np.int64(it), f"run_{tag}_trust": np.float64(tw),
                    f"run_{tag}_knn": np.float64(TR.knn_accuracy(Y, lab, 5))})
        print(f"sklearn exact run, {tag}: KL {kl:.6f} after {it + 1} iterations, trustworthiness {tw:.4f}, "
              f"5-NN accuracy {float(out[f'run_{tag}_knn']):.4f}")
    out["run_kl_spread"] = np.float64(abs(runs["f32"][1] - runs["f64"][1]) / runs["f64"][1])
    print(f"relative KL spread between the float64 and the float32 run: {float(out['run_kl_spread']):.2e}")

    spread = runs["f64"][0].astype(np.float32)
    out.update(y_tiny=y0, y_spread=spread)
    Pc = squareform(P, checks=False)
    for yname, Y in (("tiny", y0), ("spread", spread)):
        for ename, ex in (("x1", 1.0), ("x12", 12.0)):
            kl, g = T._kl_divergence(Y.astype(np.float64).ravel(), Pc * ex, 1, X.shape[0], 2)
            rkl, rg, _ = TR.kl_grad(P, Y, ex)
            err = max(abs(rkl - kl) / abs(kl), float(np.abs(rg.ravel() - g).max() / np.abs(g).max()))
            print(f"_kl_divergence at {yname} Y, exaggeration {ex}: KL {kl:.9f}, restatement within {err:.2e}")
            assert err <= 1e-12, "the restatement does not reproduce sklearn"
            out[f"kl_{yname}_{ename}"], out[f"grad_{yname}_{ename}"] = np.float64(kl), g.reshape(-1, 2)
    path = os.path.join(HERE, "tsne.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
