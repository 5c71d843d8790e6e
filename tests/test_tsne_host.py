"""CPU-only checks of the t-SNE / PCA feature (gesture2vec_amd/embedding.py, csrc/tsne.hip): the numpy restatement the GPU tests
compare against (tests/_tsne_ref.py) is pinned to what sklearn 1.7 recorded in tests/golden/tsne.npz, and the public classes
validate their arguments, pickle without device state and refuse host tensors."""
import os
import pickle

import numpy as np
import pytest
import torch

import _tsne_inputs as TI
import _tsne_ref as TR


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "tsne.npz"))


@pytest.fixture(scope="module")
def base_P():
    return TR.joint(TI.base()[0], TI.PERPLEXITY)


def test_inputs_are_the_recorded_ones(fx):
    X, lab = TI.base()
    assert TI.sha(X) == str(fx["base_sha_x"]) and TI.sha(lab) == str(fx["base_sha_labels"])
    assert TI.sha(TI.small()[0]) == str(fx["small_sha_x"])
    assert X.shape == (720, 400) and np.array_equal(np.bincount(lab), np.full(6, 120))


def test_joint_matches_sklearn(fx, base_P):
    """sklearn rounds its squared distances to fp32 and the restatement does not: the recorded gaps (1.7e-8 of max P on 97 rows,
    5.6e-6 on 720) are reproduced, and nothing else separates the two"""
    from_condensed = np.zeros((TI.SMALL_N, TI.SMALL_N))
    from_condensed[np.triu_indices(TI.SMALL_N, 1)] = fx["small_P"]
    Psk = from_condensed + from_condensed.T
    P = TR.joint(TI.small()[0], TI.PERPLEXITY)
    gap = float(np.abs(P - Psk).max() / Psk.max())
    assert abs(gap - float(fx["gap_small"])) <= 1e-3 * float(fx["gap_small"]) and gap <= 1e-7
    assert np.array_equal(P, P.T) and not P.diagonal().any() and abs(P.sum() - 1.0) <= 1e-12
    rows = fx["base_P_rows"]
    gap = float(np.abs(base_P[rows] - fx["base_P"]).max() / base_P.max())
    assert gap <= 1.001 * float(fx["gap_base"]) <= 1e-5
    # with the distances rounded as sklearn rounds them, the restatement is sklearn's P to rounding
    C, _ = TR.conditionals(TR.sqdist(TI.small()[0]).astype(np.float32), TI.PERPLEXITY)
    S = C + C.T
    P32 = np.maximum(S / S.sum(), TR.EPS)
    np.fill_diagonal(P32, 0.0)
    assert float(np.abs(P32 - Psk).max() / Psk.max()) <= 1e-9


@pytest.mark.parametrize("yname", ["tiny", "spread"])
@pytest.mark.parametrize("ename,ex", [("x1", 1.0), ("x12", 12.0)])
def test_kl_and_gradient_match_sklearn(fx, base_P, yname, ename, ex):
    kl, g, Z = TR.kl_grad(base_P, fx[f"y_{yname}"], ex)
    ref = fx[f"grad_{yname}_{ename}"]
    assert abs(kl - float(fx[f"kl_{yname}_{ename}"])) <= 1e-10 * abs(kl)
    assert float(np.abs(g - ref).max()) <= 1e-10 * float(np.abs(ref).max()) and Z > 0.0
    rows = np.array([0, 7, 719])
    _, gr, _ = TR.kl_grad(base_P[rows], fx[f"y_{yname}"], ex, rows=rows, Z=Z)
    assert float(np.abs(gr - g[rows]).max()) <= 1e-12 * float(np.abs(ref).max())


def test_update_rule_is_sklearns():
    rng = np.random.default_rng(3)
    p, upd, grad = (rng.normal(size=(40, 2)).astype(np.float32) for _ in range(3))
    gains = (0.5 + rng.random((40, 2))).astype(np.float32)
    gains[0] = 0.011                                             # lands on the floor
    y, v, g, n2 = TR.update(p, upd, gains, grad, 0.8, 200.0)
    gains2, grad2 = gains.copy(), grad.copy()                    # sklearn's lines, verbatim
    inc = upd * grad2 < 0.0
    dec = np.invert(inc)
    gains2[inc] += 0.2
    gains2[dec] *= 0.8
    np.clip(gains2, 0.01, np.inf, out=gains2)
    grad2 *= gains2
    upd2 = 0.8 * upd - 200.0 * grad2
    assert np.array_equal(g, gains2) and np.array_equal(v, upd2) and np.array_equal(y, p + upd2)
    assert n2 == float((grad2.astype(np.float64) ** 2).sum()) and y.dtype == np.float32


def test_quality_measures_on_the_recorded_map(fx):
    X, lab = TI.base()
    assert TR.knn_accuracy(fx["y_spread"], lab, 5) == float(fx["run_f64_knn"]) == 1.0
    assert abs(TR.trustworthiness(X, fx["y_spread"], 5) - float(fx["run_f64_trust"])) <= 1e-4
    assert 0.0 < float(fx["run_kl_spread"]) < 0.05


def test_header_declares_the_kernels():
    from gesture2vec_amd import _lib
    for name in ("g2v_tsne_max_rows", "g2v_tsne_affinities_workspace", "g2v_tsne_affinities", "g2v_tsne_gradient_workspace",
                 "g2v_tsne_gradient", "g2v_tsne_update"):
        assert name in _lib.EXPORTS


def test_constructor_errors():
    from gesture2vec_amd.embedding import PCA, TSNE
    t = TSNE()
    assert (t.n_components, t.perplexity, t.early_exaggeration, t.learning_rate, t.max_iter, t.n_iter_without_progress,
            t.min_grad_norm, t.init, t.random_state) == (2, 30.0, 12.0, "auto", 1000, 300, 1e-7, "pca", None)
    for kw in (dict(n_components=3), dict(method="barnes_hut"), dict(perplexity=0.0), dict(early_exaggeration=0.5),
               dict(learning_rate="fast"), dict(learning_rate=-1.0), dict(max_iter=100), dict(init="spectral")):
        with pytest.raises(ValueError):
            TSNE(**kw)
    with pytest.raises(ValueError):
        PCA(0)


def test_no_cpu_fallback():
    from gesture2vec_amd.embedding import PCA, TSNE, latent_map
    x = torch.zeros(64, 8)
    for call in (lambda: TSNE().fit(x), lambda: TSNE().fit_transform(x), lambda: PCA(2).fit(x), lambda: PCA(2).update(x),
                 lambda: latent_map(x)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_pickles_without_device_state():
    from gesture2vec_amd.embedding import PCA, TSNE
    p = PCA(3)
    p.mean_, p.components_ = np.arange(4.0), np.eye(3, 4)
    p.explained_variance_, p.explained_variance_ratio_, p.n_samples_ = np.ones(3), np.full(3, 0.25), 10
    p._dev = {"cuda:0": object()}
    p._mom = object()
    q = pickle.loads(pickle.dumps(p))
    assert q._dev == {} and q._mom is None and q.n_components == 3 and q.n_samples_ == 10
    assert np.array_equal(q.components_, p.components_) and np.array_equal(q.mean_, p.mean_)
    t = TSNE(perplexity=7.0, init=np.zeros((5, 2)), random_state=4)
    t.embedding_, t.kl_divergence_, t.n_iter_ = torch.ones(5, 2), 1.25, 999
    u = pickle.loads(pickle.dumps(t))
    assert u.perplexity == 7.0 and u.kl_divergence_ == 1.25 and u.n_iter_ == 999 and not u.embedding_.is_cuda
    assert torch.equal(u.embedding_, t.embedding_)


def test_embedding_maps_flag_and_skip(tmp_path):
    """train_autoencoder_VQVAE.py --embedding-maps: off by default; a net without a quantiser is skipped, as the reference's try does"""
    import sys
    from types import SimpleNamespace
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "scripts"))
    import train_autoencoder_VQVAE as T
    from config.parse_args import parse_args
    cfg = ["-c", os.path.join(root, "config", "VQ-VAE_synthetic.yml"), "--synthetic"]
    assert parse_args(cfg).embedding_maps is False and parse_args(cfg + ["--embedding-maps"]).embedding_maps is True
    T.write_embedding_map(SimpleNamespace(model_save_path=str(tmp_path)), SimpleNamespace(vq=False, vq_layer=None), 4)
    assert not os.path.exists(tmp_path / "plots")
