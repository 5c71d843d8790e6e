"""Host-side surface of placing new rows into a fitted t-SNE map (embedding.TSNE.transform, embedding.LatentMap) and the numpy
restatement the GPU tests compare against (tests/_tsne_place_ref.py, tests/_tsne_place_inputs.py).  No GPU."""
import pickle

import numpy as np
import pytest
import torch

import _tsne_place_inputs as PI
import _tsne_place_ref as PR


def _fitted(N=40, d=6):
    """a TSNE that holds host rows and a host map as if it had fitted them: enough for every check that comes before the kernels"""
    from gesture2vec_amd.embedding import TSNE
    t = TSNE()
    g = torch.Generator().manual_seed(0)
    t.fit_rows_, t.embedding_ = torch.randn(N, d, generator=g), torch.randn(N, 2, generator=g)
    return t


def test_transform_before_fit():
    from gesture2vec_amd.embedding import TSNE, LatentMap
    t = TSNE()
    assert t.fit_rows_ is None and t.transform_kl_ is None
    with pytest.raises(ValueError, match="not fitted"):
        t.transform(torch.zeros(3, 6))
    with pytest.raises(ValueError, match="not fitted"):
        LatentMap().transform(torch.zeros(3, 6))


def test_transform_argument_errors():
    t = _fitted()
    x = torch.zeros(3, 6)
    with pytest.raises(ValueError, match="must have 6 columns"):
        t.transform(torch.zeros(3, 5))
    with pytest.raises(ValueError, match="k_aff"):
        t.transform(x, perplexity=50)                              # k_aff = min(39, 150) = 39 <= 50
    with pytest.raises(ValueError, match="k_aff"):
        t.transform(x, perplexity=0.3)                             # k_aff = 0
    with pytest.raises(ValueError, match=r"k \(41\)"):
        t.transform(x, k=41)                                       # more than the 40 fitted rows
    with pytest.raises(ValueError, match=r"k \(129\)"):
        _fitted(200).transform(x, k=129)                           # more than the kernels keep
    with pytest.raises(ValueError, match="initialization"):
        t.transform(x, initialization="spectral")
    with pytest.raises(ValueError, match=r"must be \(3, 2\)"):
        t.transform(x, initialization=np.zeros((4, 2)))


def test_no_cpu_fallback():
    from gesture2vec_amd.embedding import LatentMap
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _fitted().transform(torch.zeros(3, 6))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LatentMap().fit(torch.zeros(30, 6))


def test_pickles_hold_host_tensors():
    from gesture2vec_amd.embedding import LatentMap
    t = _fitted()
    t.transform_kl_ = torch.zeros(3, dtype=torch.float64)
    back = pickle.loads(pickle.dumps(t))
    for name in ("fit_rows_", "embedding_", "transform_kl_"):
        assert not getattr(back, name).is_cuda and torch.equal(getattr(back, name), getattr(t, name))
    lm = LatentMap(n_pca=4, sample_size=30, random_state=1, perplexity=7.0)
    lm.tsne.fit_rows_, lm.tsne.embedding_ = t.fit_rows_, t.embedding_
    lm.coords_, lm.rows_ = t.embedding_, torch.arange(40)
    back = pickle.loads(pickle.dumps(lm))
    assert (back.n_pca, back.sample_size, back.random_state, back.tsne.perplexity) == (4, 30, 1, 7.0)
    assert torch.equal(back.coords_, lm.coords_) and torch.equal(back.rows_, lm.rows_) and torch.equal(back.tsne.fit_rows_, t.fit_rows_)


def test_inputs_leave_few_close_calls():
    """the case the conditionals are compared on: fewer than 2 % of its rows have two float64 distances closer than tau_i at rank
    k_aff or at rank kk, where the device's neighbour list may differ from the restatement's"""
    c = PI.main_case()
    assert PI.K_AFF == PR.k_aff(len(c["X"]), PI.PERPLEXITY)
    share = PI.close_calls(c["D"], c["X"], c["Z"], (PI.K_AFF, max(PI.K_AFF, PI.K)))
    assert share < 0.02
    X64 = c["X"].astype(np.float64)
    assert float(np.abs(X64.mean(0)).max()) < 0.05                 # centred as PCA scores are, to a few hundredths of the noise width
    assert np.array_equal(c["Z"][1], c["X"][3]) and np.array_equal(c["X"][4], c["X"][5])


def test_restatement_is_consistent():
    """neighbours in (d^2, index) order; conditionals at the asked perplexity; the analytic gradient is the derivative of the KL;
    the clip bounds the step; a row's result does not depend on the other rows"""
    c = PI.main_case()
    assert c["d2"][1, 0] == 0.0 and c["idx"][1, 0] == 3 and list(c["idx"][2, :2]) == [4, 5]
    assert (np.diff(c["d2"], axis=1) >= 0).all()
    p = PR.conditionals(c["d2"][:, :PI.K_AFF], PI.PERPLEXITY)
    H = -(p * np.log(p)).sum(1)
    assert float(np.abs(p.sum(1) - 1.0).max()) < 1e-12 and float(np.abs(H - np.log(PI.PERPLEXITY)).max()) <= 1e-5
    S = slice(0, 20)
    y = c["y0"][S].astype(np.float64)
    _, g, _ = PR.kl_grad(c["Y"], c["idx"][S], c["p"][S], y)
    h = 1e-5
    for a in range(2):
        e = np.zeros(2)
        e[a] = h
        num = (PR.kl_grad(c["Y"], c["idx"][S], c["p"][S], y + e)[0] - PR.kl_grad(c["Y"], c["idx"][S], c["p"][S], y - e)[0]) / (2 * h)
        assert float(np.abs(num - g[:, a]).max()) <= 1e-8
    big = np.full((20, 2), 3.0)
    y1, v1, _ = PR.step(y, np.zeros_like(y), np.ones_like(y), big, 0.8, 0.1, 0.25)
    assert np.allclose(np.sqrt(((y1 - y) ** 2).sum(1)), 0.1 * 0.8 * 0.25)
    whole = PR.descend(c["Y"], c["idx"][S], c["p"][S], c["y0"][S], n_iter=5)[0]
    part = PR.descend(c["Y"], c["idx"][3:4], c["p"][3:4], c["y0"][3:4], n_iter=5)[0]
    assert np.array_equal(whole[3:4], part)
