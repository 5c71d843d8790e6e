"""Device-side exact t-SNE and PCA (csrc/tsne.hip, gesture2vec_amd/embedding.py) against the float64 restatement
(tests/_tsne_ref.py) and what sklearn 1.7 recorded (tests/golden/tsne.npz).

Bars.  P: max |dP| / max P <= max(4 x gap, 1e-6), where gap is the recorded distance between the restatement and sklearn's own P on
the same input (sklearn rounds its squared distances to fp32; 1.7e-8 .. 1.1e-5 on these inputs).  Gradient, KL, Z and the short
trajectory: 4 x the distance between the restatement evaluated in float32 and in float64, computed in the test (about 5e-7 of
max |grad| and 2e-7 of the KL on the recorded Y).  Full run: KL <= sklearn's float64 KL x (1 + m), trustworthiness >= sklearn's - m,
m = 3 x the relative KL spread between sklearn's float64 and float32 runs (6.2e-4 recorded, m = 1.9e-3); 5-NN accuracy 1.0."""
import functools
import os

import numpy as np
import pytest
import torch

import _tsne_inputs as TI
import _tsne_ref as TR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P_FLOOR = 1e-6
P_CASES = {"n97": (TI.SMALL_N, 400), "n1000": (1000, 400), "n1037": (1037, 48), "ld52": (300, 50)}
BIG_N, BIG_D = 23200, 16                                          # 4 N^2 bytes > 2^31


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "tsne.npz"))


def _sync(t):
    torch.cuda.synchronize()
    return t


@functools.lru_cache(maxsize=None)
def _base_P():
    """the device's P of the base case, on the device and as float64 on the host"""
    from gesture2vec_amd import ops
    P = _sync(ops.tsne_affinities(torch.from_numpy(TI.base()[0]).to(DEV), TI.PERPLEXITY))
    return P, P.cpu().numpy().astype(np.float64)


def _descend_device(P, y0, n_iter, exaggeration, momentum, lr):
    from gesture2vec_amd import ops
    y = torch.from_numpy(y0).to(DEV)
    vel, gains = torch.zeros_like(y), torch.ones_like(y)
    for _ in range(n_iter):
        grad, _ = ops.tsne_gradient(P, y, exaggeration, False)
        ops.tsne_update(y, vel, gains, grad, momentum, lr)
    return _sync(y)


# ---- 1. the joint P -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(P_CASES))
def test_joint_probabilities(fx, name):
    from gesture2vec_amd import ops
    N, d = P_CASES[name]
    X = TI.small()[0] if name == "n97" else TI.rows(N, d)
    assert TI.sha(X) == str(fx[f"sha_{name}"])
    if name == "ld52":                                            # rows on a pitch of 52 floats, the two spare columns hold junk
        wide = torch.full((N, 52), 7.5, device=DEV)
        wide[:, :d] = torch.from_numpy(X).to(DEV)
        xd = wide[:, :d]
        assert xd.stride(0) == 52
    else:
        xd = torch.from_numpy(X).to(DEV)
    P = _sync(ops.tsne_affinities(xd, TI.PERPLEXITY))
    assert P.shape == (N, N) and P.dtype == torch.float32
    assert torch.equal(P, P.t()) and not P.diagonal().any() and float(P.min().item()) == 0.0
    ref = TR.joint(X, TI.PERPLEXITY)
    got = P.cpu().numpy().astype(np.float64)
    err = float(np.abs(got - ref).max() / ref.max())
    bound = max(4.0 * float(fx[f"gap_{name}"]), P_FLOOR)
    print(f"{name}: N = {N}, d = {d}: max |dP| / max P = {err:.2e} (bound {bound:.2e}), sum P = {got.sum():.9f}")
    assert err <= bound and abs(got.sum() - 1.0) <= 1e-5
    assert (got[~np.eye(N, dtype=bool)] >= TR.EPS).all()
    if name != "n97":                                             # planted bitwise duplicates: distance exactly 0, the row's largest entry
        for m in range(TI.N_DUP):
            assert got[2 * m].argmax() == 2 * m + 1 and got[2 * m + 1].argmax() == 2 * m


# ---- 2. gradient, KL and Z ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("yname", ["tiny", "spread"])
@pytest.mark.parametrize("ex", [1.0, 12.0])
def test_gradient_kl_and_z(fx, yname, ex):
    """bounds: 4 x |restatement in float32 - restatement in float64| on the same P and Y (about 5e-7 of max |grad|, 2e-7 of the KL and
    of Z on these inputs)"""
    from gesture2vec_amd import ops
    P, P64 = _base_P()
    Y = fx[f"y_{yname}"]
    kl, g, Z = TR.kl_grad(P64, Y, ex)
    kl32, g32, Z32 = TR.kl_grad(P64, Y, ex, dtype=np.float32)
    gmax = float(np.abs(g).max())
    bg, bk, bz = 4.0 * float(np.abs(g32 - g).max()) / gmax, 4.0 * abs(kl32 - kl) / abs(kl), 4.0 * abs(Z32 - Z) / Z
    grad, out = ops.tsne_gradient(P, torch.from_numpy(Y).to(DEV), ex, True)
    out = _sync(out).cpu().numpy()
    gd = grad.cpu().numpy()
    eg, ek, ez = float(np.abs(gd - g).max()) / gmax, abs(out[0] - kl) / abs(kl), abs(out[2] - Z) / Z
    print(f"{yname} Y, exaggeration {ex}: grad within {eg:.2e} (bound {bg:.2e}), KL {out[0]:.9f} within {ek:.2e} ({bk:.2e}), "
          f"Z within {ez:.2e} ({bz:.2e})")
    assert eg <= bg and ek <= bk and ez <= bz
    assert abs(out[1] - float((gd.astype(np.float64) ** 2).sum())) <= 1e-12 * out[1]
    grad2, out2 = ops.tsne_gradient(P, torch.from_numpy(Y).to(DEV), ex, False)
    assert torch.equal(grad2, grad) and np.isnan(float(out2[0].item())) and float(out2[2].item()) == out[2]


# ---- 3. a short trajectory ------------------------------------------------------------------------------------------------------
def test_short_trajectory():
    """25 exploration iterations (exaggeration 12, momentum 0.5, learning rate 50) from the fixed init; bound: 4 x the distance
    between the restatement's float32 and float64 trajectories, relative to max |y|"""
    P, P64 = _base_P()
    y0 = TI.init_y(720)
    y64 = TR.descend(P64, y0, 25, 12.0, 0.5, 50.0)
    y32 = TR.descend(P64, y0, 25, 12.0, 0.5, 50.0, dtype=np.float32)
    scale = float(np.abs(y64).max())
    bound = 4.0 * float(np.abs(y32 - y64).max()) / scale
    err = float(np.abs(_descend_device(P, y0, 25, 12.0, 0.5, 50.0).cpu().numpy() - y64).max()) / scale
    print(f"25 iterations: within {err:.2e} of the float64 trajectory (bound {bound:.2e}, max |y| = {scale:.3e})")
    assert err <= bound


# ---- 4. the full run on the base case -------------------------------------------------------------------------------------------
def test_full_run(fx):
    from gesture2vec_amd.embedding import TSNE
    X, lab = TI.base()
    m = 3.0 * float(fx["run_kl_spread"])
    t = TSNE(perplexity=TI.PERPLEXITY, init=TI.init_y(720)).fit(torch.from_numpy(X).to(DEV))
    Y = t.embedding_.cpu().numpy().astype(np.float64)
    trust, knn = TR.trustworthiness(X, Y, 5), TR.knn_accuracy(Y, lab, 5)
    print(f"full run: KL {t.kl_divergence_:.6f} (sklearn float64 {float(fx['run_f64_kl']):.6f}, float32 {float(fx['run_f32_kl']):.6f}, "
          f"m = {m:.2e}), trustworthiness {trust:.4f} (sklearn {float(fx['run_f64_trust']):.4f}), 5-NN accuracy {knn:.4f}, "
          f"{t.n_iter_ + 1} iterations, learning rate {t.learning_rate_}")
    assert t.embedding_.is_cuda and t.embedding_.shape == (720, 2) and t.learning_rate_ == 50.0 and t.n_iter_ == 999
    assert t.kl_divergence_ <= float(fx["run_f64_kl"]) * (1.0 + m)
    assert knn == 1.0
    assert trust >= float(fx["run_f64_trust"]) - m


# ---- 5. determinism -------------------------------------------------------------------------------------------------------------
def test_same_input_same_bits():
    from gesture2vec_amd import ops
    from gesture2vec_amd.embedding import TSNE
    X = torch.from_numpy(TI.rows(1037, 48)).to(DEV)
    P1, P2 = ops.tsne_affinities(X, TI.PERPLEXITY), ops.tsne_affinities(X, TI.PERPLEXITY)
    assert torch.equal(P1, P2)
    y = torch.from_numpy((3.0 * np.random.RandomState(1).standard_normal((1037, 2))).astype(np.float32)).to(DEV)
    (g1, o1), (g2, o2) = ops.tsne_gradient(P1, y, 12.0, True), ops.tsne_gradient(P1, y, 12.0, True)
    assert torch.equal(g1, g2) and torch.equal(o1, o2)
    runs = [TSNE(max_iter=250, init="random", random_state=5).fit(X) for _ in range(2)]
    assert torch.equal(runs[0].embedding_, runs[1].embedding_) and runs[0].kl_divergence_ == runs[1].kl_divergence_


# ---- 6. byte offsets past 2^31 --------------------------------------------------------------------------------------------------
def test_offsets_past_2_31():
    """N = 23200: the last rows of P start beyond 2^31 bytes.  64 sampled rows (the first, the last, 62 seeded): their 64 x 64 block
    of P against the restatement's conditionals of those rows (sum (C + C^T) = 2 N), bound max(4 x the effect of rounding the
    distances to fp32, 1e-6) of the block's largest entry; their gradient rows against the restatement on the device's own P rows,
    bound 4 x its float32 - float64 distance."""
    from gesture2vec_amd import ops
    N = BIG_N
    assert 4 * N * N > 2 ** 31
    X = TI.rows(N, BIG_D)
    S = np.unique(np.concatenate([[0, N - 1], np.random.default_rng(6).choice(N, 62, replace=False)]))
    P = _sync(ops.tsne_affinities(torch.from_numpy(X).to(DEV), TI.PERPLEXITY))
    assert torch.equal(P[-512:, :], P[:, -512:].t()) and not P.diagonal().any()
    assert abs(float(P.sum(dtype=torch.float64).item()) - 1.0) <= 1e-5
    D = TR.sqdist(X, S)
    C = TR.conditionals(D, TI.PERPLEXITY, S)[0][:, S]
    C32 = TR.conditionals(D.astype(np.float32), TI.PERPLEXITY, S)[0][:, S]
    ref, ref32 = (C + C.T) / (2.0 * N), (C32 + C32.T) / (2.0 * N)
    Sd = torch.from_numpy(S).to(DEV)
    rows = P[Sd].cpu().numpy().astype(np.float64)
    got = rows[:, S].copy()
    off = ~np.eye(len(S), dtype=bool)
    bound = max(4.0 * float(np.abs(ref32 - ref).max() / ref.max()), P_FLOOR)
    err = float(np.abs(got - np.maximum(ref, TR.EPS))[off].max() / ref.max())
    print(f"N = {N}: P block within {err:.2e} of max (bound {bound:.2e})")
    assert err <= bound

    yd = torch.from_numpy((5.0 * np.random.RandomState(2).standard_normal((N, 2))).astype(np.float32)).to(DEV)
    Z = 0.0                                                       # the reference's Z: float64, in row blocks
    y64 = yd.double()
    for a in range(0, N, 2048):
        Z += float((1.0 / (1.0 + torch.cdist(y64[a:a + 2048], y64) ** 2)).sum().item())
    Z -= N
    Y = yd.cpu().numpy()
    _, g, _ = TR.kl_grad(rows, Y, 1.0, rows=S, Z=Z)
    _, g32, _ = TR.kl_grad(rows, Y, 1.0, dtype=np.float32, rows=S, Z=Z)
    grad, out = ops.tsne_gradient(P, yd, 1.0, False)
    gd = _sync(grad).cpu().numpy()[S]
    gmax = float(np.abs(g).max())
    eg, bg = float(np.abs(gd - g).max()) / gmax, 4.0 * float(np.abs(g32 - g).max()) / gmax
    ez = abs(float(out[2].item()) - Z) / Z
    print(f"N = {N}: gradient rows within {eg:.2e} (bound {bg:.2e}), Z within {ez:.2e}")
    assert eg <= bg and ez <= 1e-6
    del P
    torch.cuda.empty_cache()


# ---- 7. PCA ---------------------------------------------------------------------------------------------------------------------
def test_pca_against_sklearn(fx):
    """The covariance comes from fp32 products of rows rounded once about the shift, summed in float64: |d cov| <= 8 x 2^-24 |cov|, so
    a variance is within that of sklearn's and component k within 8 x 2^-24 lambda_0 / gap_k of it (gap_k: distance of lambda_k to its
    neighbours; the 50th component's upper neighbour is not recorded, so 49 are compared).  transform: an fp32 dot product of length
    400 plus the bias, |d| <= 2 x 401 x 2^-24 |x| |c| with |c| = 1, on top of the component error times |x - mean|."""
    from gesture2vec_amd.embedding import PCA
    X, _ = TI.base()
    xd = torch.from_numpy(X).to(DEV)
    pca = PCA(50)
    T = _sync(pca.fit_transform(xd))
    lam = fx["pca_explained_variance"]
    u = 8.0 * 2.0 ** -24
    assert T.shape == (720, 50) and T.stride(0) % 4 == 0
    assert float(np.abs(pca.mean_ - fx["pca_mean"]).max()) <= 2.0 ** -23 * float(np.abs(X).max())
    assert float(np.abs(pca.explained_variance_ - lam).max()) <= u * lam[0]
    assert float(np.abs(pca.explained_variance_ratio_ - fx["pca_explained_variance_ratio"]).max()) <= 2.0 * u
    gap = np.minimum(np.r_[np.inf, lam[:-2] - lam[1:-1]], lam[:-1] - lam[1:])           # of components 0 .. 48
    cerr = np.abs(pca.components_[:49] - fx["pca_components"][:49]).max(axis=1)
    print(f"PCA: variances within {float(np.abs(pca.explained_variance_ - lam).max() / lam[0]):.2e} of lambda_0, components within "
          f"{float((cerr * gap / lam[0]).max()):.2e} lambda_0 / gap")
    assert (cerr <= u * lam[0] / gap).all()
    assert (pca.components_[np.arange(50), np.abs(pca.components_).argmax(1)] > 0).all()
    xc = X.astype(np.float64) - pca.mean_
    rown = float(np.sqrt((X.astype(np.float64) ** 2).sum(1)).max())
    mine = xc @ pca.components_.T
    tol = 2.0 * 401 * 2.0 ** -24 * rown
    Th = T.cpu().numpy().astype(np.float64)
    assert float(np.abs(Th - mine).max()) <= tol
    xn = float(np.sqrt((xc ** 2).sum(1)).max())
    assert (np.abs(Th[:, :49] - fx["pca_transform"][:, :49]).max(axis=0) <= tol + np.sqrt(400.0) * cerr * xn).all()


def test_pca_pass_through_and_batches():
    from gesture2vec_amd.embedding import PCA
    X, _ = TI.base()
    xd = torch.from_numpy(X).to(DEV)
    few_rows, few_cols = xd[:30].contiguous(), xd[:, :40].contiguous()
    for x in (few_rows, few_cols):                                # fewer than n_components rows / columns: unchanged, as the reference
        p = PCA(50).fit(x)
        assert p.components_ is None and p.transform(x) is x and PCA(50).fit_transform(x) is x
    one = PCA(10).fit(xd)
    two = PCA(10).update(xd[:400]).update(xd[400:]).fit()
    assert two.n_samples_ == one.n_samples_ == 720
    # the same shift, but the moments' fp32 chains (<= 1024 rows, then float64) break at other rows: the bars of the sklearn
    # comparison above hold between the two, |d cov| <= 8 x 2^-24 |cov| (components 0 .. 8 have both neighbours among the ten)
    lam, u = one.explained_variance_, 8.0 * 2.0 ** -24
    assert float(np.abs(two.explained_variance_ - lam).max()) <= u * lam[0]
    assert float(np.abs(two.mean_ - one.mean_).max()) <= 2.0 ** -23 * float(np.abs(X).max())
    gap = np.minimum(np.r_[np.inf, lam[:-2] - lam[1:-1]], lam[:-1] - lam[1:])
    assert (np.abs(two.components_[:9] - one.components_[:9]).max(axis=1) <= u * lam[0] / gap).all()
    assert torch.equal(PCA(10).fit(xd).transform(xd), one.transform(xd))


# ---- 8. the wrappers ------------------------------------------------------------------------------------------------------------
def test_wrappers(tmp_path):
    from types import SimpleNamespace
    from gesture2vec_amd.embedding import TSNE, codebook_map, latent_map
    book = torch.nn.Embedding(512, 400)
    book.weight.data = torch.from_numpy(TI.clusters(8, 64, 400, 8)[0])
    net = SimpleNamespace(vq=True, vq_layer=SimpleNamespace(_embedding=book.to(DEV)))
    cm = _sync(codebook_map(net, max_iter=250))
    assert cm.shape == (512, 2) and cm.is_cuda and bool(torch.isfinite(cm).all())
    with pytest.raises(ValueError, match="no quantiser"):
        codebook_map(SimpleNamespace(vq=False, vq_layer=None))
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    import train_autoencoder_VQVAE as T                            # --embedding-maps: the same map, written where the reference saves its .png
    T.write_embedding_map(SimpleNamespace(model_save_path=str(tmp_path)), net, 3)
    saved = np.load(tmp_path / "plots" / "Embedding_Epoch(3).npz")["coords"]
    assert saved.shape == (512, 2) and np.isfinite(saved).all()

    X, lab = TI.base()
    xd = torch.from_numpy(X).to(DEV)
    coords, idx = latent_map(xd, sample_size=300, random_state=3, max_iter=300)
    want = np.random.RandomState(3).permutation(720)[:300]
    assert np.array_equal(idx.cpu().numpy(), want) and coords.shape == (300, 2)
    assert TR.knn_accuracy(_sync(coords).cpu().numpy().astype(np.float64), lab[want], 5) >= 0.99
    again, _ = latent_map(xd, sample_size=300, random_state=3, max_iter=300)
    assert torch.equal(again, coords)
    full, idx = latent_map(xd[:100], n_pca=50, max_iter=250, perplexity=10.0)          # 100 rows, 400 columns: PCA(50) still applies
    assert full.shape == (100, 2) and np.array_equal(idx.cpu().numpy(), np.arange(100))

    with pytest.raises(ValueError, match=r"perplexity \(30.0\) must be less than n_samples \(30\)"):
        TSNE().fit(xd[:30])
    with pytest.raises(ValueError, match="sample_size="):
        TSNE().fit(torch.zeros(32769, 4, device=DEV))
    with pytest.raises(ValueError, match=r"must be \(720, 2\)"):
        TSNE(init=np.zeros((5, 2))).fit(xd)


# ---- 9. scripts/embed_latents.py ------------------------------------------------------------------------------------------------
def test_embed_latents_script(golden_dir, tmp_path):
    import pickle
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    import embed_latents
    from utils.train_utils import load_checkpoint_and_model
    from gesture2vec_amd.kmeans import KMeans
    from gesture2vec_amd.pipeline import chunk_latents
    ckpt = os.path.join(golden_dir, "plain_ae_ckpt.bin")
    args, net, _, _, pose_dim = load_checkpoint_and_model(ckpt, DEV, "autoencoder_vq")
    net.eval()
    real = torch.randn(200, int(args.n_poses), pose_dim, generator=torch.Generator().manual_seed(5))
    np.save(tmp_path / "chunks.npy", real.numpy())
    lat = chunk_latents(net, real.to(DEV))
    km = KMeans(n_clusters=8, init="random", n_init=1, max_iter=50, random_state=0).fit(lat)
    with open(tmp_path / "km.pk", "wb") as f:
        pickle.dump(km, f)
    common = ["--checkpoint", ckpt, "--chunks", str(tmp_path / "chunks.npy"), "--device", DEV, "--max-iter", "250"]
    res = embed_latents.main(common + ["--kmeans", str(tmp_path / "km.pk"), "--sample-rows", "120", "--seed", "4",
                                       "--out", str(tmp_path / "map.npz"), "--scatter-txt", str(tmp_path / "scatter.txt")])
    rows = np.random.RandomState(4).permutation(200)[:120]
    saved = np.load(tmp_path / "map.npz")
    assert np.array_equal(saved["rows"], rows) and saved["coords"].shape == (120, 2) and np.isfinite(saved["coords"]).all()
    assert np.array_equal(saved["codes"], km.predict_device(lat).cpu().numpy()[rows])
    assert np.array_equal(res["coords"], saved["coords"])
    lines = open(tmp_path / "scatter.txt").read().split("\n")
    assert lines[0] == "512" and len(lines) == 122 and lines[-1] == ""
    assert lines[1] == "{},{:.3f},{:.3f}".format(int(saved["codes"][0]), saved["coords"][0, 0], saved["coords"][0, 1])
    plain = embed_latents.main(common + ["--out", str(tmp_path / "plain.npz")])                # no ids without a quantiser or k-means
    assert (plain["codes"] == -1).all() and np.array_equal(plain["rows"], np.arange(200))
