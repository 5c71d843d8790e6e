"""Device-side silhouette coefficient (csrc/silhouette.hip, gesture2vec_amd/silhouette.py) against sklearn's recorded values
(tests/golden/silhouette.npz) and the float64 restatement from differences (tests/_silhouette_ref.py): shapes, label sets, row strides,
more rows than one pass of row tiles, the edge rules, `sample_size`, and the k scan of scripts/cluster_latents.py.

Bars.  Per sample |s - ref| <= 5e-6 and |score - ref| <= 1e-6: an fp32 numpy restatement of the Gram form with the near pairs
re-evaluated is within 4.7e-7 per sample and 3.5e-9 on the mean on the recorded inputs, times ten for the summation order; the plain
Gram form is off by 1.2e-5 .. 5.2e-5 per sample there, so it is the near-pair path that these tests pin.  a and b: within 5e-6 of the
restatement, relative to the mean distance."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import _kmeans_inputs as KI
import _silhouette_inputs as SI
import _silhouette_ref as SR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
S_BAR, SCORE_BAR, AB_BAR = 5e-6, 1e-6, 5e-6
RECORDED = [("shipped", "nearest"), ("small", "nearest"), ("small", "skewed"), ("mid", "nearest")]


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "silhouette.npz"))


def _check_rows(N, seed=0):
    """every row up to 1000 rows; beyond, the rows of the planted pairs and 128 seeded ones (the restatement costs N x E per row)"""
    if N <= 1000:
        return np.arange(N)
    return np.unique(np.concatenate([np.arange(0, 70), np.random.default_rng(N + seed).choice(N, 128, replace=False)]))


def _run(x, lab, K):
    from gesture2vec_amd import ops
    res = ops.silhouette_samples(x, torch.from_numpy(lab).to(DEV), K)
    torch.cuda.synchronize()
    return res


def _compare(tag, res, D, lab, rows, K, s_ref=None):
    """a, b, s of `rows` against the restatement from their distance rows D (and s against `s_ref` where given)"""
    a, b, s = (res[k].cpu().numpy() for k in ("a", "b", "s"))
    ra, rb, rs = SR.terms(D, lab, rows)
    scale = float(D.mean())
    ea, eb = float(np.abs(a[rows] - ra).max()) / scale, float(np.abs(b[rows] - rb).max()) / scale
    es = float(np.abs(s[rows] - rs).max())
    msg = f"{tag}: a within {ea:.2e}, b within {eb:.2e} of the mean distance {scale:.3f}; s within {es:.2e} of the restatement"
    if s_ref is not None:
        es2, esc = float(np.abs(s - s_ref).max()), abs(float(res["out"][0].item()) / len(s) - float(s_ref.mean()))
        msg += f", within {es2:.2e} of sklearn per sample and {esc:.2e} on the score"
    print(msg)
    assert not np.isnan(s).any()
    assert ea <= AB_BAR and eb <= AB_BAR and es <= S_BAR
    if s_ref is not None:
        assert es2 <= S_BAR and esc <= SCORE_BAR
    assert np.array_equal(res["counts"].cpu().numpy()[:K], np.bincount(lab, minlength=K))
    assert int(res["counts"][K].item()) == 0 and int(res["out"][1].item()) == len(np.unique(lab))
    tot = float(res["out"][0].item())
    assert abs(tot - float(s.sum())) <= 1e-9 * max(1.0, float(np.abs(s).sum()))


# ---- 1. sklearn's recorded values ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case_distances(name):
    X, _, _ = SI.case(name)
    rows = _check_rows(X.shape[0])
    return rows, SR.distances(X, rows)


@pytest.mark.parametrize("name,which", RECORDED)
def test_against_sklearn(fx, name, which):
    X, sets, K = SI.case(name)
    lab = sets[which]
    assert KI.sha(X) == str(fx[f"{name}_sha_x"]) and KI.sha(lab) == str(fx[f"{name}_{which}_sha_labels"])
    rows, D = _case_distances(name)
    res = _run(torch.from_numpy(X).to(DEV), lab, K)
    _compare(f"{name}/{which}", res, D, lab, rows, K, s_ref=fx[f"{name}_{which}_s"])


# ---- 2. shapes and label sets against the restatement --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rows(N, E):
    rng = np.random.default_rng(1000 * E + N)
    X = SI.plant_pairs(np.tanh(rng.normal(size=(N, E)) * 0.8 + 0.1).astype(np.float32), N + E)
    rows = _check_rows(N)
    return X, torch.from_numpy(X).to(DEV), rows, SR.distances(X, rows)


def _label_sets(N, K, rng):
    """name -> (labels, number of ids): K clusters drawn uniformly; one cluster with 90 % of the rows; K clusters on the even ids of 2 K"""
    uniform = rng.integers(0, K, N)
    skewed = np.where(rng.random(N) < 0.9, K // 2, rng.integers(0, K, N))
    unused = 2 * rng.integers(0, K, N)                                          # odd ids stay empty
    return {"uniform": (uniform.astype(np.int64), K), "skewed": (skewed.astype(np.int64), K), "unused": (unused.astype(np.int64), 2 * K)}


SHAPES = [(E, K, N) for E in (16, 48, 400, 512) for K in (2, 17, 300) for N in (17, 1000, 4133) if K < N]


@pytest.mark.parametrize("E,K,N", SHAPES)
def test_shapes_against_float64(E, K, N):
    X, xd, rows, D = _rows(N, E)
    for which, (lab, ids) in _label_sets(N, K, np.random.default_rng(7 * N + K)).items():
        res = _run(xd, lab, ids)
        _compare(f"E={E} K={K} N={N} {which}", res, D, lab, rows, ids)
        again = _run(xd, lab, ids)
        for key in ("a", "b", "s", "out", "counts"):
            assert torch.equal(res[key], again[key]), f"{key} differs between two calls"


def test_two_rows():
    X, xd, rows, D = _rows(2, 16)
    res = _run(xd, np.array([0, 1]), 2)                          # two clusters of one row
    assert torch.equal(res["s"], torch.zeros(2, dtype=torch.float64, device=DEV)) and int(res["out"][1].item()) == 2
    res = _run(xd, np.array([0, 0]), 1)                          # one cluster: a = d, no other cluster
    assert abs(float(res["a"][0].item()) - D[0, 1]) <= AB_BAR * D[0, 1] and torch.isinf(res["b"]).all() and not res["s"].any()


def test_row_stride():
    """a column slice of a wider tensor (ld = 64 > E = 48) gives the bits of the contiguous rows"""
    from gesture2vec_amd.silhouette import silhouette_samples
    X, xd, _, _ = _rows(1000, 48)
    lab = _label_sets(1000, 17, np.random.default_rng(3))["uniform"][0]
    wide = torch.randn(1000, 64, device=DEV)
    wide[:, 8:56] = xd
    view = wide[:, 8:56]
    assert view.stride(0) == 64 and not view.is_contiguous()
    from gesture2vec_amd import ops
    res = ops.silhouette_samples(view, torch.from_numpy(lab).to(DEV), 17)
    ref = _run(xd, lab, 17)
    for key in ("a", "b", "s", "out"):
        assert torch.equal(res[key], ref[key]), key
    assert torch.equal(silhouette_samples(view, lab, 17), ref["s"])


# ---- 3. more owner tiles than one pass over the chip ----------------------------------------------------------------------------------
def test_many_row_tiles():
    N, E, K = 65539, 400, 300
    rng = np.random.default_rng(11)
    X = SI.plant_pairs(np.tanh(rng.normal(size=(N, E)) * 0.8 + 0.1).astype(np.float32), 11)
    lab = rng.integers(0, K, N).astype(np.int64)
    lab[10:66] = lab[10]                                          # the planted pairs share a cluster
    rows = np.unique(np.concatenate([np.arange(10, 66), rng.choice(N, 456, replace=False)]))[:512]
    res = _run(torch.from_numpy(X).to(DEV), lab, K)
    _compare(f"E={E} K={K} N={N}", res, SR.distances(X, rows), lab, rows, K)


# ---- 4. edge rules ------------------------------------------------------------------------------------------------------------------
def test_edge_rules():
    from gesture2vec_amd import ops
    from gesture2vec_amd._lib import G2VLibraryError
    from gesture2vec_amd.silhouette import silhouette_samples, silhouette_score
    X, xd, rows, D = _rows(1000, 48)
    rng = np.random.default_rng(5)
    lab = rng.integers(0, 6, 1000).astype(np.int64)
    lab[[3, 500, 999]] = [6, 7, 8]                               # three clusters of one row
    s = silhouette_samples(xd, lab)
    assert s.dtype == torch.float64 and s.is_cuda and s.shape == (1000,)
    assert not s[[3, 500, 999]].any()
    _compare("singletons", _run(xd, lab, 9), D, lab, rows, 9)

    same = torch.full((40, 16), 0.37, device=DEV)                # identical rows in two clusters: a = b = 0 -> s = 0, no NaN
    res = _run(same, (np.arange(40) % 2).astype(np.int64), 2)
    for key in ("a", "b", "s"):
        assert torch.equal(res[key], torch.zeros(40, dtype=torch.float64, device=DEV)), key

    dup = xd[:64].clone()                                        # bitwise duplicates: distance exactly 0
    dup[1] = dup[0]
    lab2 = np.r_[0, 0, 1 + np.arange(62) % 3].astype(np.int64)
    res = _run(dup, lab2, 4)
    assert float(res["a"][0].item()) == 0.0 and float(res["a"][1].item()) == 0.0
    assert float(res["s"][0].item()) == 1.0 and float(res["b"][0].item()) == float(res["b"][1].item()) > 0.0

    with pytest.raises(ValueError, match="Number of labels is 1"):
        silhouette_score(xd, np.zeros(1000, np.int64))
    with pytest.raises(ValueError, match="Number of labels is 17"):
        silhouette_samples(xd[:17], np.arange(17))
    with pytest.raises(G2VLibraryError, match="E % 4"):
        ops.silhouette_samples(torch.zeros(32, 18, device=DEV), torch.zeros(32, dtype=torch.int64, device=DEV), 2)
    with pytest.raises(G2VLibraryError, match="E <= 512"):
        ops.silhouette_samples(torch.zeros(32, 516, device=DEV), torch.zeros(32, dtype=torch.int64, device=DEV), 2)
    bad = lab.copy()
    bad[17] = 9
    bad[18] = -1
    bad[19] = 1 << 40
    with pytest.raises(ValueError, match=r"3 labels are outside \[0, 9\)"):
        silhouette_samples(xd, bad, n_clusters=9)
    res = _run(xd, bad, 9)                                        # reported, never used as an address
    assert int(res["counts"][9].item()) == 3 and not res["s"][17:20].any()
    torch.cuda.synchronize()


# ---- 5. sample_size -----------------------------------------------------------------------------------------------------------------
def test_sample_size(fx):
    from gesture2vec_amd.silhouette import silhouette_samples, silhouette_score
    name, seed, size = SI.SAMPLE
    X, sets, K = SI.case(name)
    xd, lab = torch.from_numpy(X).to(DEV), sets["nearest"]
    score = silhouette_score(xd, lab, sample_size=size, random_state=seed)
    idx = np.random.RandomState(seed).permutation(X.shape[0])[:size]
    sub = silhouette_samples(xd[torch.from_numpy(idx).to(DEV)].contiguous(), lab[idx])
    assert abs(score - float(sub.mean().item())) <= 1e-12
    err = abs(score - float(fx["sample_score"]))
    print(f"sample_size = {size}, random_state = {seed}: score {score!r}, within {err:.2e} of sklearn's")
    assert err <= SCORE_BAR
    assert silhouette_score(xd, lab, sample_size=size, random_state=np.random.RandomState(seed)) == score
    assert abs(silhouette_score(xd, lab, n_clusters=K) - float(silhouette_samples(xd, lab).mean().item())) <= 1e-12


# ---- 6. the k scan of scripts/cluster_latents.py -------------------------------------------------------------------------------------
def test_scan_k_prints_and_returns_the_silhouette(golden_dir, tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import cluster_latents
    from utils.train_utils import load_checkpoint_and_model
    from gesture2vec_amd.kmeans import KMeans
    from gesture2vec_amd.silhouette import silhouette_score
    ckpt = os.path.join(golden_dir, "plain_ae_ckpt.bin")
    args, net, _, _, pose_dim = load_checkpoint_and_model(ckpt, DEV, "autoencoder_vq")
    net.eval()
    real = torch.randn(700, int(args.n_poses), pose_dim, generator=torch.Generator().manual_seed(5))
    np.save(tmp_path / "chunks.npy", real.numpy())
    common = ["--checkpoint", ckpt, "--chunks", str(tmp_path / "chunks.npy"), "--device", DEV]
    curve = cluster_latents.main(common + ["--scan-k", "8:17:8"])
    printed = capsys.readouterr().out
    assert [c[0] for c in curve] == [8, 16] and all(len(c) == 3 for c in curve)
    lat = cluster_latents.latents_of(net, real.to(DEV), 65536)
    for k, inertia, sil in curve:
        km = KMeans(n_clusters=k, init="random", n_init=10, max_iter=300, random_state=0, check_every=4).fit(lat)
        assert km.inertia_ == inertia
        assert sil == silhouette_score(lat, km.labels_) == km.silhouette(lat)
        assert -1.0 <= sil <= 1.0 and f"k = {k}: inertia {inertia!r}, silhouette {sil!r}" in printed
    sampled = cluster_latents.main(common + ["--scan-k", "8:9:8", "--silhouette-rows", "300"])
    assert sampled[0][2] == KMeans(n_clusters=8, init="random", n_init=10, max_iter=300, random_state=0,
                                   check_every=4).fit(lat).silhouette(lat, sample_size=300, random_state=0)
    assert cluster_latents.main(common + ["--scan-k", "8:9:8", "--no-silhouette"])[0][2] is None
    km = cluster_latents.main(common + ["--n_clusters", "8", "--out", str(tmp_path / "km.pk")])
    assert f"silhouette: {km.silhouette(lat)!r}" in capsys.readouterr().out
