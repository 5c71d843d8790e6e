"""GPU tests of the device k-means (gesture2vec_amd/csrc/kmeans.hip, gesture2vec_amd/kmeans.py): the update kernels against float64
numpy, empty-cluster relocation and seeding against the restatement (tests/_kmeans_ref.py), whole fits against sklearn's recorded
ones (tests/golden/kmeans.npz), convergence gating, the padded centres, and the callers on the plain-autoencoder checkpoint."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import _kmeans_inputs as KI
import _kmeans_ref as KR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "kmeans.npz"))


# ---- g2v_kmeans_update against float64 numpy --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rows(N, E):
    rng = np.random.default_rng(1000 * E + N)
    X = np.tanh(rng.normal(size=(N, E)) * 0.8 + 0.1).astype(np.float32)
    return X, torch.from_numpy(X).to(DEV)


def _label_sets(N, K, rng):
    uniform = rng.integers(0, K, N)
    skewed = np.where(rng.random(N) < 0.9, K // 2, rng.integers(0, K, N))       # one cluster holds 90 % of the rows
    unused = 2 * rng.integers(0, (K + 1) // 2, N)                               # odd ids stay empty ...
    outside = rng.random(N) < 0.05
    unused[outside] = rng.choice([-1, -7, K, K + 5], int(outside.sum()))
    if N > 2:
        unused[N // 2] = K                                                      # ... and ids outside [0, K) are ignored
        unused[N // 3] = -1
    return {"uniform": uniform.astype(np.int64), "skewed": skewed.astype(np.int64), "unused": unused.astype(np.int64)}


@pytest.mark.parametrize("N", [1, 17, 1000, 4133, 65539])
@pytest.mark.parametrize("K", [1, 2, 17, 300])
@pytest.mark.parametrize("E", [16, 48, 400, 512])
def test_update_against_float64(E, K, N):
    """counts exact; sums within 1e-12 of sum |x| over the cluster's rows (float64 in another order); centres within 1e-6 max|x| (one
    fp32 rounding of a float64 quotient is 6e-8 relative); inertia and shift within 1e-6 relative; n_changed exact; same bits twice"""
    from gesture2vec_amd import ops
    X, xd = _rows(N, E)
    rng = np.random.default_rng(7 * N + 13 * K + E)
    C = (np.tanh(rng.normal(size=(K, E))) * 0.7).astype(np.float32)
    cd = torch.from_numpy(C).to(DEV)
    X64 = X.astype(np.float64)
    xmax = float(np.abs(X).max())
    for name, lab in _label_sets(N, K, rng).items():
        prev = lab.copy()
        flip = rng.random(N) < 0.3
        prev[flip] = (prev[flip] + 1 + rng.integers(0, 3, int(flip.sum()))) % (K + 3)       # (always a different value)
        ref = KR.update(X, lab, C, prev, relocate=False)
        ld, pd = torch.from_numpy(lab).to(DEV), torch.from_numpy(prev).to(DEV)
        got = ops.kmeans_update(xd, ld, cd, pd, relocate=False)
        again = ops.kmeans_update(xd, ld, cd, pd, relocate=False)
        for key in ("counts", "sums", "centers_new", "stats"):
            assert torch.equal(got[key].view(torch.uint8), again[key].view(torch.uint8)), f"{name}: {key} differs between two calls"
        counts, sums = got["counts"].cpu().numpy(), got["sums"].cpu().numpy()
        centers, stats = got["centers_new"].cpu().numpy(), got["stats"].cpu().numpy()
        assert np.array_equal(counts, ref["counts"]), name
        ok = (lab >= 0) & (lab < K)
        absum = np.zeros((K, E))
        order = np.argsort(lab[ok], kind="stable")
        starts = np.cumsum(ref["counts"]) - ref["counts"]
        if order.size:
            absum[ref["counts"] > 0] = np.add.reduceat(np.abs(X64[ok][order]), starts[ref["counts"] > 0], axis=0)
        serr = np.abs(sums - ref["sums"])
        cerr = float(np.abs(centers.astype(np.float64) - ref["centers"].astype(np.float64)).max())
        print(f"E={E} K={K} N={N} {name}: sum err / (1e-12 sum|x|) max {float((serr / (1e-12 * absum + 1e-300)).max()):.3f}, centres {cerr:.2e} "
              f"(bound {1e-6 * xmax:.2e}), inertia {stats[0]!r} vs {ref['inertia']!r}, shift {stats[1]!r} vs {ref['shift']!r}")
        assert (serr <= 1e-12 * absum).all(), name
        assert cerr <= 1e-6 * xmax, name
        assert abs(stats[0] - ref["inertia"]) <= 1e-6 * ref["inertia"], name
        assert abs(stats[1] - ref["shift"]) <= 1e-6 * ref["shift"], name
        assert stats[2] == ref["n_changed"] == int(flip.sum()), name
        assert stats[3] == 0
        no_prev = ops.kmeans_update(xd, ld, cd, None, relocate=False)
        assert no_prev["stats"][2].item() == N and torch.equal(no_prev["sums"], got["sums"])


def test_update_refuses_what_it_cannot_do():
    from gesture2vec_amd import _lib, ops
    x = torch.zeros(8, 6, device=DEV)
    with pytest.raises(_lib.G2VLibraryError, match="E % 4"):
        ops.kmeans_update(x, torch.zeros(8, dtype=torch.int64, device=DEV), torch.zeros(2, 6, device=DEV))
    with pytest.raises(_lib.G2VLibraryError):
        ops.kmeans_update(torch.zeros(8, 8), torch.zeros(8, dtype=torch.int64), torch.zeros(2, 8))


# ---- relocation -------------------------------------------------------------------------------------------------------------------
def _dup_case():
    X, init = KI.make(1200, 48, 12, 7)
    init = init.copy()
    init[[3, 7, 9]] = init[0]                                                   # three duplicated centres: empty at the first step
    return X, init


def test_relocation_step_equals_the_restatement():
    from gesture2vec_amd import ops
    from gesture2vec_amd.kmeans import KMeans
    X, init = _dup_case()
    xd = torch.from_numpy(X).to(DEV)
    lab_d = KMeans.from_centers(init).predict_device(xd)
    lab, gap = KR.assign(X, init)
    assert float(gap[gap > 0].min()) > 1e-5
    assert np.array_equal(lab_d.cpu().numpy(), lab) and not np.isin([3, 7, 9], lab).any()
    ref = KR.update(X, lab, init)
    got = ops.kmeans_update(xd, lab_d, torch.from_numpy(init).to(DEV), None, relocate=True)
    assert len(ref["relocated_rows"]) == 3 and got["stats"][3].item() == 3
    assert got["relocated_rows"][:3].cpu().tolist() == ref["relocated_rows"]
    assert np.array_equal(got["counts"].cpu().numpy(), ref["counts"])
    centers = got["centers_new"].cpu().numpy()
    for k, r in zip((3, 7, 9), ref["relocated_rows"]):
        assert np.array_equal(centers[k], X[r])
    assert float(np.abs(centers.astype(np.float64) - ref["centers"]).max()) <= 1e-6 * float(np.abs(X).max())
    assert abs(got["stats"][1].item() - ref["shift"]) <= 1e-6 * ref["shift"]
    assert torch.equal(lab_d, KMeans.from_centers(init).predict_device(xd))     # labels are not touched


def test_fit_with_relocation_equals_the_restatement():
    from gesture2vec_amd.kmeans import KMeans
    X, init = _dup_case()
    ref = KR.lloyd(X, init, track_gap=True)
    assert ref["relocated"] == 3 and ref["min_pos_gap"] > 1e-5
    km = KMeans(n_clusters=12, init=init).fit(torch.from_numpy(X).to(DEV))
    assert km.n_iter_ == ref["n_iter"]
    assert np.array_equal(km.labels_, ref["labels"])
    assert float(np.abs(km.cluster_centers_.astype(np.float64) - ref["centers"]).max()) <= 1e-6 * float(np.abs(X).max())
    assert abs(km.inertia_ - ref["inertia"]) <= 1e-6 * ref["inertia"]


# ---- the recorded sklearn fits ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fit(name, check_every=1):
    from gesture2vec_amd.kmeans import KMeans
    N, E, K, seed = KI.CASES[name]
    X, init = KI.make(N, E, K, seed)
    return X, init, KMeans(n_clusters=K, init=init, check_every=check_every).fit(torch.from_numpy(X).to(DEV))


@pytest.mark.parametrize("name", list(KI.CASES))
def test_fit_equals_sklearn(fx, name):
    """every label, n_iter_, the centres within 1e-6 max|x|, the inertia within 1e-5; predict_device on 1000 fresh rows = the float64
    argmin wherever the relative top-2 gap exceeds 1e-4, with at most 1 % of the rows inside that band"""
    N, E, K, seed = KI.CASES[name]
    X, init, km = _fit(name)
    assert KI.sha(X) == str(fx[f"{name}_sha_x"]) and KI.sha(init) == str(fx[f"{name}_sha_init"]), "the seeded inputs moved"
    print(f"{name}: n_iter {km.n_iter_} (sklearn {int(fx[f'{name}_n_iter'])}), inertia {km.inertia_!r} (sklearn {float(fx[f'{name}_inertia'])!r}), "
          f"labels differing {int((km.labels_ != fx[f'{name}_labels']).sum())}")
    assert km.labels_.shape == (N,) and km.labels_.min() >= 0 and km.labels_.max() < K
    assert np.array_equal(km.labels_, fx[f"{name}_labels"].astype(km.labels_.dtype))
    assert km.n_iter_ == int(fx[f"{name}_n_iter"])
    KI.check_centers(fx, name, km.cluster_centers_, 1e-6 * float(np.abs(X).max()))
    assert abs(km.inertia_ - float(fx[f"{name}_inertia"])) <= 1e-5 * km.inertia_
    fresh = KI.fresh_rows(N, E, K, seed)
    ref, gap = KR.assign(fresh, km.cluster_centers_)
    got = km.predict_device(torch.from_numpy(fresh).to(DEV))
    assert got.dtype == torch.int64 and got.is_cuda
    safe = gap > 1e-4
    print(f"{name}: {int((~safe).sum())} of 1000 fresh rows inside the 1e-4 band")
    assert (~safe).sum() <= 10
    assert np.array_equal(got.cpu().numpy()[safe], ref[safe])
    host = km.predict(fresh)
    assert isinstance(host, np.ndarray) and np.array_equal(host, got.cpu().numpy())
    assert np.array_equal(km.predict(torch.from_numpy(fresh)), host)


@pytest.mark.parametrize("name", ["small", "mid"])
def test_check_every_is_bitwise_the_same(name):
    """8 iterations per read-back: the iterations enqueued past convergence are no-ops (14 iterations = 8 + 6 of 8; 4 of 8)"""
    _, _, one = _fit(name)
    _, _, eight = _fit(name, 8)
    assert eight.n_iter_ == one.n_iter_
    assert np.array_equal(eight.cluster_centers_.view(np.uint32), one.cluster_centers_.view(np.uint32))
    assert np.array_equal(eight.labels_, one.labels_)
    assert eight.inertia_ == one.inertia_


def test_stops_by_max_iter_and_by_tol_like_the_restatement():
    from gesture2vec_amd.kmeans import KMeans
    N, E, K, seed = KI.CASES["small"]
    X, init = KI.make(N, E, K, seed)
    xd = torch.from_numpy(X).to(DEV)
    for kw in (dict(max_iter=3), dict(tol=3e-2)):
        ref = KR.lloyd(X, init, **kw)
        for m in (1, 8):
            km = KMeans(n_clusters=K, init=init, check_every=m, **kw).fit(xd)
            assert km.n_iter_ == ref["n_iter"] < 14, kw
            assert np.array_equal(km.labels_, ref["labels"]), kw
            assert float(np.abs(km.cluster_centers_.astype(np.float64) - ref["centers"]).max()) <= 1e-6, kw


def test_tolerance_kernel():
    from gesture2vec_amd import ops
    for N, E in ((1, 16), (1500, 48), (4133, 400)):
        X = np.random.default_rng(N).normal(size=(N, E)).astype(np.float32) * 0.5 + 0.25
        got = ops.kmeans_tolerance(torch.from_numpy(X).to(DEV), 1e-4).item()
        ref = KR.tolerance(X, 1e-4)
        assert abs(got - ref) <= 1e-12 * max(ref, 1e-30) + 1e-24, (N, E, got, ref)


# ---- seeding ----------------------------------------------------------------------------------------------------------------------
def test_kmeans_pp_picks_equal_the_restatement(fx):
    from gesture2vec_amd.kmeans import KMeans
    N, E, K, seed, rs_seed = KI.PP_CASE
    X, _ = KI.make(N, E, K, seed)
    assert KI.sha(X) == str(fx["pp_sha_x"])
    xd = torch.from_numpy(X).to(DEV)
    km = KMeans(n_clusters=K, init="k-means++", random_state=rs_seed)
    centers, rows = km._kmeans_pp(xd, np.random.RandomState(rs_seed))
    print("k-means++ rows:", rows)
    assert rows == fx["pp_rows"].tolist()
    assert np.array_equal(centers.cpu().numpy(), X[rows])
    km.fit(xd)
    assert km.init_rows_ == rows and km.labels_.max() < K


def test_random_init_indices_equal_numpys(fx):
    from gesture2vec_amd.kmeans import KMeans
    N, E, K, seed, rs_seed = KI.PP_CASE
    X, _ = KI.make(N, E, K, seed)
    km = KMeans(n_clusters=K, init="random", random_state=rs_seed, max_iter=2).fit(torch.from_numpy(X).to(DEV))
    assert km.init_rows_ == np.random.RandomState(rs_seed).permutation(N)[:K].tolist() == fx["pp_random_rows"].tolist()
    assert km.n_iter_ == 2 and np.isfinite(km.cluster_centers_).all() and km.labels_.max() < K


def test_n_init_keeps_the_lowest_inertia():
    from gesture2vec_amd.kmeans import KMeans
    X, _ = KI.make(1500, 48, 16, 1)
    xd = torch.from_numpy(X).to(DEV)
    singles = []
    rs = np.random.RandomState(3)
    for _ in range(3):
        singles.append(KMeans(n_clusters=16, init="random", random_state=rs, max_iter=50).fit(xd).inertia_)
    best = KMeans(n_clusters=16, init="random", n_init=3, random_state=3, max_iter=50).fit(xd)
    assert best.inertia_ == min(singles)


# ---- K = 300 padded to 304 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1000, 4133])           # g2v_vq_assign_fwd below 2048 rows, the packed kernel above
def test_padded_centres_never_win(N):
    from gesture2vec_amd.kmeans import KMeans
    X, init = KI.make(4133, 400, 300, 1)
    X = X[:N].copy()
    X[5] = np.nan                                     # an all-NaN row
    X[6] = 0.0
    X[7] = 1e30                                       # |x|^2 overflows fp32: every distance is +inf or NaN
    X[8, ::2] = np.nan
    X[9, 3] = np.inf                                  # x . 0 = NaN at the padding rows too: the first NaN (a real centre) wins
    X[10] = -np.inf
    X[11, 7], X[11, 8] = np.inf, -np.inf
    km = KMeans.from_centers(init)
    xd = torch.from_numpy(X).to(DEV)
    a = km.predict_device(xd).cpu().numpy()
    b = km.predict_device(xd).cpu().numpy()
    assert np.array_equal(a, b)
    assert a.min() >= 0 and a.max() < 300, (a.min(), a.max(), a[5:12])
    clean = np.ones(N, bool)
    clean[[5, 7, 8, 9, 10, 11]] = False
    ref, gap = KR.assign(X[clean], init)
    safe = gap > 1e-4
    assert np.array_equal(a[clean][safe], ref[safe])
    assert _fit("shipped")[2].labels_.max() < 300


# ---- end to end on the plain-autoencoder checkpoint -------------------------------------------------------------------------------
def test_plain_autoencoder_end_to_end(golden_dir):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from utils.train_utils import load_checkpoint_and_model
    from gesture2vec_amd.kmeans import KMeans
    from gesture2vec_amd.metrics import gesture_metrics
    from gesture2vec_amd.pipeline import chunk_latents, chunks_to_codes
    args, net, _, _, pose_dim = load_checkpoint_and_model(os.path.join(golden_dir, "plain_ae_ckpt.bin"), DEV, "autoencoder_vq")
    assert net.vq is False
    g = torch.Generator().manual_seed(5)
    real = torch.randn(700, int(args.n_poses), pose_dim, generator=g).to(DEV)
    gen = (0.8 * torch.randn(500, int(args.n_poses), pose_dim, generator=g) + 0.1).to(DEV)
    lat = chunk_latents(net, real)
    km = KMeans(n_clusters=16, random_state=0, check_every=4).fit(lat)
    lat2, codes = chunks_to_codes(net, real, kmeans=km)
    assert torch.equal(lat2, lat) and codes.dtype == torch.int64 and codes.is_cuda
    assert np.array_equal(codes.cpu().numpy(), km.labels_)
    with pytest.raises(ValueError, match="no quantiser"):
        chunks_to_codes(net, real)
    m = gesture_metrics(net, real, gen, kmeans=km)
    print("gesture_metrics with k-means codes:", m)
    for key in ("frechet", "hellinger", "perplexity_real", "perplexity_generated", "wasserstein"):
        assert m[key] is not None and np.isfinite(m[key]), key
    assert abs(m["perplexity_real"] - km.code_perplexity()) <= 1e-9 * m["perplexity_real"]
    plain = gesture_metrics(net, real, gen)
    assert plain["hellinger"] is None and plain["frechet"] == m["frechet"]


def test_sentence_dataset_takes_kmeans_ids():
    """TrinityDataset_sentencelevel.batches() with an autoencoder that has no vq_layer: cluster_ids = kmeans.predict_device(rows)"""
    from gesture2vec_amd.data.dataset import TrinityDataset_sentencelevel
    from gesture2vec_amd.kmeans import KMeans
    X, init = KI.make(60, 16, 5, 2)
    km = KMeans.from_centers(init)

    class Net:                                         # no vq_layer
        pass

    ds = TrinityDataset_sentencelevel.__new__(TrinityDataset_sentencelevel)
    ds.n_samples, ds.vq_net, ds.kmeans = 6, Net(), km
    items = [(torch.arange(3 + i), torch.zeros(4, 2), torch.zeros(3), {"k": i}, torch.from_numpy(X[10 * i:10 * i + 10]), torch.zeros(1))
             for i in range(6)]
    ds.__class__ = type("DS", (TrinityDataset_sentencelevel,), {"__getitem__": lambda self, i: items[i]})
    batches = list(ds.batches(3, DEV, shuffle=False))
    assert len(batches) == 2
    for words, lengths, poses, audio, aux, lat, codes, gpt3 in batches:
        assert codes.shape == (3, 10) and codes.dtype == torch.int64
        assert torch.equal(codes.reshape(-1), km.predict_device(lat.reshape(30, 16)))
