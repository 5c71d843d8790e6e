"""Device-side DTW k-means (csrc/dtw.hip, gesture2vec_amd/timeseries.py) against the float64 restatement (tests/_dtw_ref.py).
No run of tslearn stands behind these tests: parity with it rests on its definition.

Bounds.  dtw^2: every term of every cost and of the path sum is a non-negative float64 product, so whatever the order of the sums the
result is within (F + T + S) 2^-53 <= 7.2e-14 relative of the exact value, and so is the restatement's; the bar is 1e-12.  sums: the
same argument per element, against the sum of |x| over the contributing terms.  Centres: 1e-12 per update, 25 updates in a fit, a
factor of four over: 1e-10 max|x|.  Labels, counts, n_iter and which clusters stop are compared exactly: tests/test_dtw_host.py
shows that no decision on these inputs is closer than 1e-9 relative.  The `exact` family (small integers) is compared bit for bit."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

import _dtw_inputs as DI
import _dtw_ref as DR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"

from gesture2vec_amd import _lib, ops  # noqa: E402
from gesture2vec_amd.timeseries import TimeSeriesKMeans, dtw_cdist  # noqa: E402

SHAPES_TS = [(1, 1), (1, 7), (7, 1), (2, 2), (15, 17), (16, 16), (17, 33), (34, 34), (63, 64), (64, 64)]
WIDTHS = [1, 3, 40, 135, 512]
SHAPES_NM = [(1, 1), (5, 3), (67, 41)]
REL = 1e-12


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int64)


def _ulps(got, want):
    return np.abs(got.view(np.int64) - want.view(np.int64))


def _check_cdist(x, y, want2, tag):
    """every output of one g2v_dtw_cdist call against want2 = the restatement's dtw^2 -> the largest relative error"""
    xd, yd = _dev(x), _dev(y)
    out2, labels, best = ops.dtw_cdist(xd, yd, squared=True, want_labels=True)
    out1 = dtw_cdist(xd, yd)
    again = ops.dtw_cdist(xd, yd, squared=True, want_labels=True)
    torch.cuda.synchronize()
    got2, got1 = out2.cpu().numpy(), out1.cpu().numpy()
    err = float(np.max(np.abs(got2 - want2) / np.where(want2 > 0, want2, 1.0)))
    print(f"{tag}: dtw^2 off by {err:.2e} relative (bar {REL:.0e})")
    assert np.all(got2[want2 == 0] == 0)
    assert err < REL
    assert int(_ulps(got1, np.sqrt(got2)).max()) <= 2                       # squared=False: the square root, rounded or adjacent
    assert np.array_equal(labels.cpu().numpy(), np.argmin(got2, axis=1))     # (numpy's argmin: the lowest index on ties)
    assert np.array_equal(best.cpu().numpy(), got2.min(axis=1))
    for a, b in zip((out2, labels, best), again):
        assert torch.equal(a, b)
    only = ops.dtw_cdist(xd, yd, want_out=False, want_labels=True)
    assert only[0] is None and torch.equal(only[1], labels) and torch.equal(_bits(only[2]), _bits(best))
    return err


# ---- 1. dtw_cdist --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("T,S", SHAPES_TS)
def test_cdist_against_the_restatement(T, S, F):
    """the three (N, M) of one (T, S, F) share one reference: the smaller ones are its leading blocks"""
    N, M = SHAPES_NM[-1]
    x, y = DI.random_pair(N, M, T, S, F, 100 * T + S + F)
    want = DR.cdist2(x, y)
    for n, m in SHAPES_NM:
        _check_cdist(x[:n], y[:m], want[:n, :m], f"T={T} S={S} F={F} N={n} M={m}")


def test_cdist_300_by_130_at_the_shipped_shape():
    x, y = DI.random_pair(300, 130, 34, 34, 135, 77)
    y[7] = y[3]                                                              # two equal centres: a tie for every row, index 3 wins
    _check_cdist(x, y, DR.cdist2(x, y), "T=34 S=34 F=135 N=300 M=130")
    labels = ops.dtw_cdist(_dev(x), _dev(y), want_out=False, want_labels=True)[1]
    assert not bool((labels == 7).any())


def test_cdist_of_a_set_with_itself():
    x, _ = DI.random_pair(70, 1, 20, 20, 9, 5)
    xd = _dev(x)
    d = dtw_cdist(xd)
    d2 = dtw_cdist(xd, squared=True)
    torch.cuda.synchronize()
    assert d.dtype == torch.float64 and tuple(d.shape) == (70, 70)
    assert bool((torch.diagonal(d) == 0).all()) and bool((torch.diagonal(d2) == 0).all())
    assert torch.equal(_bits(d2), _bits(d2.t()))                             # the cost is symmetric, and so are min and +
    assert torch.equal(_bits(d), _bits(dtw_cdist(xd, xd.double())))          # fp32 centres widen exactly
    want = DR.cdist2(x, x.astype(np.float64))
    assert float(np.max(np.abs(d2.cpu().numpy() - want) / np.where(want > 0, want, 1.0))) < REL


# ---- 2. the exact family ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,T,S,F,K", [(40, 6, 6, 3, 4), (150, 17, 12, 5, 5), (33, 34, 34, 2, 3), (20, 1, 5, 4, 2), (20, 5, 1, 4, 2)])
def test_exact_family_bit_for_bit(N, T, S, F, K):
    x = DI.exact(N, T, F, 11 * N + T)
    c = DI.exact(K + 1, S, F, 13 * N + S)[:K].astype(np.float64)
    if T == S:
        c[0] = x[0]                                                          # a centre that is a row: 0 apart, twice (the last row copies row 0)
    want2 = DR.cdist2(x, c)
    out2, labels, best = ops.dtw_cdist(_dev(x), _dev(c), squared=True, want_labels=True)
    torch.cuda.synchronize()
    assert np.array_equal(out2.cpu().numpy(), want2)
    lab = np.argmin(want2, axis=1)
    assert np.array_equal(labels.cpu().numpy(), lab) and np.array_equal(best.cpu().numpy(), want2.min(axis=1))
    ref = DR.dba_accumulate(x, lab, c)
    got = ops.dtw_dba_accumulate(_dev(x), labels, _dev(c))
    torch.cuda.synchronize()
    assert np.array_equal(got["counts"].cpu().numpy(), ref["counts"])        # ties everywhere: this pins the tie rule on the device
    assert np.array_equal(got["sums"].cpu().numpy(), ref["sums"])
    assert np.array_equal(got["cost"].cpu().numpy(), ref["cost"])


# ---- 3. g2v_dtw_dba_accumulate on the planted cases -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted():
    return {name: DI.planted(name) for name in DI.CASES}


@pytest.mark.parametrize("which", ["uniform", "heavy", "holes"])
@pytest.mark.parametrize("name", list(DI.CASES))
def test_dba_accumulate(planted, name, which):
    x, init, K = planted[name]
    labels = DI.label_sets(x.shape[0], K, 3)[which]
    live = None
    if which == "holes":
        live = np.ones(K, dtype=np.uint8)
        live[K - 1] = 0
    ref = DR.dba_accumulate(x, labels, init, live)
    assert ref["path_gap"] > DI.GAP
    xd, ld, cd = _dev(x), _dev(labels), _dev(init)
    out = {"sums": torch.full((K,) + init.shape[1:], -7.0, dtype=torch.float64, device=DEV),
           "counts": torch.full((K, init.shape[1]), -7, dtype=torch.int64, device=DEV),
           "cost": torch.full((K,), -7.0, dtype=torch.float64, device=DEV)}
    got = ops.dtw_dba_accumulate(xd, ld, cd, None if live is None else _dev(live), out=out)
    again = ops.dtw_dba_accumulate(xd, ld, cd, None if live is None else _dev(live))
    torch.cuda.synchronize()
    t = ref["touched"]
    sums, counts, cost = got["sums"].cpu().numpy(), got["counts"].cpu().numpy(), got["cost"].cpu().numpy()
    assert np.array_equal(counts[t], ref["counts"][t])
    err_s = float(np.max(np.abs(sums[t] - ref["sums"][t]) / np.maximum(ref["abs"][t], 1e-300)))
    err_c = float(np.max(np.abs(cost[t] - ref["cost"][t]) / np.where(ref["cost"][t] > 0, ref["cost"][t], 1.0)))
    print(f"{name}/{which}: sums off by {err_s:.2e} of sum |x|, cost by {err_c:.2e} relative (bars {REL:.0e})")
    assert err_s < REL and err_c < REL
    assert np.all(sums[~t] == -7.0) and np.all(counts[~t] == -7) and np.all(cost[~t] == -7.0)      # not live: untouched
    if which == "holes":
        assert np.all(counts[1] == 0) and np.all(sums[1] == 0) and cost[1] == 0                  # live without rows: overwritten
    for key in ("sums", "counts", "cost"):
        assert torch.equal(got[key][_dev(t)], again[key][_dev(t)])


# ---- 4. whole fits ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ref_fits(planted):
    return {name: DR.fit(planted[name][0], planted[name][1], max_iter=5, max_iter_barycenter=5) for name in DI.FIT_CASES}


@pytest.mark.parametrize("name", DI.FIT_CASES)
def test_fit_from_a_given_init(planted, ref_fits, name):
    x, init, K = planted[name]
    ref = ref_fits[name]
    assert not ref["empty"] and ref["centre_gap"] > DI.GAP and ref["path_gap"] > DI.GAP
    km = TimeSeriesKMeans(n_clusters=K, max_iter=5, max_iter_barycenter=5, init=init).fit(_dev(x))
    assert km.labels_.dtype == np.int32 and np.array_equal(km.labels_, ref["labels"])
    assert km.n_iter_ == ref["n_iter"]
    err_i = abs(km.inertia_ - ref["inertia"]) / ref["inertia"]
    err_c = float(np.max(np.abs(km.cluster_centers_ - ref["centers"])) / np.max(np.abs(x)))
    print(f"{name}: inertia off by {err_i:.2e} relative (bar 1e-11), centres by {err_c:.2e} max|x| (bar 1e-10)")
    assert km.cluster_centers_.dtype == np.float64 and km.cluster_centers_.shape == init.shape
    assert err_i < 1e-11 and err_c < 1e-10
    assert np.array_equal(km.predict(x), DR.cdist2(x, km.cluster_centers_).argmin(axis=1))


# ---- 5. the stop rule -------------------------------------------------------------------------------------------------------------------
def _one_assignment(x, init):
    xd, cd = _dev(x), _dev(init)
    labels = ops.dtw_cdist(xd, cd, want_out=False, want_labels=True)[1]
    return xd, cd, labels, torch.bincount(labels, minlength=init.shape[0])


def test_enqueued_steps_equal_stepping_one_at_a_time(planted):
    x, init, K = planted["n150"]
    xd, c_all, labels, members = _one_assignment(x, init)
    state, prev, live = ops.dtw_dba_state(K, DEV)
    for _ in range(8):                                                       # all eight enqueued, nothing read back
        ops.dtw_dba_update(ops.dtw_dba_accumulate(xd, labels, c_all, live), members, state, c_all, 1e-5)
    c_one = _dev(init)
    state1, prev1, live1 = ops.dtw_dba_state(K, DEV)
    alive = []
    for _ in range(8):
        acc = ops.dtw_dba_accumulate(xd, labels, c_one, live1)
        ops.dtw_dba_update(acc, members, state1, c_one, 1e-5)
        torch.cuda.synchronize()
        alive.append(live1.cpu().numpy().copy())                             # a read-back after every step
    assert torch.equal(_bits(c_all), _bits(c_one)) and torch.equal(state, state1)
    assert np.array_equal(alive[-1], live.cpu().numpy())


def test_clusters_stop_where_the_restatement_stops_them(planted):
    """second-round barycentres of n150: the restatement stops some clusters after 2 steps and others not at all"""
    x, init, K = planted["n150"]
    centers = init.copy()
    lab0 = DR.cdist2(x, centers).argmin(axis=1)
    DR.barycenters(x, lab0, centers, 5, 1e-5)
    lab1 = DR.cdist2(x, centers).argmin(axis=1)
    members = np.bincount(lab1, minlength=K)
    start = centers.copy()
    prev, live = np.full(K, np.inf), np.ones(K, dtype=np.uint8)
    xd, ld, cd, md = _dev(x), _dev(lab1), _dev(start), _dev(members)
    state, prev_d, live_d = ops.dtw_dba_state(K, DEV)
    history = []
    for _ in range(5):
        DR.dba_update(DR.dba_accumulate(x, lab1, centers, live), members, prev, live, centers, 1e-5)
        ops.dtw_dba_update(ops.dtw_dba_accumulate(xd, ld, cd, live_d), md, state, cd, 1e-5)
        torch.cuda.synchronize()
        assert np.array_equal(live_d.cpu().numpy(), live)
        history.append(live.copy())
    assert any(0 < h.sum() < K for h in history)                             # some clusters stopped while others went on
    on = prev < np.inf
    assert float(np.max(np.abs(prev_d.cpu().numpy()[on] - prev[on]) / prev[on])) < 1e-11
    assert float(np.max(np.abs(cd.cpu().numpy() - centers))) < 1e-10 * np.max(np.abs(x))


def test_tol_stops_the_outer_loop_where_the_restatement_stops(planted):
    x, init, K = planted["n150"]
    inert = DR.fit(x, init, max_iter=4, max_iter_barycenter=5, tol=0.0)["inertias"]
    steps = np.abs(np.diff(inert))
    tol = 1.5 * float(steps[1])                                              # a tolerance the second or the third assignment meets
    assert min(abs(s - tol) for s in steps) > 1e-9 * tol                     # the stop itself is not decided by rounding
    ref = DR.fit(x, init, max_iter=12, max_iter_barycenter=5, tol=tol)
    assert not ref["empty"] and ref["centre_gap"] > DI.GAP and ref["path_gap"] > DI.GAP and ref["n_iter"] in (2, 3)
    km = TimeSeriesKMeans(n_clusters=K, max_iter=12, max_iter_barycenter=5, tol=tol, init=init).fit(_dev(x))
    print(f"tol {tol:.3e}: n_iter {km.n_iter_} (restatement {ref['n_iter']})")
    assert km.n_iter_ == ref["n_iter"]
    assert np.array_equal(km.labels_, ref["labels"])


# ---- 6. smaller behaviours --------------------------------------------------------------------------------------------------------------
def test_predict_on_fresh_rows_of_another_length(planted, ref_fits):
    x, init, K = planted["n300"]
    km = TimeSeriesKMeans.from_centers(ref_fits["n300"]["centers"])
    fresh = DI.fresh("n300", 50, 27)                                         # S = 20, T = 27
    d2 = DR.cdist2(fresh, km.cluster_centers_)
    assert DR.centre_gap(d2) > DI.GAP
    got = km.predict(fresh)
    assert got.dtype == np.int32 and np.array_equal(got, d2.argmin(axis=1))
    dev = km.predict_device(_dev(fresh))
    assert dev.is_cuda and dev.dtype == torch.int64 and np.array_equal(dev.cpu().numpy(), got)
    assert np.array_equal(km.predict(torch.from_numpy(fresh)), got)
    again = pickle.loads(pickle.dumps(km))
    assert again._dev == {} and np.array_equal(again.predict(fresh), got)
    assert km.n_clusters == K and km.cluster_centers_.dtype == np.float64


def test_n_init_keeps_the_lowest_inertia(planted):
    x, _, K = planted["n150"]
    xd = _dev(x)
    rs = np.random.RandomState(4)
    singles = []
    for _ in range(3):                                                       # the three draws n_init=3 makes from one stream
        rows = rs.permutation(x.shape[0])[:K]
        singles.append(TimeSeriesKMeans(n_clusters=K, max_iter=3, max_iter_barycenter=3, init=x[rows].astype(np.float64)).fit(xd))
    km = TimeSeriesKMeans(n_clusters=K, max_iter=3, max_iter_barycenter=3, n_init=3, random_state=4).fit(xd)
    best = min(singles, key=lambda m: m.inertia_)
    assert km.inertia_ == best.inertia_ and np.array_equal(km.labels_, best.labels_)
    assert np.array_equal(km.cluster_centers_, best.cluster_centers_)
    assert len(km.init_rows_) == K and km.inertia_ <= min(m.inertia_ for m in singles)
    again = pickle.loads(pickle.dumps(km))
    assert np.array_equal(again.predict(x), km.predict(x)) and np.array_equal(km.fit_predict(xd), km.labels_)


def test_an_empty_cluster_raises_with_an_array_init(planted):
    x, init, K = planted["n150"]
    dup = init.copy()
    dup[3] = dup[1]                                                          # centre 3 can never win: the lowest index takes every tie
    with pytest.raises(ValueError, match="cluster 3 is empty"):
        TimeSeriesKMeans(n_clusters=K, max_iter=2, init=dup).fit(_dev(x))


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(planted):
    x, init, K = planted["n150"]
    with pytest.raises((_lib.G2VLibraryError, RuntimeError, TypeError)):
        dtw_cdist(torch.from_numpy(x))
    with pytest.raises((_lib.G2VLibraryError, RuntimeError, TypeError)):
        TimeSeriesKMeans(n_clusters=K).fit(torch.from_numpy(x))
    L = ops.dtw_max_len()
    assert L >= 64
    assert ops.dtw_workspace(4, 2, L + 1, 3, 8) == 0 and ops.dtw_workspace(4, 2, 3, L + 1, 8) == 0
    assert ops.dtw_workspace(4, 2, 3, 3, 513) == 0 and ops.dtw_workspace(4, 2, L, L, 512) > 0
    for T, S, F in ((L + 1, 3, 8), (3, L + 1, 8), (3, 3, 513)):
        with pytest.raises(_lib.G2VLibraryError, match=r"\(-4\)"):
            dtw_cdist(torch.zeros(4, T, F, device=DEV), torch.zeros(2, S, F, device=DEV))
        with pytest.raises(_lib.G2VLibraryError, match=r"\(-4\)"):
            ops.dtw_dba_accumulate(torch.zeros(4, T, F, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV),
                                   torch.zeros(2, S, F, dtype=torch.float64, device=DEV))
    for kw, named in (({"metric": "euclidean"}, "euclidean"), ({"metric": "softdtw"}, "softdtw"), ({"init": "k-means++"}, "k-means"),
                      ({"metric_params": {"sakoe_chiba_radius": 2}}, "metric_params"), ({"dtw_inertia": True}, "dtw_inertia")):
        with pytest.raises((NotImplementedError, TypeError), match=named):
            TimeSeriesKMeans(n_clusters=K, **kw)
    with pytest.raises((NotImplementedError, TypeError), match="weights"):
        TimeSeriesKMeans(n_clusters=K).fit(_dev(x), sample_weight=np.ones(len(x)))
    with pytest.raises((NotImplementedError, TypeError), match="unequal length"):
        TimeSeriesKMeans(n_clusters=2).fit([np.zeros((5, 3), np.float32), np.zeros((6, 3), np.float32)])
    with pytest.raises(ValueError, match="exceeds"):
        TimeSeriesKMeans(n_clusters=len(x) + 1).fit(_dev(x))


# ---- 8. scripts/cluster_latents.py --algorithm dtw ---------------------------------------------------------------------------------------
def test_cluster_latents_dtw(golden_dir, tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import cluster_latents
    from utils.train_utils import load_checkpoint_and_model
    ckpt = os.path.join(golden_dir, "plain_ae_ckpt.bin")
    args, _, _, _, pose_dim = load_checkpoint_and_model(ckpt, DEV, "autoencoder_vq")
    chunks, _ = DI.series(200, int(args.n_poses), pose_dim, 4, 9)
    np.save(tmp_path / "chunks.npy", chunks)
    common = ["--checkpoint", ckpt, "--chunks", str(tmp_path / "chunks.npy"), "--device", DEV]
    out = tmp_path / "dtw.pk"
    km = cluster_latents.main(common + ["--algorithm", "dtw", "--n_clusters", "4", "--max_iter", "5", "--max-iter-barycenter", "5",
                                        "--seed", "1", "--out", str(out)])
    printed = capsys.readouterr().out
    assert isinstance(km, TimeSeriesKMeans) and km.cluster_centers_.shape == (4, int(args.n_poses), pose_dim)
    assert f"n_iter: {km.n_iter_}\n" in printed and f"inertia: {km.inertia_!r}\n" in printed and f"wrote {out}\n" in printed
    assert f"code-usage perplexity: {km.code_perplexity()!r} of 4\n" in printed
    with open(out, "rb") as f:
        saved = pickle.load(f)
    assert saved._dev == {} and np.array_equal(saved.labels_, km.labels_)
    ref = DR.fit(chunks, chunks[km.init_rows_].astype(np.float64), max_iter=5, max_iter_barycenter=5)
    assert not ref["empty"] and ref["centre_gap"] > DI.GAP and ref["path_gap"] > DI.GAP
    assert np.array_equal(km.labels_, ref["labels"]) and km.n_iter_ == ref["n_iter"]
    # the written model predicts the labels it printed wherever the last update moved no row (labels_ are those of the centres
    # before the last update): on these planted rows that is every row
    assert np.array_equal(DR.cdist2(chunks, ref["centers"]).argmin(axis=1), ref["labels"])
    assert np.array_equal(saved.predict(chunks), km.labels_)
    # the other algorithms still return what they did
    from gesture2vec_amd.agglomerative import AgglomerativeClustering
    from gesture2vec_amd.dbscan import DBSCAN
    from gesture2vec_amd.kmeans import KMeans
    k2 = cluster_latents.main(common + ["--n_clusters", "4", "--no-silhouette", "--out", str(tmp_path / "km.pk")])
    assert isinstance(k2, KMeans) and k2.cluster_centers_.shape[0] == 4
    db = cluster_latents.main(common + ["--algorithm", "dbscan", "--out", str(tmp_path / "db.npz")])
    assert isinstance(db, DBSCAN)
    ac = cluster_latents.main(common + ["--algorithm", "ward", "--n_clusters", "4", "--out", str(tmp_path / "w.npz")])
    assert isinstance(ac, AgglomerativeClustering) and ac.n_clusters_ == 4
