"""Device-side soft-DTW (csrc/softdtw.hip, gesture2vec_amd/timeseries.py) against the float64 restatement (tests/_softdtw_ref.py).
No run of tslearn stands behind these tests: parity with it rests on its definition.

Bars, computed here from the restatement's own tiles.  About eight roundings per cell, each at most an ulp of max(|R|, gamma),
accumulate along T + S diagonals:
    tol_R = 8 (T + S) 2^-52 max(max|R|, gamma)                       values, absolute
    tol_E = 2 (T + S) tol_R / gamma                                  alignment cells, absolute (E <= 1)
    tol_G[i, f] = tol_E sum_n w_n sum_j 2 |z_if - x_njf| + 8 2^-52 sum |terms|
tests/test_softdtw_host.py holds the restatement itself to them against its longdouble run.  Labels, n_iter and the evaluation
counts are compared exactly: the host test shows that no assignment on these inputs is closer than 1e-9 relative.  Centres of a fit
are asked to 1e-9 max|centre|: not a rounding bound but the condition of having taken the optimiser's trajectory (a perturbation
of value and gradient by 1e-10 relative moves an L-BFGS-B result by 3e-10; another line-search branch is far above)."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

import _dtw_inputs as DI
import _softdtw_ref as SR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"

from gesture2vec_amd import _lib, ops  # noqa: E402
from gesture2vec_amd.timeseries import (SoftDTWKMeans, TimeSeriesKMeans, dtw_cdist, soft_dtw_alignment, soft_dtw_cdist,  # noqa: E402
                                        softdtw_barycenter)

SLAB = 128                                                                   # SDTW_SLAB of csrc/softdtw.hip


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int64)


def _check_cdist(x, y, gamma, want, maxR, tag):
    """every output of one g2v_softdtw_cdist call against the restatement's values -> the largest error in units of the bar"""
    T, S = x.shape[1], y.shape[1]
    xd, yd = _dev(x), _dev(y)
    out, labels, best = ops.softdtw_cdist(xd, yd, gamma, want_labels=True)
    again = ops.softdtw_cdist(xd, yd, gamma, want_labels=True)
    only = ops.softdtw_cdist(xd, yd, gamma, want_out=False, want_labels=True)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.all(np.isfinite(got))
    ratio = float(np.max(np.abs(got - want) / SR.tol_R(T, S, maxR, gamma)))
    print(f"{tag}: values off by {float(np.max(np.abs(got - want))):.2e}, {ratio:.2e} of the bar")
    assert ratio < 1.0
    assert np.array_equal(labels.cpu().numpy(), np.argmin(got, axis=1))      # (numpy's argmin: the lowest index on ties)
    assert np.array_equal(best.cpu().numpy(), got.min(axis=1))
    for a, b in zip((out, labels, best), again):
        assert torch.equal(a, b) and (a.dtype != torch.float64 or torch.equal(_bits(a), _bits(b)))
    assert only[0] is None and torch.equal(only[1], labels) and torch.equal(_bits(only[2]), _bits(best))
    return ratio


# ---- 1. soft_dtw_cdist ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", SR.WIDTHS)
@pytest.mark.parametrize("T,S", SR.SHAPES_TS)
def test_cdist_against_the_restatement(T, S, F):
    """the three (N, M) of one (T, S, F) share one reference: the smaller ones are its leading blocks"""
    x, y, g, want, maxR = SR.cdist_case(T, S, F)
    for n, m in SR.SHAPES_NM:
        _check_cdist(x[:n], y[:m], g, want[:n, :m], maxR[:n, :m], f"T={T} S={S} F={F} gamma={g} N={n} M={m}")


@pytest.mark.parametrize("gamma", SR.GAMMAS)
def test_cdist_every_gamma_at_the_shipped_shape(gamma):
    x, y = SR.inputs(40, 13, 34, 34, 135)
    y[7] = y[3]                                                              # two equal centres: a tie for every row, index 3 wins
    want, maxR = SR.cdist(x, y, gamma)
    _check_cdist(x, y, gamma, want, maxR, f"T=34 S=34 F=135 gamma={gamma} N=40 M=13")
    labels = ops.softdtw_cdist(_dev(x), _dev(y), gamma, want_out=False, want_labels=True)[1]
    assert not bool((labels == 7).any())


def test_cdist_of_the_scaled_series_stays_finite():
    """the series times 100 at gamma = 0.01: exponents reach -1e6, exp underflows to 0 and nothing becomes NaN"""
    x, y, g, want, maxR = SR.scaled_case()
    _check_cdist(x, y, g, want, maxR, "scaled by 100, gamma=0.01")
    xd, yd = _dev(x), _dev(y)
    labels = ops.softdtw_cdist(xd, yd, g, want_out=False, want_labels=True)[1]
    assert np.array_equal(labels.cpu().numpy(), want.argmin(axis=1))         # (the host test: decided by more than 1e-9)
    E, value = soft_dtw_alignment(xd[:5], yd[0], g)
    assert bool(torch.isfinite(E).all()) and bool(torch.isfinite(value).all())
    assert np.array_equal(value.cpu().numpy(), ops.softdtw_cdist(xd[:5], yd[:1], g)[0].cpu().numpy()[:, 0])


def test_cdist_wrapper():
    x, y = SR.inputs(9, 4, 12, 10, 5)
    xd, yd = _dev(x), _dev(y)
    v = soft_dtw_cdist(xd, yd, gamma=0.5)
    assert v.dtype == torch.float64 and tuple(v.shape) == (9, 4) and torch.equal(_bits(v), _bits(ops.softdtw_cdist(xd, yd, 0.5)[0]))
    assert torch.equal(_bits(soft_dtw_cdist(xd, yd, gamma=0.0)), _bits(dtw_cdist(xd, yd, squared=True)))      # as tslearn does
    self_ = soft_dtw_cdist(xd, gamma=1.0)
    assert tuple(self_.shape) == (9, 9) and torch.equal(_bits(self_), _bits(soft_dtw_cdist(xd, xd.double(), gamma=1.0)))
    with pytest.raises(ValueError, match="gamma"):
        soft_dtw_cdist(xd, yd, gamma=-1.0)


# ---- 2. soft_dtw_alignment -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", SR.WIDTHS)
@pytest.mark.parametrize("T,S", SR.SHAPES_TS)
def test_alignment_against_the_restatement(T, S, F):
    g = SR.case_gamma(T, S, F)
    x, y = SR.inputs(5, 1, T, S, F)
    ref = SR.alignment(x, y[0], g)
    maxR = np.abs(ref["R"]).max(axis=(1, 2))
    xd, zd = _dev(x), _dev(y[0])
    E, value = soft_dtw_alignment(xd, zd, g)
    E2, value2 = soft_dtw_alignment(xd, zd, g)
    torch.cuda.synchronize()
    assert tuple(E.shape) == (5, S, T) and tuple(value.shape) == (5,) and E.dtype == torch.float64
    assert torch.equal(_bits(E), _bits(E2)) and torch.equal(_bits(value), _bits(value2))
    rv = float(np.max(np.abs(value.cpu().numpy() - ref["value"]) / SR.tol_R(T, S, maxR, g)))
    re_ = float(np.max(np.abs(E.cpu().numpy() - ref["E"]) / SR.tol_E(T, S, maxR, g)[:, None, None]))
    print(f"T={T} S={S} F={F} gamma={g}: value at {rv:.2e} of its bar, E at {re_:.2e} of its bar")
    assert rv < 1.0 and re_ < 1.0
    assert bool((E[:, -1, -1] == 1).all())
    one_E, one_v = soft_dtw_alignment(xd[2], zd, g)                          # a single (T, F) row
    assert tuple(one_E.shape) == (S, T) and torch.equal(_bits(one_E), _bits(E[2])) and torch.equal(_bits(one_v), _bits(value[2]))


# ---- 3. g2v_softdtw_grad ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted():
    return {name: DI.planted(name) for name in DI.CASES}


def _check_grad(x, rows, z, gamma, w, tag, x_ref=None):
    """one evaluation over the member rows against the restatement -> (value, grad) device tensors"""
    T, S = x.shape[1], z.shape[0]
    ref = SR.objective((x if x_ref is None else x_ref)[rows], z, gamma, w)
    xd, rd, zd = _dev(x), _dev(np.asarray(rows, dtype=np.int64)), _dev(z)
    wd = None if w is None else _dev(np.asarray(w, dtype=np.float64))
    value, grad = ops.softdtw_grad(xd, rd, zd, gamma, wd)
    value2, grad2 = ops.softdtw_grad(xd, rd, zd, gamma, wd)
    torch.cuda.synchronize()
    assert torch.equal(_bits(value), _bits(value2)) and torch.equal(_bits(grad), _bits(grad2))
    wsum = float(len(rows) if w is None else np.sum(w))
    bar_v = wsum * SR.tol_R(T, S, ref["maxR"], gamma) + 8 * SR.EPS * ref["abs_value"]
    bar_g = SR.tol_E(T, S, ref["maxR"], gamma) * ref["lever"] + 8 * SR.EPS * ref["terms"]
    rv = abs(float(value.cpu().numpy()[0]) - ref["value"]) / bar_v
    rg = float(np.max(np.abs(grad.cpu().numpy() - ref["grad"]) / bar_g))
    print(f"{tag}: {len(rows)} rows, value at {rv:.2e} of its bar, gradient at {rg:.2e} of its bar")
    assert np.isfinite(rv) and np.isfinite(rg) and rv < 1.0 and rg < 1.0
    return value, grad


@pytest.mark.parametrize("weighted", [False, True], ids=["ones", "weights"])
@pytest.mark.parametrize("which", ["uniform", "heavy", "holes"])
@pytest.mark.parametrize("name", ["n300", "t64", "f135"])
def test_grad_on_member_patterns(planted, name, which, weighted):
    """n300's heavy cluster spans three slabs; t64 is the tile that needs more than 64 KB of LDS; f135 the shipped width"""
    x, init, K = planted[name]
    labels = DI.label_sets(x.shape[0], K, 3)[which]
    k = {"uniform": 2 % K, "heavy": K - 1, "holes": 0}[which]
    rows = np.flatnonzero(labels == k)
    assert len(rows) >= 2 and (name != "n300" or which != "heavy" or len(rows) > 2 * SLAB)
    w = np.random.RandomState(len(rows)).uniform(0.5, 2.0, size=len(rows)) if weighted else None
    _check_grad(x, rows, init[k], SR.FIT_GAMMA, w, f"{name}/{which}")


@pytest.mark.parametrize("R", [1, SLAB - 1, SLAB, SLAB + 1])
def test_grad_at_the_slab_edges_and_with_extra_rows(planted, R):
    x, init, K = planted["n300"]
    rows = np.sort(np.random.RandomState(R).permutation(x.shape[0])[:R])
    w = np.random.RandomState(R + 1).uniform(0.5, 2.0, size=R)
    value, grad = _check_grad(x, rows, init[1], 1.0, w, f"R={R}")
    small = x[:int(rows.max()) + 1]                                          # x without the rows past the last member
    value2, grad2 = _check_grad(small, rows, init[1], 1.0, w, f"R={R}, fewer rows")
    assert torch.equal(_bits(value), _bits(value2)) and torch.equal(_bits(grad), _bits(grad2))
    packed, _ = _check_grad(x[rows], np.arange(R), init[1], 1.0, w, f"R={R}, packed")      # the same members under other ids
    assert torch.equal(_bits(value), _bits(packed))


# ---- 4. barycentres and whole fits ------------------------------------------------------------------------------------------------------
def test_barycenter_against_the_restatement(planted):
    x, init, K = planted["n150"]
    X = x[:40]
    w = np.random.RandomState(2).uniform(0.5, 2.0, size=40)
    for kw in ({"init": init[0]}, {}, {"weights": w}, {"max_iter": 0}):
        kw = {"max_iter": 5, **kw}
        want, nfev_want = SR.barycenter(X, 0.5, **kw)
        got, nfev = softdtw_barycenter(_dev(X), gamma=0.5, return_nfev=True, **kw)
        err = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
        print(f"barycentre {sorted(kw)}: {nfev} evaluations (restatement {nfev_want}), off by {err:.2e} max|centre| (bar 1e-9)")
        assert got.dtype == np.float64 and got.shape == want.shape and nfev == nfev_want and err < 1e-9
    assert np.array_equal(softdtw_barycenter(X, gamma=0.5, max_iter=5, init=init[0]),      # numpy series are moved to the device
                          softdtw_barycenter(_dev(X), gamma=0.5, max_iter=5, init=init[0]))


@pytest.fixture(scope="module")
def fits(planted):
    return {name: SoftDTWKMeans(n_clusters=planted[name][2], max_iter=5, max_iter_barycenter=5, gamma=SR.FIT_GAMMA,
                                init=planted[name][1]).fit(_dev(planted[name][0])) for name in DI.FIT_CASES}


@pytest.mark.parametrize("name", DI.FIT_CASES)
def test_fit_from_a_given_init(planted, fits, name):
    x, init, K = planted[name]
    ref, km = SR.fit_case(name), fits[name]
    assert not ref["empty"] and ref["centre_gap"] > DI.GAP
    assert km.labels_.dtype == np.int32 and np.array_equal(km.labels_, ref["labels"])
    assert km.n_iter_ == ref["n_iter"]
    assert len(km.nfev_) == len(ref["nfev"]) and all(np.array_equal(a, b) for a, b in zip(km.nfev_, ref["nfev"]))
    err_c = float(np.max(np.abs(km.cluster_centers_ - ref["centers"])) / np.max(np.abs(ref["centers"])))
    bar_i = SR.tol_R(x.shape[1], init.shape[1], ref["maxR"], SR.FIT_GAMMA)
    err_i = abs(km.inertia_ - ref["inertia"])
    print(f"{name}: {sum(int(e.sum()) for e in km.nfev_)} evaluations, centres off by {err_c:.2e} max|centre| (bar 1e-9), "
          f"inertia by {err_i:.2e} (bar {bar_i:.2e})")
    assert km.cluster_centers_.dtype == np.float64 and km.cluster_centers_.shape == init.shape
    assert err_c < 1e-9 and err_i < bar_i
    v, _ = SR.cdist(x, km.cluster_centers_, SR.FIT_GAMMA)
    assert SR.centre_gap(v) > DI.GAP and np.array_equal(km.predict(x), v.argmin(axis=1))


def test_predict_on_fresh_rows_of_another_length_and_pickle(fits):
    km = fits["n300"]
    fresh = DI.fresh("n300", 50, 27)                                         # S = 20, T = 27
    v, _ = SR.cdist(fresh, km.cluster_centers_, SR.FIT_GAMMA)
    assert SR.centre_gap(v) > DI.GAP
    got = km.predict(fresh)
    assert got.dtype == np.int32 and np.array_equal(got, v.argmin(axis=1))
    dev = km.predict_device(_dev(fresh))
    assert dev.is_cuda and dev.dtype == torch.int64 and np.array_equal(dev.cpu().numpy(), got)
    again = pickle.loads(pickle.dumps(km))
    assert again._dev == {} and again.gamma == km.gamma and np.array_equal(again.predict(fresh), got)
    assert all(np.array_equal(a, b) for a, b in zip(again.nfev_, km.nfev_))
    bare = SoftDTWKMeans.from_centers(km.cluster_centers_, gamma=km.gamma)
    assert np.array_equal(bare.predict(torch.from_numpy(fresh)), got)


def test_an_empty_cluster_raises_with_an_array_init_and_random_init_fits(planted):
    x, init, K = planted["n150"]
    dup = init.copy()
    dup[3] = dup[1]                                                          # centre 3 can never win: the lowest index takes every tie
    with pytest.raises(ValueError, match="cluster 3 is empty"):
        SoftDTWKMeans(n_clusters=K, max_iter=2, gamma=0.5, init=dup).fit(_dev(x))
    km = SoftDTWKMeans(n_clusters=K, max_iter=2, max_iter_barycenter=2, metric_params={"gamma": 0.5}, random_state=0).fit(_dev(x))
    same = SoftDTWKMeans(n_clusters=K, max_iter=2, max_iter_barycenter=2, gamma=0.5, init=x[km.init_rows_].astype(np.float64)).fit(_dev(x))
    assert len(km.init_rows_) == K and np.array_equal(km.labels_, same.labels_) and km.inertia_ == same.inertia_
    assert np.array_equal(km.cluster_centers_, same.cluster_centers_)        # the same input gives the same bits


# ---- 5. limits ------------------------------------------------------------------------------------------------------------------------
def test_limits_and_refusals():
    L = ops.dtw_max_len()
    assert ops.softdtw_workspace(4, 2, L + 1, 3, 8) == 0 and ops.softdtw_workspace(4, 2, 3, L + 1, 8) == 0
    assert ops.softdtw_workspace(4, 2, 3, 3, 513) == 0 and ops.softdtw_workspace(4, 2, L, L, 512) > 0
    rows = torch.arange(4, dtype=torch.int64, device=DEV)
    for T, S, F in ((L + 1, 3, 8), (3, L + 1, 8), (3, 3, 513)):
        x, y = torch.zeros(4, T, F, device=DEV), torch.zeros(2, S, F, dtype=torch.float64, device=DEV)
        with pytest.raises(_lib.G2VLibraryError, match=r"\(-4\)"):
            ops.softdtw_cdist(x, y, 0.5)
        with pytest.raises(_lib.G2VLibraryError, match=r"\(-4\)"):
            ops.softdtw_alignment(x, y[0], 0.5)
        with pytest.raises(_lib.G2VLibraryError, match=r"\(-4\)"):
            ops.softdtw_grad(x, rows, y[0], 0.5)
    x, y = torch.zeros(4, 3, 8, device=DEV), torch.zeros(2, 3, 8, dtype=torch.float64, device=DEV)
    for g in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(_lib.G2VLibraryError, match=r"\(-1\)"):
            ops.softdtw_cdist(x, y, g)
        with pytest.raises(_lib.G2VLibraryError, match=r"\(-1\)"):
            ops.softdtw_alignment(x, y[0], g)
        with pytest.raises(_lib.G2VLibraryError, match=r"\(-1\)"):
            ops.softdtw_grad(x, rows, y[0], g)
    with pytest.raises((_lib.G2VLibraryError, RuntimeError, TypeError)):
        soft_dtw_cdist(torch.zeros(4, 3, 8))
    with pytest.raises(NotImplementedError, match="softdtw"):
        TimeSeriesKMeans(n_clusters=2, metric="softdtw")
    # rows outside [0, N) contribute nothing
    x, y = SR.inputs(6, 1, 5, 4, 3)
    v_in, g_in = ops.softdtw_grad(_dev(x), _dev(np.array([1, 4], dtype=np.int64)), _dev(y[0]), 0.5)
    v_out, g_out = ops.softdtw_grad(_dev(x), _dev(np.array([-3, 1, 4, 6], dtype=np.int64)), _dev(y[0]), 0.5)
    assert torch.equal(_bits(v_in), _bits(v_out)) and torch.equal(_bits(g_in), _bits(g_out))


# ---- 6. scripts/cluster_latents.py --algorithm softdtw ---------------------------------------------------------------------------------
def test_cluster_latents_softdtw(golden_dir, tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import cluster_latents
    from utils.train_utils import load_checkpoint_and_model
    ckpt = os.path.join(golden_dir, "plain_ae_ckpt.bin")
    args, _, _, _, pose_dim = load_checkpoint_and_model(ckpt, DEV, "autoencoder_vq")
    chunks, _ = DI.series(200, int(args.n_poses), pose_dim, 4, 9)
    np.save(tmp_path / "chunks.npy", chunks)
    out = tmp_path / "softdtw.pk"
    km = cluster_latents.main(["--checkpoint", ckpt, "--chunks", str(tmp_path / "chunks.npy"), "--device", DEV, "--algorithm", "softdtw",
                               "--gamma", "0.5", "--n_clusters", "4", "--max_iter", "3", "--max-iter-barycenter", "3", "--seed", "1",
                               "--out", str(out)])
    printed = capsys.readouterr().out
    assert isinstance(km, SoftDTWKMeans) and km.gamma == 0.5 and km.cluster_centers_.shape == (4, int(args.n_poses), pose_dim)
    assert f"n_iter: {km.n_iter_}\n" in printed and f"inertia: {km.inertia_!r}\n" in printed and f"wrote {out}\n" in printed
    assert f"code-usage perplexity: {km.code_perplexity()!r} of 4\n" in printed
    with open(out, "rb") as f:
        saved = pickle.load(f)
    assert saved._dev == {} and np.array_equal(saved.labels_, km.labels_)
    ref = SR.fit(chunks, chunks[km.init_rows_].astype(np.float64), 0.5, max_iter=3, max_iter_barycenter=3)
    assert not ref["empty"] and ref["centre_gap"] > DI.GAP
    assert np.array_equal(km.labels_, ref["labels"]) and km.n_iter_ == ref["n_iter"]
    assert all(np.array_equal(a, b) for a, b in zip(km.nfev_, ref["nfev"]))
    v, _ = SR.cdist(chunks, ref["centers"], 0.5)
    assert SR.centre_gap(v) > DI.GAP and np.array_equal(saved.predict(chunks), v.argmin(axis=1))
