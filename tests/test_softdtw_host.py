"""CPU-only: the yardstick of the soft-DTW tests (tests/_softdtw_ref.py) and their inputs are checked before the device is asked,
and so is what of gesture2vec_amd/timeseries.SoftDTWKMeans needs no device.

Slack.  The identities below hold exactly for real numbers; the restatement is float64, so each is asked up to the rounding bar
the header's recursion earns (tests/_softdtw_ref.py: tol_R, eight roundings per cell along T + S diagonals, and tol_E)."""
import os
import pickle
import re

import numpy as np
import pytest

import _dtw_inputs as DI
import _dtw_ref as DR
import _softdtw_ref as SR

from gesture2vec_amd.timeseries import SoftDTWKMeans, TimeSeriesKMeans

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("P,T,S,F,gamma", [(3, 5, 4, 2, 1.0), (4, 9, 12, 3, 0.5), (2, 7, 7, 5, 0.01)])
def test_gradient_against_central_differences(P, T, S, F, gamma):
    """bar: a difference quotient of step h carries the values' rounding, at most sum_n w_n tol_R each side, over 2h; its
    truncation h^2 f''' / 6 is below 1e-7 of the gradient at h = 1e-6 on inputs of order one"""
    x, y = DI.random_pair(P, 1, T, S, F, 7)
    z, w, h = y[0], np.linspace(0.5, 2.0, P), 1e-6
    o = SR.objective(x, z, gamma, w)
    num = np.zeros_like(z)
    for i in range(S):
        for f in range(F):
            zp, zm = z.copy(), z.copy()
            zp[i, f] += h
            zm[i, f] -= h
            num[i, f] = (SR.objective(x, zp, gamma, w)["value"] - SR.objective(x, zm, gamma, w)["value"]) / (2 * h)
    bar = w.sum() * SR.tol_R(T, S, o["maxR"], gamma) / h + 1e-7 * np.abs(o["grad"]).max()
    err = float(np.abs(num - o["grad"]).max())
    print(f"T={T} S={S} F={F} gamma={gamma}: gradient off the difference quotient by {err:.2e} (bar {bar:.2e})")
    assert err < bar
    plain = SR.objective(x, z, gamma)                                       # weights absent: all ones
    ones = SR.objective(x, z, gamma, np.ones(P))
    assert plain["value"] == ones["value"] and np.array_equal(plain["grad"], ones["grad"])


@pytest.mark.parametrize("F", SR.WIDTHS)
@pytest.mark.parametrize("T,S", SR.SHAPES_TS)
def test_sandwich_between_dtw_and_its_log3_bound(T, S, F):
    """dtw^2 - gamma log 3 (T + S - 2) <= sdtw_gamma <= dtw^2: by induction over the cells, softmin lies between min - gamma log 3
    and min, and the (0, 0) cell adds nothing"""
    x, y, g, v, maxR = SR.cdist_case(T, S, F)
    d2 = DR.cdist2(x, y)
    slack = SR.tol_R(T, S, np.maximum(maxR, d2), g)
    assert np.all(np.isfinite(v))
    assert np.all(v <= d2 + slack)
    assert np.all(v >= d2 - g * np.log(3.0) * (T + S - 2) - slack)


@pytest.mark.parametrize("T,S,F,gamma", [(1, 1, 3, 0.5), (1, 7, 3, 1.0), (7, 1, 2, 0.01), (12, 12, 3, 0.01), (20, 17, 5, 0.5),
                                         (34, 34, 16, 1.0)])
def test_alignment_is_a_soft_path(T, S, F, gamma):
    """E is the expected number of visits of a cell under the Gibbs distribution over the warping paths: it lies in [0, 1], is 1 at
    both ends, and every path visits every row and every column at least once"""
    x, y = SR.inputs(6, 1, T, S, F)
    a = SR.alignment(x, y[0], gamma)
    E = a["E"]
    tol = SR.tol_E(T, S, np.abs(a["R"]).max(), gamma)
    assert E.shape == (6, S, T) and np.all(E >= 0) and np.all(E <= 1 + tol)
    assert np.all(np.abs(E[:, 0, 0] - 1) <= tol) and np.all(E[:, -1, -1] == 1)
    assert np.all(E.sum(axis=2) >= 1 - T * tol) and np.all(E.sum(axis=1) >= 1 - S * tol)
    wide = SR.alignment(x, y[0], gamma, np.longdouble)                      # and the bars hold for the restatement itself
    assert float(np.abs(wide["E"] - E).max()) <= tol
    assert float(np.abs(wide["value"] - a["value"]).max()) <= SR.tol_R(T, S, np.abs(a["R"]).max(), gamma)


def test_the_scaled_case_is_finite_and_decided():
    x, y, g, v, maxR = SR.scaled_case()
    assert np.all(np.isfinite(v)) and float(maxR.max()) / g > 1e6           # exponents of that order
    assert SR.centre_gap(v) > DI.GAP


@pytest.mark.parametrize("name", DI.FIT_CASES)
def test_fit_cases_are_decided_by_more_than_rounding(name):
    """only then may the device test demand equal labels"""
    ref = SR.fit_case(name)
    assert not ref["empty"] and ref["centre_gap"] > DI.GAP
    assert len(ref["nfev"]) == ref["n_iter"] and all(e.min() >= 1 for e in ref["nfev"])


def test_barycenter_edges():
    x, _ = SR.inputs(9, 1, 6, 6, 3)
    z0, n0 = SR.barycenter(x, 0.5, max_iter=0)
    assert n0 == 0 and np.allclose(z0, x.astype(np.float64).mean(axis=0), rtol=0, atol=1e-15)
    z, n = SR.barycenter(x, 0.5, max_iter=5)
    assert n >= 2 and SR.objective(x, z, 0.5)["value"] < SR.objective(x, z0, 0.5)["value"]


def test_class_surface_and_refusals():
    km = SoftDTWKMeans(n_clusters=40, metric="softdtw", max_iter=5, max_iter_barycenter=5, metric_params={"gamma": 0.5},
                       random_state=0)                                       # the reference's call, only the class name changed
    assert (km.n_clusters, km.max_iter, km.max_iter_barycenter, km.gamma, km.metric) == (40, 5, 5, 0.5, "softdtw")
    assert SoftDTWKMeans(gamma=0.25).gamma == 0.25 and SoftDTWKMeans().gamma == 1.0
    assert SoftDTWKMeans(verbose=1, n_jobs=2).cluster_centers_ is None
    for name in ("fit", "fit_predict", "predict", "predict_device", "from_centers", "code_perplexity"):
        assert callable(getattr(SoftDTWKMeans, name))
    assert SoftDTWKMeans.fit is TimeSeriesKMeans.fit and SoftDTWKMeans.predict_device is TimeSeriesKMeans.predict_device
    for kw, named in (({"metric_params": {"sakoe_chiba_radius": 2}}, "metric_params"), ({"init": "k-means++"}, "k-means"),
                      ({"metric_params": {"gamma": 0.5, "global_constraint": "itakura"}}, "metric_params")):
        with pytest.raises(NotImplementedError, match=named):
            SoftDTWKMeans(n_clusters=3, **kw)
    for g in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="gamma"):
            SoftDTWKMeans(gamma=g)
    with pytest.raises(ValueError, match="softdtw"):
        SoftDTWKMeans(metric="dtw")
    with pytest.raises(TypeError, match="frobnicate"):
        SoftDTWKMeans(frobnicate=1)
    with pytest.raises(NotImplementedError, match="weights"):
        SoftDTWKMeans().fit(np.zeros((4, 3, 2), np.float32), sample_weight=np.ones(4))
    with pytest.raises(NotImplementedError, match="unequal length"):
        SoftDTWKMeans(n_clusters=2).fit([np.zeros((5, 3), np.float32), np.zeros((6, 3), np.float32)])
    with pytest.raises(RuntimeError, match="not fitted"):
        SoftDTWKMeans().predict_device(None)


def test_pickle_round_trip_without_device_state():
    c = np.arange(24, dtype=np.float64).reshape(2, 4, 3)
    km = SoftDTWKMeans.from_centers(c, gamma=0.5)
    km._dev["cuda:0"] = object()                                             # whatever a predict left behind
    again = pickle.loads(pickle.dumps(km))
    assert isinstance(again, SoftDTWKMeans) and again._dev == {} and again.gamma == 0.5 and again.n_clusters == 2
    assert np.array_equal(again.cluster_centers_, c) and again.cluster_centers_.dtype == np.float64
    arr = pickle.loads(pickle.dumps(SoftDTWKMeans(n_clusters=2, init=c)))
    assert np.array_equal(arr.init, c)


def test_time_series_kmeans_still_refuses_softdtw_and_names_the_class():
    with pytest.raises(NotImplementedError, match="softdtw") as e:
        TimeSeriesKMeans(n_clusters=3, metric="softdtw")
    assert "SoftDTWKMeans" in str(e.value)
    with pytest.raises(NotImplementedError, match="metric_params"):
        TimeSeriesKMeans(n_clusters=3, metric_params={"gamma": 0.5})


def test_the_source_is_built_and_declared():
    mk = open(os.path.join(ROOT, "gesture2vec_amd", "csrc", "Makefile")).read()
    assert "softdtw.hip" in re.search(r"^SRCS\s*=(.*)$", mk, re.M)[1].split()
    from gesture2vec_amd import _lib
    for name in ("g2v_softdtw_workspace", "g2v_softdtw_cdist", "g2v_softdtw_alignment", "g2v_softdtw_grad"):
        assert name in _lib.EXPORTS
    csrc = os.path.join(ROOT, "gesture2vec_amd", "csrc")                     # the cost phase is written once, and both include it
    assert sum("s0 = fma(d0, d0, s0);" in open(os.path.join(csrc, n)).read() for n in os.listdir(csrc)
               if n.endswith((".hip", ".hpp"))) == 1
    for n in ("dtw.hip", "softdtw.hip"):
        assert '#include "dtw_tile.hpp"' in open(os.path.join(csrc, n)).read()
