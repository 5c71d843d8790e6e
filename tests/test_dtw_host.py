"""CPU-only: the float64 restatement of the DTW block (tests/_dtw_ref.py) against brute force over all warping paths, its tie rule,
and the conditions under which tests/test_gpu_dtw.py may ask the device for equality: on every named input no assignment and no
path cell is decided by less than 1e-9 relative and no cluster goes empty.  Checked on the restatement alone."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import _dtw_inputs as DI
import _dtw_ref as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tile(a, b):
    cost = DR.cost_tiles(a[None].astype(np.float64), b[None].astype(np.float64))[0]
    return cost, DR.acc_tiles(cost[None])[0]


@pytest.mark.parametrize("T,S", list(itertools.product(range(1, 6), range(1, 6))))
def test_dtw2_is_the_minimum_over_all_paths(T, S):
    rs = np.random.RandomState(10 * T + S)
    for kind in ("random", "exact"):
        if kind == "random":
            a, b = rs.normal(size=(T, 3)), rs.normal(size=(S, 3))
        else:
            a, b = DI.exact(1, T, 2, T + S)[0], DI.exact(1, S, 2, 7 * T + S)[0]
        cost, acc = _tile(a, b)
        want, _ = DR.brute_force(cost)
        path, _ = DR.walk(acc)
        along = sum(cost[i, j] for i, j in reversed(path))                  # (in the order the recurrence added them)
        if kind == "exact":
            assert acc[-1, -1] == want and along == want
        else:
            assert abs(acc[-1, -1] - want) <= 1e-14 * max(want, 1e-300) * (T + S)
            assert abs(along - want) <= 1e-14 * max(want, 1e-300) * (T + S)
        assert path[0] == (T - 1, S - 1) and path[-1] == (0, 0)
        steps = {(p[0] - q[0], p[1] - q[1]) for p, q in zip(path[:-1], path[1:])}
        assert steps <= {(1, 1), (1, 0), (0, 1)}
        assert DR.cdist2(a[None].astype(np.float32), b[None])[0, 0] == \
            _tile(a.astype(np.float32), b)[1][-1, -1]                       # the pair-vectorised route: the same bits


def test_tie_order_on_crafted_ties():
    """all-equal costs: every interior cell ties three ways and the walk takes the diagonal, then (i-1, j) on the edge it reaches"""
    acc = DR.acc_tiles(np.ones((1, 4, 3)))[0]
    path, gap = DR.walk(acc)
    assert path == [(3, 2), (2, 1), (1, 0), (0, 0)] and gap == 0.0
    acc = DR.acc_tiles(np.ones((1, 2, 4)))[0]
    assert DR.walk(acc)[0] == [(1, 3), (0, 2), (0, 1), (0, 0)]
    # (i-1, j) and (i, j-1) tie below the diagonal: (i-1, j) is preferred
    assert DR.walk(np.array([[9.0, 1.0], [1.0, 5.0]]))[0] == [(1, 1), (0, 1), (0, 0)]
    # (i-1, j-1) ties with (i, j-1): the diagonal is preferred
    assert DR.walk(np.array([[1.0, 3.0], [1.0, 5.0]]))[0] == [(1, 1), (0, 0)]
    # (i, j-1) alone is the smallest
    assert DR.walk(np.array([[2.0, 3.0], [1.0, 5.0]]))[0] == [(1, 1), (1, 0), (0, 0)]


def test_identical_series_are_exactly_zero_apart():
    x, y = DI.random_pair(4, 1, 9, 9, 5, 3)
    d2 = DR.cdist2(x, x.astype(np.float64))
    assert np.all(np.diag(d2) == 0.0) and np.all(d2[~np.eye(4, dtype=bool)] > 0)


def test_dba_step_by_hand():
    """one centre of two rows, one member of three: the path, the sums, the counts and the cost written out"""
    c = np.array([[[0.0], [4.0]]])
    x = np.array([[[0.0], [1.0], [4.0]]], dtype=np.float32)
    acc = DR.dba_accumulate(x, np.array([0]), c)
    # cost = [[0, 1, 16], [16, 9, 0]]; acc = [[0, 1, 17], [16, 9, 1]]; path (1,2) -> (0,1) -> (0,0)
    assert acc["cost"][0] == 1.0 and acc["counts"].tolist() == [[2, 1]] and acc["sums"][0, :, 0].tolist() == [1.0, 4.0]
    prev, live = np.array([np.inf]), np.ones(1, dtype=np.uint8)
    DR.dba_update(acc, np.array([1]), prev, live, c, 1e-5)
    assert c[0, :, 0].tolist() == [0.5, 4.0] and prev[0] == 1.0 and live[0] == 1


@pytest.fixture(scope="module")
def fits():
    out = {}
    for name in DI.FIT_CASES:
        x, init, K = DI.planted(name)
        out[name] = DR.fit(x, init, max_iter=5, max_iter_barycenter=5)
    return out


@pytest.mark.parametrize("name", DI.FIT_CASES)
def test_fit_cases_decide_nothing_by_rounding(fits, name):
    r = fits[name]
    print(f"{name}: n_iter {r['n_iter']}, centre gap {r['centre_gap']:.2e}, path gap {r['path_gap']:.2e}, "
          f"steps {[s.tolist() for s in r['steps']]}")
    assert not r["empty"]
    assert r["centre_gap"] > DI.GAP and r["path_gap"] > DI.GAP


@pytest.mark.parametrize("name", [n for n in DI.CASES if n not in DI.FIT_CASES])
def test_round_cases_decide_nothing_by_rounding(name):
    """three assign-and-update rounds (one barycentre step each) on the two shapes that are not fitted whole"""
    x, init, K = DI.planted(name)
    r = DR.fit(x, init, max_iter=3, max_iter_barycenter=1, tol=0.0)
    print(f"{name}: centre gap {r['centre_gap']:.2e}, path gap {r['path_gap']:.2e}")
    assert not r["empty"] and r["n_iter"] == 3
    assert r["centre_gap"] > DI.GAP and r["path_gap"] > DI.GAP


def test_label_sets_are_what_the_device_test_needs():
    for name in DI.CASES:
        N, _, _, K = DI.CASES[name]
        sets = DI.label_sets(N, K, 3)
        assert np.mean(sets["heavy"] == K - 1) > 0.85
        assert not np.any(sets["holes"] == 1) and np.any(sets["holes"] < 0) and np.any(sets["holes"] >= K)


def test_cluster_latents_help_lists_old_and_new_options():
    run = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "cluster_latents.py"), "--help"], capture_output=True,
                         text=True, cwd=ROOT)
    assert run.returncode == 0, run.stderr
    text = " ".join(run.stdout.split())
    for opt in ("--checkpoint", "--chunks", "--n_clusters", "--max_iter", "--n_init", "--seed", "--check_every", "--scan-k",
                "--silhouette-rows", "--no-silhouette", "--out", "--algorithm", "{kmeans,dbscan}", "--distance-threshold", "--eps",
                "--min-samples", "--batch_rows", "--device"):
        assert opt in text, opt
    for opt in ("dtw", "--max-iter-barycenter"):
        assert opt in text, opt
