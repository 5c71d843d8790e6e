"""Joint angles from generated clips, the part that needs no GPU: the float64 restatements of tests/_clip_angles_ref.py against
what scipy 1.15.3 recorded into tests/golden/clip_angles.npz (tests/golden/make_fixtures_clip_angles.py), the smoothing spline's
system against two independent statements of its limits, and the Python surface's refusals and exports.

What is NOT held here or anywhere: a recorded run of csaps or of scipy 1.10.1.  Neither is installed where the fixture is recorded.
csaps' spline is checked through its definition (de Boor's system, which equals scipy's make_smoothing_spline at lam = (1-p)/p);
scipy 1.10.1's from_matrix (Markley on the raw matrix) is checked on exact rotations, where it agrees with the recorded version."""
import os

import numpy as np
import pytest
import torch

import _clip_angles_ref as R

SPLINE_F = (5, 6, 34, 340)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "clip_angles.npz"))


def test_fixture_inputs_are_the_shared_recipe_and_inside_the_conditions(fx):
    assert np.array_equal(fx["noisy"], R.noisy_matrices(512, 20240917)) and np.array_equal(fx["exact"], R.branch_matrices())
    assert (np.linalg.det(fx["noisy"].astype(np.float64)) > 0).all()
    for method in R.METHODS:
        assert (np.abs(R.euler_zxy(fx["noisy"], method)[:, 1]) < R.X_MAX_HELD).all()
    assert (np.abs(fx["noisy_zxy"][:, 1]) < R.X_MAX_HELD).all()


def test_procrustes_restatement_matches_scipy(fx):
    err = R.angle_diff(R.euler_zxy(fx["noisy"], "procrustes"), fx["noisy_zxy"])
    print(f"procrustes restatement against scipy {fx['scipy_version']}: {err.max():.2e} degrees over {err.shape[0]} matrices")
    assert err.max() <= 1e-9


def test_markley_restatement_matches_scipy_on_exact_rotations(fx):
    assert set(R.markley_branch(fx["exact"]).tolist()) == {0, 1, 2, 3}
    for method in R.METHODS:
        err = R.angle_diff(R.euler_zxy(fx["exact"], method), fx["exact_zxy"])
        assert err.max() <= 1e-9, (method, err.max())
    # ... and on decoder-like matrices the two are different functions: which is why both are offered
    diff = R.angle_diff(R.euler_zxy(fx["noisy"], "markley"), fx["noisy_zxy"])
    assert np.median(diff) > 0.1


def test_lock_rule_and_inverse():
    lock = R.zxy_matrix(np.array([(0, 90, 0), (90, 90, 0), (180, -90, 0), (-90, -90, 0)], dtype=np.float64)).round() + 0.0
    assert np.array_equal(lock[0], [[1, 0, 0], [0, 0, -1], [0, 1, 0]]) and np.array_equal(lock[1], [[0, 0, 1], [1, 0, 0], [0, 1, 0]])
    for method in R.METHODS:
        a = R.euler_zxy(lock, method)
        assert (a[:, 2] == 0).all() and np.abs(np.abs(a[:, 1]) - 90).max() <= 1e-9
        assert np.abs(R.zxy_matrix(a) - lock).max() <= 1e-12
    ang = np.random.RandomState(3).uniform(-1, 1, (200, 3)) * np.array([180.0, 89.0, 180.0])
    assert R.angle_diff(R.euler_zxy(R.zxy_matrix(ang), "markley"), ang).max() <= 1e-9
    bad = np.stack([np.zeros((3, 3)), np.diag([1.0, 1.0, -1.0]), np.eye(3)])
    a = R.euler_zxy(bad, "procrustes")
    assert np.isnan(a[:2]).all() and np.array_equal(a[2], np.zeros(3))


def test_spline_restatement_matches_scipy(fx):
    for F in SPLINE_F:
        y, s = fx[f"spline_y_{F}"], fx[f"spline_s_{F}"]
        assert np.array_equal(y, R.spline_data(F, 4, 1000 + F)) and np.abs(y).max() <= 180.0
        for solver in (R._solve_dense, R._solve_banded):
            err = np.abs(R.smoothing_spline(y, 0.5, solver=solver) - s).max()
            assert err <= 1e-9, (F, solver.__name__, err)


def test_spline_limits_and_small_systems():
    x = np.arange(40.0)
    y = R.spline_data(40, 5, 7).astype(np.float64)
    line = np.stack([np.polyval(np.polyfit(x, y[:, c], 1), x) for c in range(5)], axis=1)
    assert np.abs(R.smoothing_spline(y, 0.0) - line).max() <= 1e-9             # p = 0: the least-squares straight line
    assert np.array_equal(R.smoothing_spline(y, 1.0), y)                       # p = 1: interpolation
    assert np.array_equal(R.smoothing_spline(y[:2], 0.5), y[:2])               # F = 2: no unknowns
    flat = np.stack([3.0 * x - 50.0, np.full(40, 33.25)], axis=1)               # a line and a constant have no curvature to remove
    assert np.abs(R.smoothing_spline(flat, 0.5) - flat).max() <= 1e-9
    for F in (3, 4, 5, 1500):                                                  # the truncated bands; past DENSE_MAX the banded solver
        yy = R.spline_data(F, 3, F).astype(np.float64)
        banded = R.smoothing_spline(yy, 0.5, solver=R._solve_banded)
        assert np.abs(banded - R.smoothing_spline(yy, 0.5, solver=R._solve_dense)).max() <= 1e-9
        if F - 2 > R.DENSE_MAX:
            assert np.array_equal(banded, R.smoothing_spline(yy, 0.5))
    t = np.moveaxis(np.stack([y, 2 * y]), 1, 2)                                # (2, 5, 40): the axis argument
    assert np.array_equal(R.smoothing_spline(t, 0.5, axis=2)[1].T, R.smoothing_spline(2 * y, 0.5))


class _Cuda:                                           # shapes and flags only: the refusals come before any launch
    is_cuda = True

    def __init__(self, *shape):
        self.shape = shape

    def dim(self):
        return len(self.shape)


def test_python_refusals():
    from gesture2vec_amd import generate as G
    for call in (lambda: G.rotmat_to_euler(torch.zeros(4, 18)), lambda: G.smoothing_spline(torch.zeros(1, 8, 3)),
                 lambda: G.clip_angles(torch.zeros(1, 8, 9)), lambda: G.clip_angles(torch.zeros(1, 8, 9), spline=None)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="nearest"):
        G.rotmat_to_euler(_Cuda(4, 18), nearest="svd")
    with pytest.raises(ValueError, match="nearest"):
        G.clip_angles(_Cuda(1, 4, 18), nearest="horn")
    for shape in ((4, 17), (4, 0), (2, 3, 10), ()):
        with pytest.raises(ValueError, match="9 entries per joint"):
            G.rotmat_to_euler(_Cuda(*shape))
    for smooth in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            G.smoothing_spline(_Cuda(1, 8, 3), smooth)
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            G.clip_angles(_Cuda(1, 8, 9), spline=smooth)
    for shape in ((8, 3), (1, 1, 3), (0, 8, 3), (1, 8, 0), (1, 2, 8, 3)):
        with pytest.raises(ValueError, match="smoothing_spline"):
            G.smoothing_spline(_Cuda(*shape))
    with pytest.raises(ValueError, match="clip_angles"):
        G.clip_angles(_Cuda(8, 9))
    assert G.NEAREST == ("markley", "procrustes") and G.SPLINE_SMOOTH == 0.5


def test_exports_constants_and_host_side_answers():
    from gesture2vec_amd import _lib, ops
    for name in ("g2v_rotmat_to_euler", "g2v_smoothing_spline", "g2v_smoothing_spline_workspace"):
        assert name in _lib.EXPORTS
    assert (_lib.ROT_MARKLEY, _lib.ROT_PROCRUSTES) == (0, 1) and ops.ROT_METHODS == {"markley": 0, "procrustes": 1}
    ws = _lib.load().g2v_smoothing_spline_workspace
    assert ws(1, 2, 1) == 0 and ws(0, 10, 3) == 0 and ws(1, 10, 0) == 0 and ws(1, 1, 1) == 0
    assert ws(1, 3, 1) == 8 * 4 and ws(4096, 204, 45) == 8 * 202 * (3 + 4096 * 45) and ws(1, 1 << 20, 3) == 8 * 6 * ((1 << 20) - 2)
    assert ws(1, (1 << 20) + 1, 3) == 0 and ws(1 << 16, 10, 1 << 15) == 0


def test_script_options_parse():
    import importlib
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    gg = importlib.import_module("generate_gestures")
    assert gg._smooth_arg("none") is None and gg._smooth_arg("None") is None and gg._smooth_arg("0.25") == 0.25
    import argparse
    for text in ("1.5", "-1"):
        with pytest.raises(argparse.ArgumentTypeError):
            gg._smooth_arg(text)
