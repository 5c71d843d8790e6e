"""Records, with the scipy installed where this is run, what tests/test_clip_angles_host.py and tests/test_gpu_clip_angles.py hold
the joint-angle code (csrc/clip_angles.hip, tests/_clip_angles_ref.py) to, into clip_angles.npz:

  noisy (512, 3, 3) float32      Rz Rx Ry with X in [-70, 70] degrees plus Gaussian noise of 0.05 (tests/_clip_angles_ref.noisy_matrices)
  noisy_zxy (512, 3) float64     Rotation.from_matrix(noisy).as_euler("ZXY", degrees=True): scipy >= 1.15 orthogonalises first
  exact (12, 3, 3) float64       exact rotations that reach all four Markley branches;  exact_zxy (12, 3): the same call on them
  spline_y_F (F, 4) float32, spline_s_F (F, 4) float64 for F in SPLINE_F: data within [-180, 180] and
                                 make_smoothing_spline(x, y, lam=1)(x) per column (= csaps' smooth = 0.5)

and asserts the conditions the angle-by-angle comparison of the tests rests on, for EVERY noisy row under BOTH methods: determinant
> 0 and |X| < 80 degrees (away from the lock, where Z and Y are well conditioned).
Run from the repository root: python tests/golden/make_fixtures_clip_angles.py"""
import os
import sys
import warnings

import numpy as np
import scipy
from scipy.interpolate import make_smoothing_spline
from scipy.spatial.transform import Rotation

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _clip_angles_ref as R  # noqa: E402

SPLINE_F = (5, 6, 34, 340)

noisy = R.noisy_matrices(512, 20240917)
assert (np.linalg.det(noisy.astype(np.float64)) > 0).all()
for method in R.METHODS:
    assert (np.abs(R.euler_zxy(noisy, method)[:, 1]) < R.X_MAX_HELD).all(), method
noisy_zxy = Rotation.from_matrix(noisy.astype(np.float64)).as_euler("ZXY", degrees=True)
assert (np.abs(noisy_zxy[:, 1]) < R.X_MAX_HELD).all()
exact = R.branch_matrices()
assert set(R.markley_branch(exact).tolist()) == {0, 1, 2, 3}
with warnings.catch_warnings():
    warnings.simplefilter("error")                           # no row of `exact` is at the lock
    exact_zxy = Rotation.from_matrix(exact).as_euler("ZXY", degrees=True)
out = dict(noisy=noisy, noisy_zxy=noisy_zxy, exact=exact, exact_zxy=exact_zxy, scipy_version=np.array(scipy.__version__))
for F in SPLINE_F:
    y = R.spline_data(F, 4, 1000 + F)
    assert np.abs(y).max() <= 180.0
    x = np.arange(F, dtype=np.float64)
    out[f"spline_y_{F}"] = y
    out[f"spline_s_{F}"] = np.stack([make_smoothing_spline(x, y[:, c].astype(np.float64), lam=1.0)(x) for c in range(y.shape[1])], axis=1)
np.savez_compressed(os.path.join(HERE, "clip_angles.npz"), **out)
