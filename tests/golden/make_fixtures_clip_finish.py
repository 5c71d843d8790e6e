"""Records scipy.signal.savgol_filter(x, 25, 5, axis=0) (mode="interp", scipy's default) once into clip_finish.npz, so that
tests/test_dec_chain_host.py can hold the Savitzky-Golay tables of g2v_clip_finish to it without importing scipy.
Run from the repository root: python tests/golden/make_fixtures_clip_finish.py"""
import os

import numpy as np
import scipy
from scipy.signal import savgol_filter

rng = np.random.RandomState(20240611)
x = rng.standard_normal((61, 4))
x[:, 1] = np.linspace(-1.0, 2.0, 61) ** 5          # a quintic: the filter reproduces it exactly, edges included
y = savgol_filter(x, 25, 5, axis=0)
np.savez(os.path.join(os.path.dirname(os.path.abspath(__file__)), "clip_finish.npz"), x=x, y=y,
         scipy_version=np.array(scipy.__version__))
