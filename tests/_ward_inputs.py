"""Seeded inputs of the Ward tests (tests/golden/make_fixtures_ward.py records the fixture's rows themselves in tests/golden/ward.npz;
the GPU distance tests draw from here).  Every generator returns X fp32 (N, E)."""
import numpy as np

FIXTURES = ("blobs_193x37", "blobs_257x3", "blobs_300x400", "chain", "noise_65x3")
KS = {"blobs_193x37": (2, 5, 9), "blobs_257x3": (3, 4, 17), "blobs_300x400": (2, 6, 30), "chain": (2, 3, 7), "noise_65x3": (2, 8, 33)}
THRESHOLD_ON = "blobs_193x37"      # the input of the one distance_threshold fit
REL_GAP = 1e-7        # a row's best and second-best neighbour, and consecutive sorted heights, differ by more than this, relative:
                      # four orders above the float64 arithmetic's noise, so neither sklearn's rounding nor the device's decides a merge


def blobs(N, E, seed, k=5):
    """k Gaussian blobs of unit spread around centres drawn 6 wide"""
    rng = np.random.default_rng(seed)
    centres = 6.0 * rng.normal(size=(k, E))
    which = rng.integers(0, k, N)
    return (centres[which] + rng.normal(size=(N, E))).astype(np.float32)


def chain(seed=0, n=40, E=5, growth=1.5):
    """n rows along the first column whose gaps grow by `growth` from one to the next, shuffled: a row's nearest neighbour is the one
    on its short side, so a round finds few mutual pairs and the rounds outrun `check_every` several times"""
    rng = np.random.default_rng(seed)
    X = np.zeros((n, E))
    X[:, 0] = np.concatenate([[0.0], np.cumsum(growth ** np.arange(n - 1))])
    X[:, 1:] = 0.05 * rng.normal(size=(n, E - 1))
    return X[rng.permutation(n)].astype(np.float32)


def noise(N, E, seed):
    return np.random.default_rng(seed).normal(size=(N, E)).astype(np.float32)
