"""Seeded inputs of the pairwise-distance tests (tests/golden/make_fixtures_repdist.py records seeds, shapes, hashes and scalars in
tests/golden/repdist.npz; the rows are regenerated here).  Elementwise and sequential numpy only (no BLAS), so the fp32 arrays are
bit-stable; the fixture stores their sha256.  Every generator returns fp32 (N, E)."""
import hashlib

import numpy as np

# the shapes whose scipy / numpy values the fixture records; their seeds are searched from 0 and stored in the fixture
GENERIC = ((300, 400), (130, 33), (65, 3), (1100, 400))
SEQUENCE = (1100, 400)        # the reference's own run: N >= 1004, it samples 1000 of range(2, N - 2)
SEQUENCE_SEEDS = (5, 11)      # of the rows, of random.seed
HIST_BINS = 64


def name_of(shape):
    return "%dx%d" % shape


def clustered(N, E, seed, k=5):
    """k Gaussian blobs of unit spread around centres drawn 6 wide"""
    rng = np.random.default_rng(seed)
    centres = 6.0 * rng.normal(size=(k, E))
    which = rng.integers(0, k, N)
    return (centres[which] + rng.normal(size=(N, E))).astype(np.float32)


def sequence(N, E, seed, k=7):
    """rows that follow each other in time: a random walk of small steps inside segments that sit around k far-apart centres, so a
    row's temporal neighbours are much closer than a row picked at random"""
    rng = np.random.default_rng(seed)
    centres = 4.0 * rng.normal(size=(k, E))
    seg = np.minimum(np.arange(N) * k // N, k - 1)
    walk = np.cumsum(0.15 * rng.normal(size=(N, E)), axis=0)
    return (centres[seg] + walk + 0.3 * rng.normal(size=(N, E))).astype(np.float32)


def hist_hi(dmax):
    """the upper end of the recorded histograms' range: just above the largest distance, so that the largest pair is not on an edge"""
    return float(dmax) * (1.0 + 2.0 ** -10)


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
