"""Inputs of the metrics fixture (tests/golden/metrics.npz), regenerated identically by tests/golden/make_fixtures_metrics.py and
by the tests: elementwise and sequential numpy only (no BLAS), so the float32 arrays are bit-stable; the fixture stores their
sha256."""
import hashlib

import numpy as np

# (N1, N2, E): both sets have more rows than columns, where the reference's sqrtm stays real and finite
FRECHET_CASES = {"wide": (4096, 3000, 400), "narrow": (1024, 1536, 128)}
SEEDS, SCALES, OFFSETS = (1, 2), (0.1, 0.11), (0.3, 0.25)
HIST_K = 512
HIST_CASES = {"a": (11, 12, 5000, 7000), "b": (21, 22, 300, 100000)}        # seed1, seed2, n1, n2


def latent_set(seed: int, N: int, E: int, scale: float, offset: float) -> np.ndarray:
    return (np.cumsum(np.random.RandomState(seed).randn(N, E), axis=1) * scale + offset).astype(np.float32)


def frechet_inputs(case: str):
    n1, n2, E = FRECHET_CASES[case]
    return (latent_set(SEEDS[0], n1, E, SCALES[0], OFFSETS[0]), latent_set(SEEDS[1], n2, E, SCALES[1], OFFSETS[1]))


def code_ids(seed: int, n: int, K: int = HIST_K) -> np.ndarray:
    """ids drawn from a peaked distribution over a third of the bins: many bins stay empty"""
    r = np.random.RandomState(seed)
    live = r.permutation(K)[:K // 3]
    return live[np.minimum((r.exponential(size=n) * len(live) / 4).astype(np.int64), len(live) - 1)].astype(np.int64)


def hist_inputs(case: str):
    s1, s2, n1, n2 = HIST_CASES[case]
    return code_ids(s1, n1), code_ids(s2, n2)


def sha256(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
