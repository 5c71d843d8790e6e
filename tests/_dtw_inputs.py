"""Seeded inputs of the DTW tests.  `planted`: K prototypes = tanh of a random walk over time; a row is a prototype read at sorted
random time indices with the end points kept (the same gesture at another speed) plus Gaussian noise 0.15, cast to fp32; the init
is K rows of a seeded permutation.  `exact`: integer-valued series in {-2 .. 2}, constant series and repeated rows included: every
operation on them is exact in float64 and ties are everywhere."""
import numpy as np

# name -> (N, T, F, K); the seed is the position in this list
CASES = {"n150": (150, 10, 8, 5), "n300": (300, 20, 40, 7), "n200": (200, 34, 12, 6), "t64": (96, 64, 4, 3), "f135": (64, 17, 135, 4)}
FIT_CASES = ("n150", "n300", "n200")         # whole fits; the other two serve three assign-and-update rounds
NOISE = 0.15
GAP = 1e-9                                   # what the host test asks of every decision before the device is asked for equality


def _prototypes(rs, K, L, F):
    return np.tanh(np.cumsum(rs.normal(0.0, 0.35, size=(K, L, F)), axis=1))


def _warp(rs, proto, T):
    L = proto.shape[0]
    idx = np.sort(rs.randint(0, L, size=T))
    idx[0], idx[-1] = 0, L - 1
    return proto[idx]


def series(N, T, F, K, seed, L=None):
    """(x (N, T, F) fp32, the planted cluster of every row)"""
    rs = np.random.RandomState(1000 + seed)
    protos = _prototypes(rs, K, L or 2 * T, F)
    which = rs.randint(0, K, size=N)
    which[:K] = np.arange(K)
    x = np.stack([_warp(rs, protos[k], T) for k in which]) + rs.normal(0.0, NOISE, size=(N, T, F))
    return x.astype(np.float32), which


def planted(name):
    """-> (x (N, T, F) fp32, init (K, T, F) float64: K rows of a seeded permutation, K)"""
    N, T, F, K = CASES[name]
    seed = list(CASES).index(name)
    x, _ = series(N, T, F, K, seed)
    rows = np.random.RandomState(seed).permutation(N)[:K]
    return x, x[rows].astype(np.float64), K


def fresh(name, N, T):
    """N new rows of the case's prototypes at another length T"""
    _, T0, F, K = CASES[name]
    seed = list(CASES).index(name)
    rs = np.random.RandomState(1000 + seed)
    protos = _prototypes(rs, K, 2 * T0, F)
    rs = np.random.RandomState(5000 + seed)
    x = np.stack([_warp(rs, protos[k], T) for k in rs.randint(0, K, size=N)]) + rs.normal(0.0, NOISE, size=(N, T, F))
    return x.astype(np.float32)


def random_pair(N, M, T, S, F, seed):
    """x (N, T, F) fp32 and y (M, S, F) float64 (not fp32-valued), smooth walks"""
    rs = np.random.RandomState(seed)
    x = np.tanh(np.cumsum(rs.normal(0.0, 0.4, size=(N, T, F)), axis=1)).astype(np.float32)
    y = np.tanh(np.cumsum(rs.normal(0.0, 0.4, size=(M, S, F)), axis=1)) + rs.normal(0.0, 0.05, size=(M, S, F))
    return x, y


def exact(N, T, F, seed):
    """integer-valued fp32 series in {-2 .. 2}: row 1 constant, row 2 all zero, the last row a copy of row 0"""
    rs = np.random.RandomState(seed)
    x = rs.randint(-2, 3, size=(N, T, F)).astype(np.float32)
    if N > 1:
        x[1] = 1.0
    if N > 2:
        x[2] = 0.0
    if N > 3:
        x[-1] = x[0]
    return x


def label_sets(N, K, seed):
    """the three label sets of the accumulate test: uniform; one cluster with 90 % of the rows; unused ids and ids outside [0, K)"""
    rs = np.random.RandomState(seed)
    uniform = rs.randint(0, K, size=N).astype(np.int64)
    heavy = np.where(rs.uniform(size=N) < 0.9, K - 1, rs.randint(0, K, size=N)).astype(np.int64)
    holes = rs.randint(0, K, size=N).astype(np.int64)
    holes[holes == 1] = 0                                         # id 1 is unused
    holes[::7] = -1
    holes[3::11] = K
    holes[5::13] = K + 5
    return {"uniform": uniform, "heavy": heavy, "holes": holes}
