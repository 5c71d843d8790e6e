"""Case tables and inputs of the codebook-update tests (tests/test_gpu_vq_update_f64.py, tests/test_vq_update_ref_host.py).

Shapes are (N, E, K): rows, row width, codes.  Every fact a table states about a case is a plain field here and is asserted from
arithmetic by the host test (a restatement of the launchers' constants in gesture2vec_amd/csrc/vq.hip, g2v_vq_stats), so that an
edited table cannot go stale; the GPU test asserts the route the call really took (see there).  Inputs are numpy, seeded by the
shape, float32 and int64 exactly as the device receives them."""
import functools
import zlib

import numpy as np

# ---- the launchers' constants, restated (vq.hip: g2v_vq_stats, stats_splits, vq_stats_kernel, vq_stats_owner_kernel) -----------
OWNER_MIN_ROWS = 1024        # tile-owner kernel from this many rows ...
OWNER_MIN_TILES = 128        # ... and this many 16 x 16 tiles of the (K, E) result
OWNER_BATCH = 64             # rows a wave requests per loop iteration (8 U, U = 8 groups of 4 rows, two batches in flight)
SLAB_CHUNK = 32              # SM: rows per chunk of the slab kernel
SLAB_TILE = 64               # codes x columns per workgroup of the slab kernel
SLAB_WORKGROUPS = 512        # the slab launch aims at this many workgroups
GRID_CAP = 2048 * 256        # elements one pass of the element-wise launchers covers (vq_bwd, codebook_grad, ste)


def cdiv(a, b):
    return -(-a // b)


def owner_route(N, E, K):
    return E % 16 == 0 and K % 16 == 0 and N >= OWNER_MIN_ROWS and (K // 16) * (E // 16) >= OWNER_MIN_TILES


def owner_rows_per_wave(N):
    """rows each of the four waves walks: ceil(N / 4) rounded up to a multiple of 4"""
    return (cdiv(N, 4) + 3) & ~3


def slab_tiles(E, K):
    return cdiv(K, SLAB_TILE) * cdiv(E, SLAB_TILE)


def slab_splits(N, E, K):
    return max(1, min(cdiv(SLAB_WORKGROUPS, slab_tiles(E, K)), cdiv(N, 2 * SLAB_CHUNK)))


def slab_rows_per_split(N, E, K):
    return cdiv(cdiv(N, slab_splits(N, E, K)), SLAB_CHUNK) * SLAB_CHUNK


def slab_last_split_rows(N, E, K):
    """rows the last split holds (<= 0: it holds none)"""
    return N - (slab_splits(N, E, K) - 1) * slab_rows_per_split(N, E, K)


# ---- statistics: (N, E, K) -> the facts claimed about the case ---------------------------------------------------------------
# owner: which kernel g2v_vq_stats picks.  rem16: N % 16 (the owner kernel's row split went wrong at 1, 2, 3).
# tiles16: (K / 16)(E / 16).  splits / last: the slab kernel's split count and the rows its last split holds.
STATS_OWNER = {
    (1024, 128, 256): dict(owner=True, rem16=0, tiles16=128),          # both thresholds met exactly
    (1025, 128, 256): dict(owner=True, rem16=1, tiles16=128),          # ceil(N / 4) = 257 > (N / 4 + 3) & ~3 = 256
    (1026, 128, 256): dict(owner=True, rem16=2, tiles16=128),
    (1027, 128, 256): dict(owner=True, rem16=3, tiles16=128),
    (1028, 128, 256): dict(owner=True, rem16=4, tiles16=128),
    (1039, 128, 256): dict(owner=True, rem16=15, tiles16=128),
    (1100, 128, 256): dict(owner=True, rem16=12, tiles16=128, ragged_batch=True),   # 276 rows per wave = 4 x 64 + 20
    (4099, 128, 512): dict(owner=True, rem16=3, tiles16=256),
    (1024, 400, 512): dict(owner=True, rem16=0, tiles16=800, column_tiles=25),
}
STATS_NEAR_MISS = {
    (1023, 128, 256): dict(owner=False, tiles16=128),                  # one row short
    (1024, 128, 240): dict(owner=False, tiles16=120),                  # eight tiles short
    (1024, 120, 512): dict(owner=False, e_rem16=8),                    # E % 16 != 0
    (1024, 128, 264): dict(owner=False, k_rem16=8),                    # K % 16 != 0
}
STATS_SLAB = {
    (1, 1, 1): dict(owner=False, splits=1, last=1),
    (33, 100, 7): dict(owner=False, splits=1, last=33),                # two chunks, the second holding one row
    (64, 64, 64): dict(owner=False, splits=1, last=64),                # one whole tile, two whole chunks
    (65, 65, 65): dict(owner=False, splits=2, last=1),                 # four tiles with one code / column in the outer ones
    (100, 100, 512): dict(owner=False, splits=2, last=36),
    (130, 48, 80): dict(owner=False, splits=3, last=2),
    (2049, 48, 80): dict(owner=False, splits=33, last=1),
    # A last split that holds NO row exists: splits is capped by the tile count while rows_per_split is rounded up to 32, e.g.
    # 128 tiles -> 4 splits, N = 257 -> ceil(257 / 4) = 65 -> 96 rows per split, 3 x 96 = 288 >= 257 (the host test searches for
    # such shapes and finds this one).  That split's workgroups run no chunk and store zeros.
    (257, 1024, 512): dict(owner=False, splits=4, last=-31),
}
STATS_CASES = {**STATS_OWNER, **STATS_NEAR_MISS, **STATS_SLAB}
ID_KINDS = ("random", "collapsed")
ADDITIVITY = {(1026, 128, 256): (513, 513), (100, 100, 512): (36, 64)}

BIG_ROWS = 3                 # the last rows carry magnitudes well above the rest: a dropped row cannot hide inside a sum's bar
BIG_SCALE = 64.0


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def collapsed_code(K):
    return min(3, K - 1)      # every row to code 3 (the last code where the codebook has fewer than four)


def empty_code(K):
    return K // 2 if K >= 2 else None      # the code the random ids never use (K = 1: a single code cannot be empty)


@functools.lru_cache(maxsize=None)
def stats_inputs(N, E, K, kind):
    """(idx int64 (N,), flat float32 (N, E)); read-only"""
    rng = np.random.default_rng(_seed("stats", N, E, K))
    flat = rng.standard_normal((N, E)).astype(np.float32)
    flat[max(0, N - BIG_ROWS):] *= np.float32(BIG_SCALE)
    if kind == "collapsed":
        idx = np.full(N, collapsed_code(K), dtype=np.int64)
    else:
        idx = rng.integers(0, K, N).astype(np.int64)
        dead = empty_code(K)
        if dead is not None:
            idx[idx == dead] = (dead + 1) % K
    idx.setflags(write=False)
    flat.setflags(write=False)
    return idx, flat


# ---- EMA update ----------------------------------------------------------------------------------------------------------------
EMA_CASES = [(1, 1), (100, 7), (128, 257), (400, 512), (128, 512)]      # (E, K)
EMA_DECAYS = [0.85, 0.99]
EMA_N_SSE = [1, 7, 300]           # > 256: the strided loop of the one-workgroup scalars kernel runs twice
EMA_THREADS = 256
BETA, EPS = 0.25, 1e-5


@functools.lru_cache(maxsize=None)
def ema_inputs(E, K, n_sse, zero_ema_w=False):
    """stats = [cnt (K) | dw (K, E)] as the statistics kernels leave them, the EMA state before the step, sse partials, and the
    two row counts as the data-parallel step passes them: N_cnt the global number of rows (the counts are global), N_loss this
    rank's.  Dead codes (every fifth, from code 1): no row now and cluster size 0 before."""
    rng = np.random.default_rng(_seed("ema", E, K))
    cnt = rng.integers(0, 10, K).astype(np.float32)
    dead = np.arange(K) % 5 == 1
    cnt[dead] = 0
    cnt[0] = max(cnt[0], 6)
    dw = (rng.standard_normal((K, E)) * np.sqrt(np.maximum(cnt, 1))[:, None]).astype(np.float32)
    dw[cnt == 0] = 0
    cs = (rng.random(K) * 5).astype(np.float32)
    cs[dead] = 0
    ema_w = np.zeros((K, E), np.float32) if zero_ema_w else rng.standard_normal((K, E)).astype(np.float32)
    sse = np.random.default_rng(_seed("sse", n_sse)).random(n_sse).astype(np.float32)
    N_cnt = int(cnt.sum())
    N_loss = N_cnt // 2
    out = dict(cnt=cnt, dw=dw, cs=cs, ema_w=ema_w, sse=sse, N_cnt=N_cnt, N_loss=N_loss, dead=dead)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ---- vq_bwd, codebook gradient, code norms, straight-through value -------------------------------------------------------------
BWD_CASES = {      # (N, E, K) -> passes of the grid-stride loop
    (33, 100, 64): dict(passes=1, rem256=228),
    (300, 128, 64): dict(passes=1, rem256=0),
    (4096, 128, 512): dict(passes=1, rem256=0, exactly_cap=True),
    (4100, 128, 512): dict(passes=2, rem256=0),
}
G_LOSS = 1.0 / 400.0


@functools.lru_cache(maxsize=None)
def bwd_inputs(N, E, K):
    rng = np.random.default_rng(_seed("bwd", N, E, K))
    z = rng.standard_normal((N, E)).astype(np.float32)
    W = rng.standard_normal((K, E)).astype(np.float32)
    gq = rng.standard_normal((N, E)).astype(np.float32)
    idx = rng.integers(0, K, N).astype(np.int64)
    out = dict(z=z, W=W, gq=gq, idx=idx, dense=W[idx].copy(), gl=np.array([G_LOSS], np.float32))
    for v in out.values():
        v.setflags(write=False)
    return out


CBGRAD_CASES = {(100, 7): dict(passes=1), (128, 512): dict(passes=1), (400, 1320): dict(passes=2)}      # (E, K)
CBGRAD_ROWS = 300
SQNORM_CASES = [(1, 1), (5, 63), (5, 64), (5, 65), (7, 400), (512, 128)]      # (K, E); four codes per workgroup
STE_COUNTS = [1, 255, 257, GRID_CAP + 1]


@functools.lru_cache(maxsize=None)
def cbgrad_inputs(E, K):
    """a real assignment of CBGRAD_ROWS rows that leaves a code empty: (idx, flat)"""
    rng = np.random.default_rng(_seed("cbgrad", E, K))
    idx = rng.integers(0, K, CBGRAD_ROWS).astype(np.int64)
    idx[idx == empty_code(K)] = (empty_code(K) + 1) % K
    flat = rng.standard_normal((CBGRAD_ROWS, E)).astype(np.float32)
    idx.setflags(write=False)
    flat.setflags(write=False)
    return idx, flat


@functools.lru_cache(maxsize=None)
def codebook(K, E):
    W = np.random.default_rng(_seed("codebook", K, E)).standard_normal((K, E)).astype(np.float32)
    W.setflags(write=False)
    return W


@functools.lru_cache(maxsize=None)
def ste_inputs(n):
    rng = np.random.default_rng(_seed("ste", n))
    z, q = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    z.setflags(write=False)
    q.setflags(write=False)
    return z, q
