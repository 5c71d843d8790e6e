"""Device-side DBSCAN (csrc/dbscan.hip, gesture2vec_amd/dbscan.py) against sklearn's recorded labels (tests/golden/dbscan.npz) and the
float64 rule (tests/_dbscan_ref.py): word and tile edges, ragged rows, a row stride, the edge rules, pairs planted at the threshold,
the chain input, repeatability, the row limit and scripts/cluster_latents.py --algorithm dbscan.

Every comparison is exact.  The device decides each pair on float64 arithmetic from the fp32 rows (the Gram form only where it is
outside the band around eps^2, sum (x_i - x_j)^2 inside it), and so does the rule; the two float64 sums differ in their order,
~1e-15 relative, and no input here has a pair that close to eps (the planted ones are 1e-8 away at the nearest)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import _dbscan_inputs as DI
import _dbscan_ref as DR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"

from gesture2vec_amd import ops  # noqa: E402
from gesture2vec_amd.dbscan import DBSCAN, check_rows  # noqa: E402


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "dbscan.npz"))


def _bits(bitmap):
    """(N, W) int64 device words -> (N, 64 W) bool"""
    b = np.ascontiguousarray(bitmap.cpu().numpy())
    return np.unpackbits(b.view(np.uint8), axis=1, bitorder="little").astype(bool)


def _check_fit(tag, X, eps, ms, xd=None, **kw):
    """labels, core indices, components, the three counts and the rounds of a fit against the rule"""
    ref = DR.fit(X, eps, ms)
    db = DBSCAN(eps=eps, min_samples=ms, **kw).fit(torch.from_numpy(X).to(DEV) if xd is None else xd)
    torch.cuda.synchronize()
    labels, core = db.labels_.cpu().numpy(), db.core_sample_indices_.cpu().numpy()
    print(f"{tag}: {int(ref['labels'].max()) + 1} clusters, {int(ref['core'].sum())} core, {int((ref['labels'] < 0).sum())} noise, "
          f"{db.n_rounds_} rounds (rule: {ref['rounds']})")
    assert db.labels_.dtype == torch.int64 and db.labels_.is_cuda and labels.shape == (X.shape[0],)
    assert np.array_equal(labels, ref["labels"])
    assert np.array_equal(core, np.nonzero(ref["core"])[0])
    assert np.array_equal(db.components_.cpu().numpy(), X[ref["core"]])
    assert db.n_clusters_ == int(ref["labels"].max()) + 1 and db.n_noise_ == int((ref["labels"] < 0).sum())
    assert db.n_features_in_ == X.shape[1] and db.n_rounds_ == ref["rounds"]
    assert np.array_equal(db._dev["counts"].cpu().numpy(), ref["counts"])
    return db, ref


# ---- 1. sklearn's recorded labels ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DI.FIXTURES)
def test_against_sklearn(fx, name):
    X, eps, ms = fx[f"{name}_x"], float(fx[f"{name}_eps"]), int(fx[f"{name}_min_samples"])
    db = DBSCAN(eps=eps, min_samples=ms).fit(torch.from_numpy(X).to(DEV))
    core = fx[f"{name}_core"].astype(np.int64)
    assert np.array_equal(db.labels_.cpu().numpy(), fx[f"{name}_labels"].astype(np.int64))
    assert np.array_equal(db.core_sample_indices_.cpu().numpy(), core)
    assert np.array_equal(db.components_.cpu().numpy(), X[core])
    assert db.fit_predict(torch.from_numpy(X).to(DEV)) is db.labels_


# ---- 2. word edges, tile edges, ragged rows, the 32-column chunk edge ---------------------------------------------------------------
@pytest.mark.parametrize("E", [1, 3, 31, 32, 33, 37, 400])
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 128, 129, 257])
def test_shapes_against_the_rule(N, E):
    X, eps, ms = DI.blobs(N, E, 1000 * E + N)
    _check_fit(f"N={N} E={E}", X, eps, ms)


def test_row_stride():
    """a column slice of a wider tensor (ld = 48 > E = 37) is read in place and gives the bits of the contiguous rows"""
    X, eps, ms = DI.blobs(129, 37, 9)
    wide = torch.randn(129, 48, device=DEV)
    wide[:, 4:41] = torch.from_numpy(X).to(DEV)
    view = wide[:, 4:41]
    assert view.stride(0) == 48 and view.data_ptr() % 16 == 0 and not view.is_contiguous()
    bm, cnt = ops.dbscan_neighbors(view, eps)
    pad = torch.zeros(129, 40, device=DEV)
    pad[:, :37] = view
    bm2, cnt2 = ops.dbscan_neighbors(pad[:, :37], eps)
    assert torch.equal(bm, bm2) and torch.equal(cnt, cnt2)
    _check_fit("ld=48 E=37", X, eps, ms, xd=view)


# ---- 3. edge rules ------------------------------------------------------------------------------------------------------------------
def test_edge_rules():
    X, eps, _ = DI.blobs(130, 40, 3)
    db, _ = _check_fit("min_samples=1", X, eps, 1)
    assert len(db.core_sample_indices_) == 130 and db.n_noise_ == 0 and int(db.labels_.min().item()) == 0
    db, _ = _check_fit("min_samples=N+1", X, eps, 131)
    assert db.n_clusters_ == 0 and db.n_noise_ == 130 and len(db.core_sample_indices_) == 0
    assert torch.equal(db.labels_, torch.full((130,), -1, dtype=torch.int64, device=DEV)) and db.components_.shape == (0, 40)
    db, _ = _check_fit("eps tiny", X, 1e-30, 1)
    assert db.n_clusters_ == 130 and torch.equal(db.labels_, torch.arange(130, device=DEV))
    dup = X.copy()
    dup[[7, 70, 129]] = dup[3]                                    # bitwise duplicates: d = 0 exactly, adjacent for any eps
    db, _ = _check_fit("duplicates", dup, 1e-30, 4)
    assert db.n_clusters_ == 1 and db.n_noise_ == 126 and list(db.core_sample_indices_.cpu().numpy()) == [3, 7, 70, 129]
    _check_fit("duplicates, shifted", dup + np.float32(30.0), 1e-30, 4)
    from gesture2vec_amd._lib import G2VLibraryError
    with pytest.raises(G2VLibraryError, match="E <= 512"):
        ops.dbscan_neighbors(torch.zeros(8, 516, device=DEV), 1.0)
    with pytest.raises(TypeError, match="fp32"):
        DBSCAN().fit(torch.zeros(8, 4, dtype=torch.float64, device=DEV))


# ---- 4. pairs at the threshold ------------------------------------------------------------------------------------------------------
def _plant(a, eps, rel, rng):
    """a row at float64 distance eps (1 + rel) from the fp32 row a, to within half of |rel| (the fp32 grid of the row moves the
    distance by ~6e-7 eps at entries of 30, so the direction is drawn until the rounded row lands there)"""
    a64 = a.astype(np.float64)
    for _ in range(200000):
        u = rng.normal(size=a.shape)
        b = (a64 + u * (eps * (1.0 + rel) / np.linalg.norm(u))).astype(np.float32)
        got = np.sqrt(((b.astype(np.float64) - a64) ** 2).sum()) / eps - 1.0
        if got * rel > 0 and 0.5 * abs(rel) <= abs(got) <= 1.5 * abs(rel):
            return b
    raise AssertionError("no row at the wanted distance")


@functools.lru_cache(maxsize=None)
def _threshold_rows(shift):
    rng = np.random.default_rng(77)
    X, eps, _ = DI.blobs(130, 37, 21)
    if shift is None:                                             # rows around the origin whose distances all lie around eps
        X = (rng.normal(size=X.shape) * eps / np.sqrt(2 * X.shape[1])).astype(np.float32)
    else:
        X = X + np.float32(shift)
    pairs = []
    for p in range(24):                                           # rows 5 p and 5 p + 1: in both row tiles that are full
        a, b = 5 * p, 5 * p + 1
        rel = (1e-6 if p < 12 else 1e-8) * (1 if p % 2 else -1)
        X[b] = _plant(X[a], eps, rel, rng)
        pairs.append((a, b, rel < 0))
    return X, eps, pairs


@pytest.mark.parametrize("shift", [30.0, 0.0, None])
def test_threshold_pairs(shift):
    """Rows shifted by 30 per column (the Gram form cancels: |x|^2 ~ 33000 against d^2 = 0.81) with pairs planted at float64 distance
    eps (1 +- 1e-6) and eps (1 +- 1e-8); the same without the shift; and (None) rows around the origin with d^2 ~ |x_i|^2 + |x_j|^2
    ~ eps^2 for every pair, which pd_tile leaves on the Gram form.  The adjacency read back from the bitmap and the counts equal the
    float64 decision for every pair.
    Checked on the device with DBS_BAND = 0 in csrc/dbscan.hip: all three cases fail.  Shifted and unshifted, 12 of 16 900 pairs and
    6 of the 24 planted ones differ, all of them planted at 1e-8 (pd_tile evaluates a near pair, d^2 < (n_i + n_j) / 8, from
    differences by itself and rounds it to fp32 once; that decides a pair at 1e-6 and not one inside an fp32 rounding of eps^2);
    around the origin 6 pairs and 3 of the planted ones differ."""
    X, eps, pairs = _threshold_rows(shift)
    want = DR.adjacency(X, eps)
    for a, b, inside in pairs:
        assert want[a, b] == inside and want[b, a] == inside
    pad = torch.zeros(X.shape[0], 40, device=DEV)                 # E = 37: a row stride of whole 16-byte vectors
    pad[:, :37] = torch.from_numpy(X).to(DEV)
    bitmap, counts = ops.dbscan_neighbors(pad[:, :37], eps)
    got = _bits(bitmap)
    N = X.shape[0]
    assert got.shape == (N, 64 * ((N + 63) // 64))
    wrong = np.argwhere(got[:, :N] != want)
    planted = sum(1 for a, b, inside in pairs if got[a, b] != inside or got[b, a] != inside)
    print(f"shift {shift}: {len(wrong)} of {N * N} pairs differ from the float64 decision, {planted} of {len(pairs)} planted pairs")
    assert len(wrong) == 0, wrong[:8]
    assert not got[:, N:].any()                                   # bits past N
    assert np.array_equal(got[:, :N], got[:, :N].T)
    assert np.array_equal(counts.cpu().numpy(), want.sum(1))


# ---- 5. the chain input, repeatability, the row limit ---------------------------------------------------------------------------------
def test_chains_converge_over_many_rounds(fx):
    X, eps, ms = fx["chains_x"], float(fx["chains_eps"]), int(fx["chains_min_samples"])
    db, ref = _check_fit("chains", X, eps, ms)
    assert db.n_rounds_ > 1 and db.n_clusters_ == 2
    one = DBSCAN(eps=eps, min_samples=ms, check_every=1).fit(torch.from_numpy(X).to(DEV))      # a read-back per round: the same bits
    assert one.n_rounds_ == db.n_rounds_ and torch.equal(one.labels_, db.labels_)


def test_same_call_twice_gives_the_same_bits():
    X, eps, ms = DI.blobs(257, 400, 4)
    xd = torch.from_numpy(X).to(DEV)
    runs = []
    for _ in range(2):
        bitmap, counts = ops.dbscan_neighbors(xd, eps)
        db = DBSCAN(eps=eps, min_samples=ms).fit(xd)
        runs.append((bitmap, counts, db.labels_, db.core_sample_indices_, db.n_rounds_))
    for a, b in zip(*runs):
        assert torch.equal(a, b) if torch.is_tensor(a) else a == b


def test_row_limit_is_refused_without_allocating():
    limit = ops.dbscan_max_rows()
    assert limit == 131072
    assert ops.dbscan_workspace(limit, 400) > 0 and ops.dbscan_workspace(limit + 1, 400) == 0
    assert ops.dbscan_workspace(0, 400) == 0 and ops.dbscan_workspace(64, 513) == 0 and ops.dbscan_workspace(64, 0) == 0
    check_rows(limit)
    with pytest.raises(ValueError, match=str(limit)):
        check_rows(limit + 1)


# ---- 6. scripts/cluster_latents.py --algorithm dbscan --------------------------------------------------------------------------------
def test_cluster_latents_dbscan(golden_dir, tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import cluster_latents
    from utils.train_utils import load_checkpoint_and_model
    ckpt = os.path.join(golden_dir, "plain_ae_ckpt.bin")
    args, net, _, _, pose_dim = load_checkpoint_and_model(ckpt, DEV, "autoencoder_vq")
    net.eval()
    real = torch.randn(300, int(args.n_poses), pose_dim, generator=torch.Generator().manual_seed(5))
    np.save(tmp_path / "chunks.npy", real.numpy())
    lat = cluster_latents.latents_of(net, real.to(DEV), 65536).cpu().numpy()
    d = np.sqrt(DR.sq_distances(lat))
    eps = float(np.quantile(d[~np.eye(len(d), dtype=bool)], 0.02))  # 2 % of the pairs are neighbours
    ref = DR.fit(lat, eps, 4)
    out = tmp_path / "db.npz"
    db = cluster_latents.main(["--checkpoint", ckpt, "--chunks", str(tmp_path / "chunks.npy"), "--device", DEV, "--algorithm", "dbscan",
                               "--eps", repr(eps), "--min-samples", "4", "--out", str(out)])
    printed = capsys.readouterr().out
    n_clusters, n_noise = int(ref["labels"].max()) + 1, int((ref["labels"] < 0).sum())
    assert f"Estimated number of clusters: {n_clusters}\n" in printed and f"Estimated number of noise points: {n_noise}\n" in printed
    saved = np.load(out)
    assert np.array_equal(saved["labels"], ref["labels"]) and np.array_equal(saved["core"], ref["core"])
    assert np.array_equal(db.labels_.cpu().numpy(), ref["labels"])
