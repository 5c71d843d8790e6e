"""Trustworthiness and continuity of a map on the device (csrc/map_quality.hip, gesture2vec_amd/embedding.py: kneighbors,
trustworthiness, continuity, map_quality, placement_quality; dbscan.k_distances) against the float64 restatement
(tests/_mapq_ref.py) and sklearn's recorded numbers (tests/golden/mapquality.npz).

Bars.  Ranks, neighbour lists and penalties are integers: equal on every entry of every row.  Both scores are formed from the same
integer sum by the same float64 expression: 1e-15 relative; and within 1e-12 of sklearn's recorded number.  That holds on inputs
that meet the preconditions of _mapq_ref (the selection's documented margin (a), no two compared float64 distances within 1e-12
relative (b)); every test asserts them on the host before it compares.  The count of pairs decided again lies between the pairs
that must be (within (BAND - 34 * 2^-24) (n_i + n_j) of a threshold in float64) and those that may be (BAND + 34 * 2^-24).
k_distances: 2e-6 relative (the selection's 3e-7 (|z|^2 + |x|^2) against d^2 >= (|z|^2 + |x|^2) / 8 of a pair on the Gram form is
2.4e-6 on d^2, half that on d); bitwise on the integer grid."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import _mapq_ref as MR
from _tsne_ref import sqdist

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(DEV)


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _fx():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "mapquality.npz")))


@functools.lru_cache(maxsize=None)
def _generic(shape):
    """inputs, the restatement and the preconditions of one generic shape (computed once)"""
    fx, name, k = _fx(), MR.name_of(shape), shape[2]
    X, Y = fx[f"{name}_x"], fx[f"{name}_y"]
    ref = MR.map_quality(X, Y, k)
    me = np.arange(X.shape[0])
    pre = {"a": (MR.selection_margin(X, k), MR.selection_margin(Y, k)),
           "b": (MR.closest_compared(sqdist(X), ref["nn_y"], me), MR.closest_compared(sqdist(Y), ref["nn_x"], me)),
           "band_t": MR.band_pairs(X, X, ref["nn_y"], me), "band_c": MR.band_pairs(Y, Y, ref["nn_x"], me)}
    return X, Y, k, ref, pre, float(fx[f"{name}_trust"]), float(fx[f"{name}_cont"])


@functools.lru_cache(maxsize=None)
def _exact():
    fx = _fx()
    X, Y = fx["exact_x"], fx["exact_y"]
    return X, Y, MR.map_quality(X, Y, MR.EXACT_K)


def _pad4(a):
    """fp32 rows on a pitch of a multiple of 4 floats, on the device (a view of the wider tensor)"""
    wide = torch.zeros((a.shape[0], (a.shape[1] + 3) & ~3), dtype=torch.float32, device=DEV)
    wide[:, :a.shape[1]] = _dev(a)
    return wide[:, :a.shape[1]]


def _rel(a, b):
    return abs(a - b) / abs(b)


# ---- 1. the generic family ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", MR.SHAPES, ids=MR.name_of)
def test_generic_ranks_penalties_and_scores(shape):
    from gesture2vec_amd import ops
    from gesture2vec_amd.embedding import continuity, kneighbors, map_quality, trustworthiness
    X, Y, k, ref, pre, sk_t, sk_c = _generic(shape)
    N = X.shape[0]
    print(f"{MR.name_of(shape)}: (a) {pre['a']}, (b) {pre['b']}, band pairs (sure, may) {pre['band_t']} / {pre['band_c']}")
    assert min(pre["a"]) > 1.0 and min(pre["b"]) > MR.REL_SEP                     # a bad input fails here, loudly
    xd, yd = _dev(X), _dev(Y)
    me = torch.arange(N, dtype=torch.int64, device=DEV)
    # the neighbours of each space
    nn_y, nn_x = kneighbors(yd, k, return_distance=False), kneighbors(xd, k, return_distance=False)
    assert nn_y.dtype == torch.int32 and np.array_equal(_host(nn_y), ref["nn_y"]) and np.array_equal(_host(nn_x), ref["nn_x"])
    # the kernel: every entry of every row
    rank_t, redo_t = ops.neighbor_ranks(_pad4(X), _pad4(X), nn_y, me)
    rank_c, redo_c = ops.neighbor_ranks(_pad4(Y), _pad4(Y), nn_x, me)
    assert rank_t.dtype == torch.int32 and tuple(rank_t.shape) == (N, k)
    assert np.array_equal(_host(rank_t), ref["rank_t"]) and np.array_equal(_host(rank_c), ref["rank_c"])
    for redo, (sure, may) in ((redo_t, pre["band_t"]), (redo_c, pre["band_c"])):
        n = int(_host(redo)[0])
        print(f"  decided again: {n} pairs (between {sure} and {may})")
        assert sure <= n <= may
        if sure:
            assert n > 0
    # the public surface
    q = map_quality(xd, yd, n_neighbors=k)
    assert q["penalty_t"].dtype == torch.int64 and q["penalty_t"].is_cuda and q["n_neighbors"] == k
    assert np.array_equal(_host(q["penalty_t"]), ref["penalty_t"]) and np.array_equal(_host(q["penalty_c"]), ref["penalty_c"])
    assert q["redecided"] == int(_host(redo_t)[0]) + int(_host(redo_c)[0])
    print(f"  trustworthiness {q['trustworthiness']!r} ({ref['trustworthiness']!r}), continuity {q['continuity']!r} "
          f"({ref['continuity']!r}); sklearn {sk_t!r}, {sk_c!r}")
    assert isinstance(q["trustworthiness"], float) and isinstance(q["continuity"], float)
    assert _rel(q["trustworthiness"], ref["trustworthiness"]) <= 1e-15 and _rel(q["continuity"], ref["continuity"]) <= 1e-15
    assert abs(q["trustworthiness"] - sk_t) <= 1e-12 and abs(q["continuity"] - sk_c) <= 1e-12
    assert trustworthiness(xd, yd, n_neighbors=k) == q["trustworthiness"] and continuity(xd, yd, n_neighbors=k) == q["continuity"]


# ---- 2. the exact family: ties and duplicates ----------------------------------------------------------------------------------------
def test_exact_family_pins_ties_and_self_removal():
    from gesture2vec_amd import ops
    from gesture2vec_amd.dbscan import k_distances
    from gesture2vec_amd.embedding import kneighbors, map_quality
    X, Y, ref = _exact()
    N, k = X.shape[0], MR.EXACT_K
    assert MR.exact_in_fp32(X) and MR.exact_in_fp32(Y)
    me_np = np.arange(N)
    assert MR.closest_compared(sqdist(X), ref["nn_y"], me_np) > MR.REL_SEP and MR.closest_compared(sqdist(Y), ref["nn_x"], me_np) > MR.REL_SEP
    xd, yd = _dev(X), _dev(Y)
    for A, ad, nn in ((X, xd, ref["nn_x"]), (Y, yd, ref["nn_y"])):
        dist, idx = kneighbors(ad, k)
        dref, iref = MR.kneighbors_other(A, k)
        assert np.array_equal(_host(idx), iref) and np.array_equal(iref, nn)
        assert np.array_equal(_host(dist), np.sqrt((dref ** 2).astype(np.float32)))           # d^2 is an integer: exact in fp32
        assert not (_host(idx) == me_np[:, None]).any()
    assert (ref["nn_y"][6] == np.arange(5)).all() and (ref["nn_y"][7] == np.arange(5)).all()  # rows 6, 7: five lower duplicates
    me = torch.arange(N, dtype=torch.int64, device=DEV)
    rank_t, redo = ops.neighbor_ranks(_pad4(X), _pad4(X), _dev(ref["nn_y"]), me)
    assert np.array_equal(_host(rank_t), ref["rank_t"])
    sure, may = MR.band_pairs(X, X, ref["nn_y"], me_np)
    assert sure > 0 and sure <= int(_host(redo)[0]) <= may                                   # equal distances are decided in float64
    q = map_quality(xd, yd, n_neighbors=k)
    assert np.array_equal(_host(q["penalty_t"]), ref["penalty_t"]) and np.array_equal(_host(q["penalty_c"]), ref["penalty_c"])
    assert _rel(q["trustworthiness"], ref["trustworthiness"]) <= 1e-15 and _rel(q["continuity"], ref["continuity"]) <= 1e-15
    for kk in (1, 2, 6):
        assert np.array_equal(_host(k_distances(xd, kk)), np.sqrt((MR.k_distances(X, kk) ** 2).astype(np.float32)))


# ---- 3. queries that are not reference rows; self on a duplicate; entries that are no row -------------------------------------------
def test_queries_apart_from_the_reference_rows_and_placement_quality():
    from gesture2vec_amd import ops
    from gesture2vec_amd.embedding import placement_quality
    fx = _fx()
    X, Y, Z, y, k = fx["placed_x"], fx["placed_y"], fx["placed_z"], fx["placed_yz"], int(fx["placed_k"])
    assert MR.selection_margin(X, k, Z) > 1.0 and MR.selection_margin(Y, k, y) > 1.0
    ref = MR.placement_quality(X, Y, Z, y, k)
    assert MR.closest_compared(MR.cross_sqdist(Z, X), ref["nn_y"]) > MR.REL_SEP
    assert MR.closest_compared(MR.cross_sqdist(y, Y), ref["nn_x"]) > MR.REL_SEP
    rank, _ = ops.neighbor_ranks(_pad4(X), _pad4(Z), _dev(ref["nn_y"]))                      # self = NULL: no row is left out
    assert tuple(rank.shape) == (37, k) and np.array_equal(_host(rank), ref["rank_t"])
    none = torch.full((37,), -1, dtype=torch.int64, device=DEV)
    assert torch.equal(ops.neighbor_ranks(_pad4(X), _pad4(Z), _dev(ref["nn_y"]), none)[0], rank)
    q = placement_quality(_dev(X), _dev(Y), _dev(Z), _dev(y), n_neighbors=k)
    assert np.array_equal(_host(q["penalty_t"]), ref["penalty_t"]) and np.array_equal(_host(q["penalty_c"]), ref["penalty_c"])
    assert q["penalty_t"].shape == (37,)
    assert _rel(q["trustworthiness"], ref["trustworthiness"]) <= 1e-15 and _rel(q["continuity"], ref["continuity"]) <= 1e-15


def test_self_on_a_bitwise_duplicate_and_entries_that_are_no_row():
    from gesture2vec_amd import ops
    X, _, ref = _exact()
    N = X.shape[0]
    assert (X[10] == X[3]).all()
    self_rows = np.arange(N)
    self_rows[3], self_rows[10] = 10, 3                           # the duplicate is left out, the row itself counts (at distance 0)
    idx = np.array(ref["nn_y"])
    idx[3, 0], idx[10, 0] = 3, 10                                 # and may be listed
    idx[5, 1], idx[5, 2], idx[6, 0], idx[7, 4] = -1, N, 6, 2 ** 31 - 1        # no row | no row | self | no row
    want = MR.neighbor_ranks(X, X, idx, self_rows)
    assert want[3, 0] == 1 and want[10, 0] == 1 and want[5, 1] == want[5, 2] == want[6, 0] == want[7, 4] == 0
    rank, _ = ops.neighbor_ranks(_pad4(X), _pad4(X), _dev(idx), _dev(self_rows, np.int64))
    assert np.array_equal(_host(rank), want)


# ---- 4. a workgroup that walks several column tiles (more row blocks than the split needs) ------------------------------------------
def test_many_query_rows_against_few_reference_rows():
    from gesture2vec_amd import ops
    X = _generic((257, 50, 127, 2))[0]
    g = np.random.default_rng(11)
    M = 8200                                                      # 129 row blocks: fewer column slices than the 5 tiles
    Z = (X[g.integers(0, X.shape[0], M)] + 0.7 * g.standard_normal((M, X.shape[1]))).astype(np.float32)
    D = MR.cross_sqdist(Z, X)
    idx = np.concatenate([MR.nearest(D, 3, False), g.integers(0, X.shape[0], (M, 2)).astype(np.int32)], axis=1)
    assert MR.closest_compared(D, idx) > MR.REL_SEP
    rank, _ = ops.neighbor_ranks(_pad4(X), _pad4(Z), _dev(idx))
    assert np.array_equal(_host(rank), MR.ranks_from(D, idx))


# ---- 5. the same bits: twice, and from a strided view ---------------------------------------------------------------------------------
def test_same_bits_twice_and_from_a_strided_view():
    from gesture2vec_amd import ops
    X, _, k, ref, _, _, _ = _generic((130, 40, 5, 2))
    N, d = X.shape
    me = torch.arange(N, dtype=torch.int64, device=DEV)
    idx = _dev(ref["nn_y"])
    xd = _dev(X)
    first = ops.neighbor_ranks(xd, xd, idx, me)
    again = ops.neighbor_ranks(xd, xd, idx, me)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    wide = torch.full((N, d + 12), float("nan"), dtype=torch.float32, device=DEV)             # columns d .. ld - 1 are never read
    wide[:, :d] = xd
    view = wide[:, :d]
    assert view.stride(0) == d + 12
    strided = ops.neighbor_ranks(view, view, idx, me)
    assert torch.equal(strided[0], first[0]) and torch.equal(strided[1], first[1])
    mixed = ops.neighbor_ranks(xd, view, idx, me)
    assert torch.equal(mixed[0], first[0])
    assert np.array_equal(_host(first[0]), ref["rank_t"])


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
def test_unsupported_shapes_raise_before_a_launch():
    from gesture2vec_amd import _lib, ops
    lib = _lib.load()
    x = torch.zeros((300, 8), dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match="k = 128"):
        ops.neighbor_ranks(x, x, torch.zeros((300, 128), dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="d = 516"):
        ops.neighbor_ranks(torch.zeros((8, 516), device=DEV), torch.zeros((8, 516), device=DEV), torch.zeros((8, 2), dtype=torch.int32, device=DEV))
    with pytest.raises(TypeError, match="multiple of 4"):
        ops.neighbor_ranks(torch.zeros((8, 6), device=DEV), x[:8], torch.zeros((8, 2), dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="columns"):
        ops.neighbor_ranks(x, torch.zeros((8, 12), device=DEV), torch.zeros((8, 2), dtype=torch.int32, device=DEV))
    with pytest.raises(TypeError):
        ops.neighbor_ranks(x, x, torch.zeros((300, 2), dtype=torch.int64, device=DEV))
    # the C entry itself: refused before any launch, the output untouched
    ws = torch.zeros((1 << 16,), dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    for k, ldx, d in ((128, 8, 8), (2, 6, 6), (2, 4, 8), (0, 8, 8), (2, 516, 516)):
        rank = torch.full((300, max(k, 1)), 7, dtype=torch.int32, device=DEV)
        idx = torch.zeros((300, max(k, 1)), dtype=torch.int32, device=DEV)
        rc = lib.g2v_neighbor_ranks(x.data_ptr(), ldx, 300 if d <= 8 else 4, x.data_ptr(), ldx, 300 if d <= 8 else 4, d, None,
                                    idx.data_ptr(), k, rank.data_ptr(), None, ws.data_ptr(), ws.numel(), stream)
        assert rc == _lib.ERR_UNSUPPORTED, (k, ldx, d)
        assert bool((_host(rank) == 7).all())


# ---- 7. kneighbors with queries, k_distances, sample_size -------------------------------------------------------------------------------
def test_kneighbors_k_distances_and_sample_size():
    from gesture2vec_amd.dbscan import k_distances
    from gesture2vec_amd.embedding import kneighbors, map_quality
    X, Y, k, ref, pre, _, _ = _generic((130, 40, 5, 2))
    assert min(pre["a"]) > 1.0
    xd, yd = _dev(X), _dev(Y)
    dist, idx = kneighbors(xd, k)
    dref, iref = MR.kneighbors_other(X, k)
    assert np.array_equal(_host(idx), iref) and dist.dtype == torch.float32
    assert np.abs(_host(dist) - dref).max() <= 2.0 ** -23 * dref.max()             # sqrt of the correctly rounded d^2
    fx = _fx()
    Z = fx["placed_z"]
    assert MR.selection_margin(X, k, Z) > 1.0
    dq, iq = kneighbors(xd, k, queries=_dev(Z))
    assert np.array_equal(_host(iq), MR.nearest(MR.cross_sqdist(Z, X), k, False)) and tuple(dq.shape) == (37, k)
    for kk in (1, 4, 12):
        got, want = _host(k_distances(xd, kk)).astype(np.float64), MR.k_distances(X, kk)
        assert got.shape == (130,) and (np.diff(got) >= 0).all()
        assert (np.abs(got - want) <= 2e-6 * want).all()
    with pytest.raises(ValueError, match="k"):
        kneighbors(xd, 130)
    with pytest.raises(ValueError, match="k"):
        kneighbors(xd, 128, queries=xd)
    sub = np.random.RandomState(3).permutation(130)[:40]
    a = map_quality(xd, yd, n_neighbors=k, sample_size=40, random_state=3)
    b = map_quality(_dev(X[sub]), _dev(Y[sub]), n_neighbors=k)
    assert a["trustworthiness"] == b["trustworthiness"] and a["continuity"] == b["continuity"] and a["redecided"] == b["redecided"]
    assert torch.equal(a["penalty_t"], b["penalty_t"]) and torch.equal(a["penalty_c"], b["penalty_c"]) and a["penalty_t"].shape == (40,)


# ---- 8. the scripts --------------------------------------------------------------------------------------------------------------------
def test_scripts_write_the_named_arrays(golden_dir, tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import cluster_latents
    import embed_latents
    from utils.train_utils import load_checkpoint_and_model
    from gesture2vec_amd.embedding import map_quality
    ckpt = os.path.join(golden_dir, "plain_ae_ckpt.bin")
    args, net, _, _, pose_dim = load_checkpoint_and_model(ckpt, DEV, "autoencoder_vq")
    net.eval()
    real = torch.randn(200, int(args.n_poses), pose_dim, generator=torch.Generator().manual_seed(5))
    np.save(tmp_path / "real.npy", real.numpy())
    common = ["--checkpoint", ckpt, "--device", DEV, "--chunks", str(tmp_path / "real.npy")]
    res = embed_latents.main(common + ["--max-iter", "250", "--sample-rows", "120", "--seed", "4", "--place-rest", "--quality", "5",
                                       "--save-map", str(tmp_path / "map.pk"), "--out", str(tmp_path / "all.npz")])
    printed = capsys.readouterr().out
    saved = np.load(tmp_path / "all.npz")
    assert saved["penalty_t"].shape == saved["penalty_c"].shape == (200,) and saved["penalty_t"].dtype == np.int64
    (ft, fc), (pt, pc) = res["quality"]["fitted"], res["quality"]["placed"]
    assert f"sample: trustworthiness {ft!r}, continuity {fc!r} over 5 neighbours of 120 rows\n" in printed
    assert f"placed rows: trustworthiness {pt!r}, continuity {pc!r} over 5 neighbours of 80 rows\n" in printed
    assert all(0.0 < v <= 1.0 for v in (ft, fc, pt, pc))
    fitted = saved["fitted"]
    for pen, score in ((saved["penalty_t"], ft), (saved["penalty_c"], fc)):
        assert MR.score(pen[fitted].sum(), 120, 120, 5) == score
    for pen, score in ((saved["penalty_t"], pt), (saved["penalty_c"], pc)):
        assert MR.score(pen[~fitted].sum(), 80, 120, 5) == score
    import pickle
    with open(tmp_path / "map.pk", "rb") as f:
        lm = pickle.load(f)
    rows = lm.rows_.numpy()
    direct = map_quality(lm.tsne.fit_rows_.to(DEV), lm.coords_.to(DEV), n_neighbors=5)
    assert np.array_equal(_host(direct["penalty_t"]), saved["penalty_t"][rows]) and direct["trustworthiness"] == ft
    placed = embed_latents.main(common + ["--map", str(tmp_path / "map.pk"), "--quality", "5", "--out", str(tmp_path / "made.npz")])
    assert placed["quality"]["fitted"] is None and np.load(tmp_path / "made.npz")["penalty_c"].shape == (200,)
    plain = embed_latents.main(common + ["--max-iter", "250", "--sample-rows", "120", "--seed", "4", "--quality", "5",
                                         "--out", str(tmp_path / "plain.npz")])
    assert plain["quality"]["placed"] is None and plain["quality"]["fitted"] == (ft, fc)
    assert np.array_equal(plain["penalty_t"], saved["penalty_t"][rows])

    capsys.readouterr()
    lat = cluster_latents.latents_of(net, real.to(DEV), 65536).cpu().numpy()
    out = tmp_path / "db.npz"
    cluster_latents.main(common + ["--algorithm", "dbscan", "--eps", "0.5", "--min-samples", "4", "--k-distances", "4", "--out", str(out)])
    curve = np.load(out)["k_distances"]
    want = MR.k_distances(lat, 4)
    assert curve.shape == (200,) and curve.dtype == np.float32 and (np.abs(curve - want) <= 2e-6 * want).all()
    assert "4-distances: quartiles " in capsys.readouterr().out
    assert set(np.load(out).files) == {"labels", "core", "k_distances"}
