"""Device-side pairwise-distance statistics and the representation-similarity metric (csrc/pair_stats.hip, gesture2vec_amd/repdist.py)
against the float64 restatement from differences (tests/_repdist_ref.py) and the reference's recorded Rep_distance.txt numbers
(tests/golden/repdist.npz).

Bars (derived, not measured; _repdist_ref has them).  pair_dist.hpp: a pair that is not near has |delta d^2| <= E 2^-53 (n_i + n_j)
<= 8 E 2^-53 d^2, so |delta d| / d <= 4 E 2^-53; a near pair carries one float64 difference chain.  With a factor 2 for the
fixed-order float64 sums: sum, mean, min, max 8 E 2^-53 relative; sum_sq 16 E 2^-53; std 16 E 2^-53 mean^2 / var (the subtraction
sum_sq / count - mean^2 loses that factor); a lag distance 4 E 2^-53; count, nonfinite and hist equal.  Equal histograms rest on a
precondition, asserted per case: no distance within 1e-9 relative of an edge, four orders above the per-pair bound.  The
reference's neighbour numbers are float32 arithmetic; their bar is the fixture's measured `ref_bar`."""
import functools
import os
import random
import sys

import numpy as np
import pytest
import torch

import _repdist_inputs as RI
import _repdist_ref as RR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"

from gesture2vec_amd import _lib, metrics, ops, repdist  # noqa: E402

STAT_SHAPES = [(1, 4), (2, 1), (63, 3), (64, 4), (65, 33), (130, 135), (257, 512), (300, 400)]
TWO_SETS = [(1, 65, 5), (129, 64, 36), (70, 200, 400)]


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "repdist.npz"))


def _dev(X):
    return torch.from_numpy(np.ascontiguousarray(X)).to(DEV)


def _edge_sets(d):
    """1, 7 and 64 uniform bins over (0, just above the largest distance), a range between the quartiles, which leaves distances
    outside on both sides, and one non-uniform array that does too"""
    top = RI.hist_hi(d.max()) if d.size else 1.0
    lo, hi = 0.31 * top, 0.83 * top
    if d.size >= 8:
        s = np.sort(d)
        lo, hi = 0.5 * (s[d.size // 4] + s[d.size // 4 + 1]), 0.5 * (s[3 * d.size // 4] + s[3 * d.size // 4 + 1])
    return [np.linspace(0.0, top, b + 1) for b in (1, 7, 64)] + [np.linspace(lo, hi, 12),
                                                                   top * np.array([0.05, 0.3, 0.35, 0.36, 0.7, 0.9])]


@functools.lru_cache(maxsize=None)
def _case(N, E, M=0):
    """the first seed from 0 whose distances keep off every edge of _edge_sets; the restatement is computed once per shape"""
    for seed in range(50):
        X = RI.clustered(N, E, seed)
        Y = RI.clustered(M, E, 1000 + seed, k=3) if M else None
        ref = RR.stats(X, Y)
        edges = _edge_sets(ref["d"])
        if all(RR.edge_gap(ref["d"], e) > RR.EDGE_GAP for e in edges):
            return X, Y, ref, edges
    raise AssertionError(f"no seed below 50 keeps every distance off the edges at {(N, M, E)}")


def _check(got, ref, E, what=""):
    """counts equal, the floating-point statistics within their bars; prints the fraction of each bar that is used"""
    assert got["count"] == ref["count"] and got["nonfinite"] == ref["nonfinite"], (got["count"], got["nonfinite"])
    used = {}
    if ref["count"] == 0:
        assert (got["sum"], got["sum_sq"], got["min"], got["max"]) == (0.0, 0.0, float("inf"), float("-inf"))
        assert np.isnan(got["mean"]) and np.isnan(got["std"])
        return used
    for k, bar in (("sum", RR.bar_sum(E)), ("mean", RR.bar_sum(E)), ("min", RR.bar_sum(E)), ("max", RR.bar_sum(E)), ("sum_sq", RR.bar_sq(E))):
        used[k] = abs(got[k] - ref[k]) / (bar * abs(ref[k])) if ref[k] != 0 else (0.0 if got[k] == 0 else np.inf)
    if ref["count"] > 1 and ref["std"] > 0:
        used["std"] = abs(got["std"] - ref["std"]) / (RR.bar_std(E, ref["mean"], ref["std"] ** 2) * ref["std"])
    else:
        assert got["std"] == ref["std"] == 0.0
    print(f"{what}: fraction of the bar used " + ", ".join(f"{k} {v:.3f}" for k, v in used.items()))
    assert all(v <= 1.0 for v in used.values()), used
    return used


# ---- 1. statistics and histograms of one set ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,E", STAT_SHAPES)
def test_statistics_against_the_restatement(N, E):
    X, _, ref, edge_sets = _case(N, E)
    x = _dev(X)
    got = repdist.pairwise_distance_stats(x)
    assert got["count"] == N * (N - 1) // 2 and "hist" not in got
    _check(got, ref, E, f"N={N} E={E}")
    for edges in edge_sets:
        uniform = np.array_equal(edges, np.linspace(edges[0], edges[-1], edges.size))
        kw = dict(bins=edges.size - 1, range=(edges[0], edges[-1])) if uniform else dict(bins=edges)
        h = repdist.pairwise_distance_stats(x, **kw)
        assert h["hist"].dtype == torch.int64 and h["hist"].is_cuda and np.array_equal(h["edges"], edges)
        want = RR.histogram(ref["d"], edges)
        assert np.array_equal(h["hist"].cpu().numpy(), want), (edges.size - 1, h["hist"].cpu().numpy() - want)
        assert all(h[k] == got[k] for k in ("count", "sum", "sum_sq", "min", "max", "nonfinite"))    # bins change no statistic
    if N > 2:
        inside = RR.histogram(ref["d"], edge_sets[3])
        assert 0 < inside.sum() < ref["count"] and (ref["d"] < edge_sets[3][0]).any() and (ref["d"] > edge_sets[3][-1]).any()


def test_fixture_shapes_against_scipy(fx):
    """the recorded scipy / numpy values of the two smaller generic shapes (the restatement is held to all four on the host)"""
    for shape in RI.GENERIC[1:3]:
        N, E = shape
        key = f"pdist/{RI.name_of(shape)}/"
        X = RI.clustered(N, E, int(fx[key + "seed"]))
        assert RI.sha256(X) == str(fx[key + "sha256"])
        hi = float(fx[key + "hi"])
        got = repdist.pairwise_distance_stats(_dev(X), bins=RI.HIST_BINS, range=(0.0, hi))
        for k in ("mean", "min", "max"):
            assert abs(got[k] - float(fx[key + k])) <= RR.bar_sum(E) * float(fx[key + k]), k
        std, mean = float(fx[key + "std"]), float(fx[key + "mean"])
        assert abs(got["std"] - std) <= RR.bar_std(E, mean, std * std) * std
        assert np.array_equal(got["hist"].cpu().numpy(), fx[key + "hist"])


def test_a_distance_exactly_on_the_last_edge():
    """integer rows: every d^2 is an integer that the Gram form and the differences both give exactly, and 30^2 + 40^2 = 50^2 puts
    one distance on the last edge, which numpy.histogram's rule counts in the last bin; larger distances are outside"""
    rng = np.random.default_rng(4)
    X = rng.integers(-3, 4, size=(70, 6)).astype(np.float32)
    X[11] = 0.0
    X[69] = (30.0, 40.0, 0.0, 0.0, 0.0, 0.0)
    ref, d2 = RR.stats(X), RR.pair_d2(X)
    assert np.array_equal(d2, np.round(d2)) and d2.max() < 2.0 ** 20
    assert (ref["d"] == 50.0).sum() >= 1 and (ref["d"] > 50.0).any()
    for edges in (np.linspace(2.5, 50.0, 20), np.array([0.0, 1.0, 49.5, 50.0])):
        assert RR.edge_gap(ref["d"], edges, skip_equal=True) > RR.EDGE_GAP
        on_edge = ref["d"][np.isin(ref["d"], edges)]
        assert np.array_equal(on_edge, np.round(on_edge))         # a distance that IS an edge is the root of a perfect square
        got = repdist.pairwise_distance_stats(_dev(X), bins=edges)
        want = RR.histogram(ref["d"], edges)
        assert np.array_equal(want, np.histogram(ref["d"], edges)[0]) and want[-1] >= 1
        assert np.array_equal(got["hist"].cpu().numpy(), want)
        assert got["sum_sq"] == ref["sum_sq"]                                                       # integers: exact in any order


# ---- 2. two sets ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,M,E", TWO_SETS)
def test_two_sets_and_swapped(N, M, E):
    X, Y, ref, edge_sets = _case(N, E, M)
    edges = edge_sets[1]
    a = repdist.pairwise_distance_stats(_dev(X), _dev(Y), bins=edges)
    b = repdist.pairwise_distance_stats(_dev(Y), _dev(X), bins=edges)
    want = RR.histogram(ref["d"], edges)
    for got, what in ((a, "x, y"), (b, "y, x")):
        assert got["count"] == N * M
        _check(got, ref, E, f"N={N} M={M} E={E} ({what})")
        assert np.array_equal(got["hist"].cpu().numpy(), want)
    assert a["min"] == b["min"] and a["max"] == b["max"]          # d(i, j) and d(j, i) are the same bits


# ---- 3. the identity sum_{i<j} d^2 = N sum |x_i|^2 - |sum x_i|^2 -------------------------------------------------------------------------
@pytest.mark.parametrize("N,E", [(200, 33), (4197, 36)])
def test_sum_of_squares_identity(N, E):
    run = ops.pair_stats_run(N)
    tiles = -(-N // 64)
    assert run >= 1 and -(-tiles // run) >= 2 and N % 64 != 0     # a strip is split over workgroups, the last tile is ragged
    if N > 4096:
        assert run >= 2                                           # ... and a workgroup walks more than one tile
    X = np.random.default_rng(N).normal(size=(N, E)).astype(np.float32)
    X64 = X.astype(np.float64)
    import math
    norms = math.fsum((X64 * X64).ravel().tolist())
    col = [math.fsum(X64[:, k].tolist()) for k in range(E)]
    want = N * norms - math.fsum(c * c for c in col)
    got = repdist.pairwise_distance_stats(_dev(X))
    assert got["count"] == N * (N - 1) // 2 and got["nonfinite"] == 0
    used = abs(got["sum_sq"] - want) / (RR.bar_sq(E) * want)
    print(f"N={N} E={E} run={run}: identity off by {used:.3f} of the bar")
    assert used <= 1.0


# ---- 4. near pairs and non-finite rows ---------------------------------------------------------------------------------------------------
def test_near_pairs():
    X = RI.clustered(65, 33, 2)
    X *= np.float32(20.0 / np.sqrt((X[7].astype(np.float64) ** 2).sum()))
    X[50] = X[7] + np.float32(1e-4 / np.sqrt(33)) * np.sign(X[7])                  # ~1e-4 apart at norm 20
    ref = RR.stats(X)
    assert 0.2e-4 < ref["min"] < 3e-4 and abs(np.sqrt((X[7].astype(np.float64) ** 2).sum()) - 20) < 1e-3
    got = repdist.pairwise_distance_stats(_dev(X))
    _check(got, ref, 33, "rows 1e-4 apart")
    X[40] = X[3]                                                                   # a bitwise duplicate: 0 apart exactly
    ref = RR.stats(X)
    edges = np.linspace(0.0, RI.hist_hi(ref["max"]), 8)
    assert ref["min"] == 0.0 and RR.edge_gap(ref["d"], edges) > RR.EDGE_GAP
    got = repdist.pairwise_distance_stats(_dev(X), bins=edges)
    assert got["min"] == 0.0
    _check(got, ref, 33, "duplicate rows")
    want = RR.histogram(ref["d"], edges)
    assert want[0] >= 2 and np.array_equal(got["hist"].cpu().numpy(), want)        # the pairs (3, 40) and (7, 50) are in the first bin


def test_a_nan_row():
    N, E = 70, 12
    X = RI.clustered(N, E, 5)
    X[66, 3] = np.nan
    ref = RR.stats(X)
    edges = np.linspace(0.0, RI.hist_hi(ref["max"]), 10)
    assert ref["nonfinite"] == N - 1 and RR.edge_gap(ref["d"], edges) > RR.EDGE_GAP
    got = repdist.pairwise_distance_stats(_dev(X), bins=edges)
    assert got["count"] == N * (N - 1) // 2 and got["nonfinite"] == N - 1
    assert np.isnan(got["sum"]) and np.isnan(got["sum_sq"]) and np.isnan(got["mean"]) and np.isnan(got["std"])
    for k in ("min", "max"):                                                       # over the distances that are numbers
        assert abs(got[k] - ref[k]) <= RR.bar_sum(E) * ref[k]
    hist = got["hist"].cpu().numpy()
    assert np.array_equal(hist, RR.histogram(ref["d"], edges)) and int(hist.sum()) == got["count"] - (N - 1)


# ---- 5. the same bits --------------------------------------------------------------------------------------------------------------------
def test_same_bits_on_every_call():
    N, E = 130, 135
    X, _, ref, edge_sets = _case(N, E)
    edges = _dev(edge_sets[2])
    pad = torch.zeros(N, 136, device=DEV)
    pad[:, :E] = _dev(X)
    x = pad[:, :E]                                                # ld = 136: a row stride of whole 16-byte vectors
    first = ops.pair_stats(x, None, edges)
    wide = torch.full((N, 160), float("nan"), device=DEV)
    wide[:, :E] = _dev(X)
    poisoned = torch.full((ops.pair_stats_workspace(N, 0, E, 64),), 0xFF, dtype=torch.uint8, device=DEV)
    for again in (ops.pair_stats(x, None, edges), ops.pair_stats(wide[:, :E], None, edges),
                  ops.pair_stats(x, None, edges, ws=poisoned)):
        for a, b in zip(first, again):
            assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    got = repdist.pairwise_distance_stats(_dev(X), bins=edge_sets[2])             # E % 4 != 0: repdist pads by itself
    assert [got["sum"], got["sum_sq"], got["min"], got["max"]] == first[0].cpu().tolist()
    perm = np.random.default_rng(1).permutation(N)
    other = repdist.pairwise_distance_stats(_dev(X[perm]), bins=edge_sets[2])
    assert all(other[k] == got[k] for k in ("count", "nonfinite", "min", "max")) and torch.equal(other["hist"], got["hist"])
    assert abs(other["sum"] - got["sum"]) <= RR.bar_sum(E) * got["sum"] and abs(other["sum_sq"] - got["sum_sq"]) <= RR.bar_sq(E) * got["sum_sq"]


# ---- 6. lag distances --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [5, 6, 64, 65, 300])
def test_lag_distances(N):
    E = 37 if N < 300 else 400
    X = RI.sequence(N, E, N)
    ids = np.repeat(np.arange(3), [max(N // 3, 1), 1, N])[:N]                        # clips: a third of the rows, ONE row, the rest
    for lags, clip in (((1, 2), None), ((1,), None), ((3, 7), None), ((1, 2), ids), ((3, 7), ids)):
        want = RR.lag_distances(X, lags, clip)
        out = repdist.lag_distances(_dev(X), lags, None if clip is None else torch.from_numpy(clip))
        assert out.dtype == torch.float64 and tuple(out.shape) == (len(lags), N) and out.is_cuda
        got = out.cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        if ok.any():
            assert np.max(np.abs(got[ok] - want[ok]) / want[ok]) <= RR.bar_lag(E)
    if N <= 6:
        assert np.isnan(repdist.lag_distances(_dev(X), (7,)).cpu().numpy()).all()   # a lag longer than the sequence
    assert np.isnan(RR.lag_distances(X, (1,), ids)[0, max(N // 3, 1)])               # the clip of one row has no neighbour


# ---- 7. the reference's numbers ------------------------------------------------------------------------------------------------------------
def test_representation_similarity_against_the_reference(fx):
    N, E = (int(v) for v in fx["reference/shape"])
    row_seed, seed = (int(v) for v in fx["reference/seeds"])
    X = RI.sequence(N, E, row_seed)
    assert RI.sha256(X) == str(fx["reference/sha256"])
    x = _dev(X)
    ref_bar = float(fx["reference/ref_bar"])
    res = {}
    for method in ("all", "random"):
        want = dict(zip(RR.KEYS, (float(v) for v in fx[f"reference/{method}"])))
        got = res[method] = repdist.representation_similarity(x, method=method, seed=seed)
        assert sorted(got) == sorted(RR.KEYS)
        assert abs(got["avg_dist_total"] - want["avg_dist_total"]) <= RR.bar_sum(E) * want["avg_dist_total"]
        worst = max(abs(got[k] - want[k]) / abs(want[k]) for k in RR.NEIGHBOUR_KEYS)
        print(f"{method}: neighbour numbers off the reference's by {worst:.2e} (bar {ref_bar:.2e})")
        assert worst <= ref_bar
    rows = repdist.similarity_rows(N, "random", 1000, seed)
    assert rows == random.Random(seed).sample(range(2, N - 2), 1000)
    lagd = repdist.lag_distances(x).cpu().numpy()
    assert abs(res["random"]["avg_20fs"] - lagd[0, rows].mean()) <= 4 * RR.bar_lag(E) * res["random"]["avg_20fs"]
    text = repdist.representation_report(x, seed=seed)
    assert repdist.parse_report(text) == res
    assert [ln for ln in text.splitlines() if ln and not any(c.isdigit() for c in ln)] == [str(h) for h in fx["reference/headings"]]
    ids = torch.arange(N) // 100                                  # clips of 100 rows: the rows at their ends are left out
    clipped = repdist.representation_similarity(x, clip_ids=ids)
    want = RR.representation_similarity(X, clip_ids=(np.arange(N) // 100), avg_total=res["all"]["avg_dist_total"])
    assert all(abs(clipped[k] - want[k]) <= 1e-12 * abs(want[k]) for k in RR.KEYS)


# ---- 8. energy distance --------------------------------------------------------------------------------------------------------------------
def test_energy_distance():
    N, M, E = 70, 200, 400
    X, Y, ref_xy, _ = _case(N, E, M)
    ref_xx, ref_yy = RR.stats(X), RR.stats(Y)
    scale = 2 * ref_xy["mean"] + 2 * ref_xx["sum"] / N ** 2 + 2 * ref_yy["sum"] / M ** 2
    bar = RR.bar_sum(E) * scale                                    # each of the three means carries bar_sum relative
    want = 2 * ref_xy["mean"] - 2 * ref_xx["sum"] / N ** 2 - 2 * ref_yy["sum"] / M ** 2
    x, y = _dev(X), _dev(Y)
    a, b = metrics.energy_distance(x, y), metrics.energy_distance(y, x)
    assert want > 0 and abs(a - want) <= bar and abs(b - want) <= bar and abs(a - b) <= bar
    same = metrics.energy_distance(x, x.clone())
    assert abs(same) <= RR.bar_sum(E) * 8 * ref_xx["sum"] / N ** 2     # the same bar with y = x: 2 mean_xy + 2 mean_xx


# ---- 9. refusals, before any launch --------------------------------------------------------------------------------------------------------
def test_refusals():
    x = torch.zeros(8, 516, device=DEV)
    out, counts = torch.zeros(4, dtype=torch.float64, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV)
    ws = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    lib = _lib.load()
    assert ops.pair_stats_workspace(8, 0, 513) == 0 and ops.pair_stats_workspace(8, 0, 4, 1025) == 0 and ops.pair_stats_run(0) == 0
    assert ops.pair_stats_workspace(8, 0, 512, 1024) > 0
    rc = lib.g2v_pair_stats(x.data_ptr(), 516, 8, None, 0, 0, 513, None, 0, out.data_ptr(), counts.data_ptr(), None, ws.data_ptr(), 4096,
                            torch.cuda.current_stream().cuda_stream)
    assert rc == _lib.ERR_UNSUPPORTED and b"E <= 512" in lib.g2v_last_error()
    rc = lib.g2v_pair_stats(x.data_ptr(), 514, 8, None, 0, 0, 4, None, 0, out.data_ptr(), counts.data_ptr(), None, ws.data_ptr(), 4096,
                            torch.cuda.current_stream().cuda_stream)
    assert rc == _lib.ERR_ARG
    torch.cuda.synchronize()
    assert float(out.sum()) == 0.0 and int(counts.sum()) == 0     # nothing was launched
    with pytest.raises(ValueError):
        repdist.pairwise_distance_stats(x[:, :513])
    with pytest.raises(ValueError):
        ops.pair_stats(x[:, :513])
    good = x[:, :8]
    for bad in (good.cpu(), good.double(), good[0], good.int()):
        for call in (repdist.pairwise_distance_stats, repdist.lag_distances, repdist.representation_similarity, repdist.representation_report):
            with pytest.raises(TypeError):
                call(bad)
        with pytest.raises(TypeError):
            repdist.pairwise_distance_stats(good, bad)
    with pytest.raises(ValueError):
        repdist.pairwise_distance_stats(good, x[:, :12])
    for kw in (dict(bins=[2.0, 1.0, 0.5]), dict(bins=16), dict(range=(0.0, 1.0)), dict(bins=1025, range=(0.0, 1.0)), dict(bins=0, range=(0.0, 1.0))):
        with pytest.raises(ValueError):
            repdist.pairwise_distance_stats(good, **kw)
    for lags in ((), (0,), (1, -2), tuple(range(1, 10)), (1.5,)):
        with pytest.raises(ValueError):
            repdist.lag_distances(good, lags)
    with pytest.raises(ValueError):
        repdist.lag_distances(good, (1,), torch.zeros(7, dtype=torch.int64))
    many = torch.zeros(1003, 4, device=DEV)
    with pytest.raises(ValueError, match="n_random"):
        repdist.representation_similarity(many, method="random")
    with pytest.raises(ValueError, match="n_random"):
        repdist.representation_report(many)
    with pytest.raises(ValueError):
        repdist.representation_similarity(many, method="neither")


# ---- 10. the scripts -----------------------------------------------------------------------------------------------------------------------
def test_scripts(golden_dir, tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import cluster_latents
    import evaluate_metrics
    from utils.train_utils import load_checkpoint_and_model
    ckpt = os.path.join(golden_dir, "plain_ae_ckpt.bin")
    args, net, _, _, pose_dim = load_checkpoint_and_model(ckpt, DEV, "autoencoder_vq")
    net.eval()
    g = torch.Generator().manual_seed(9)
    real = torch.cumsum(0.2 * torch.randn(1010, int(args.n_poses), pose_dim, generator=g), dim=0)      # chunks that follow each other
    np.save(tmp_path / "chunks.npy", real.numpy())
    lat = cluster_latents.latents_of(net, real.to(DEV), 65536)
    common = ["--checkpoint", ckpt, "--chunks", str(tmp_path / "chunks.npy"), "--device", DEV, "--algorithm", "dbscan", "--eps", "0.5"]
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    capsys.readouterr()                                           # (the loader above prints too)
    cluster_latents.main(common + ["--out", str(tmp_path / "a" / "labels.npz")])
    plain = capsys.readouterr().out
    assert not (tmp_path / "a" / "Rep_distance.txt").exists() and "Representation" not in plain
    cluster_latents.main(common + ["--out", str(tmp_path / "b" / "labels.npz"), "--rep-distance", "--rep-seed", "3"])
    printed = capsys.readouterr().out
    text = (tmp_path / "b" / "Rep_distance.txt").read_text()
    assert text in printed and (tmp_path / "b" / "labels.npz").exists()
    want = {m: repdist.representation_similarity(lat, method=m, seed=3) for m in ("all", "random")}
    assert repdist.parse_report(text) == want
    assert printed.replace(text + "\n", "").replace(f"wrote {tmp_path / 'b' / 'Rep_distance.txt'}\n", "") == \
        plain.replace(str(tmp_path / "a"), str(tmp_path / "b"))                   # the flag adds, and changes nothing else
    with pytest.raises(SystemExit):
        cluster_latents.main(common[:-4] + ["--algorithm", "dtw", "--rep-distance"])
    capsys.readouterr()
    gen = real[:300] + 0.05 * torch.randn(300, int(args.n_poses), pose_dim, generator=g)
    np.save(tmp_path / "real.npy", real[:400].numpy())
    np.save(tmp_path / "gen.npy", gen.numpy())
    ev = ["--checkpoint", ckpt, "--real", str(tmp_path / "real.npy"), "--generated", str(tmp_path / "gen.npy"), "--device", DEV]
    evaluate_metrics.main(ev)
    before = capsys.readouterr().out
    m = evaluate_metrics.main(ev + ["--energy"])
    after = capsys.readouterr().out
    lat_r, lat_g = metrics.set_latents(net, real[:400].to(DEV)), metrics.set_latents(net, gen.to(DEV))
    assert m["energy"] == metrics.energy_distance(lat_r, lat_g) and m["energy"] > 0
    assert after == before + "Energy distance --> " + repr(m["energy"]) + "\n"
