"""Placing new rows into a fitted t-SNE map on the device (csrc/tsne_place.hip, embedding.TSNE.transform, embedding.LatentMap)
against the float64 restatement (tests/_tsne_place_ref.py) on the seeded inputs of tests/_tsne_place_inputs.py.

Bars.  Neighbours: per row, the sorted float64 distances of the device's neighbours equal the restatement's kk smallest within
tau_i = 4e-6 (|z_i|^2 + max_j |x_j|^2), ten times the 3e-7 rounding include/g2v.h documents for the Gram distances; no row is exempt.
Conditionals: 4 x the effect of rounding the distances to fp32 on the restatement, relative to the row maximum, floor 1e-6 (P_FLOOR
of tests/test_gpu_tsne.py), on the rows whose device neighbour list is the restatement's (at least 98 % of them).  Gradient, KL, Z and
the trajectories of 25 and of 250 steps: 4 x the distance between the restatement evaluated in float32 and in float64, computed in the
test.  (The float32 and float64 trajectories of the restatement stay within 1e-6 of max |Y| of each other at 25 steps and 1e-7 at
250, where the rows have settled: the sign rule of the gains does not make the distance unstable, so the trajectory bound is kept
for both and no bound on the KL is needed in its place.)"""
import functools
import os
import pickle

import numpy as np
import pytest
import torch

import _tsne_place_inputs as PI
import _tsne_place_ref as PR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P_FLOOR = 1e-6
STEP_KW = dict(exaggeration=1.5, momentum=0.8, learning_rate=0.1, max_grad_norm=0.25)


def _dev(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(DEV)         # (a copy: the inputs are read-only)


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _main_dev():
    c = PI.main_case()
    return c, _dev(c["Y"]), _dev(c["idx"], np.int32), _dev(c["p"])


@functools.lru_cache(maxsize=None)
def _ref_runs(n_iter):
    """the restatement's float64 and float32 runs of n_iter steps on the shared case (computed once)"""
    c = PI.main_case()
    return (PR.descend(c["Y"], c["idx"], c["p"], c["y0"], n_iter=n_iter, **STEP_KW),
            PR.descend(c["Y"], c["idx"], c["p"], c["y0"], n_iter=n_iter, dtype=np.float32, **STEP_KW))


def _fitted_tsne(X, Y):
    """a TSNE that holds the given rows and map as if it had fitted them"""
    from gesture2vec_amd.embedding import TSNE
    t = TSNE()
    t.fit_rows_, t.embedding_ = _dev(X), _dev(Y)
    return t


# ---- 1. neighbours --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PI.NEIGHBOUR_CASES))
def test_neighbours(name):
    from gesture2vec_amd import ops
    N, d, M, kk = PI.NEIGHBOUR_CASES[name]
    X, _, Z, _ = PI.rows(N, d, M)
    if name == "ld52":                                            # rows on a pitch of 52 floats, the two spare columns hold junk
        xd, zd = torch.full((N, 52), 7.5, device=DEV), torch.full((M, 52), -3.25, device=DEV)
        xd[:, :d], zd[:, :d] = _dev(X), _dev(Z)
        xd, zd = xd[:, :d], zd[:, :d]
        assert xd.stride(0) == 52 and zd.stride(0) == 52
    else:
        xd, zd = _dev(X), _dev(Z)
    idx, d2 = ops.tsne_place_neighbors(xd, zd, kk)
    assert idx.shape == (M, kk) and idx.dtype == torch.int32 and d2.shape == (M, kk) and d2.dtype == torch.float32
    idx, d2 = _host(idx).astype(np.int64), _host(d2)
    assert idx.min() >= 0 and idx.max() < N
    assert all(len(set(r)) == kk for r in idx.tolist()), "a reference row appears twice in a list"
    assert (np.diff(d2, axis=1) >= 0).all(), "d2 must not decrease along a row"
    D = PR.sqdist(Z, X)
    want = PR.neighbors(D, kk)[1]
    got = np.sort(np.take_along_axis(D, idx, 1), axis=1)
    tau = PI.tau(X, Z)
    worst = float((np.abs(got - want).max(1) / tau).max())
    dev_err = float((np.abs(d2 - np.take_along_axis(D, idx, 1)).max(1) / tau).max())
    print(f"{name}: N = {N}, d = {d}, M = {M}, kk = {kk}: neighbour distances within {worst:.3f} tau, the device's own d2 within "
          f"{dev_err:.3f} tau of float64")
    assert worst <= 1.0 and dev_err <= 1.0
    # planted: Z[1] is X[3] bit for bit; X[4] and X[5] are equal bit for bit and the nearest rows of Z[2]
    assert idx[1, 0] == 3 and d2[1, 0] == 0.0
    assert idx[2, 0] == 4 and idx[2, 1] == 5 and d2[2, 0] == d2[2, 1]


# ---- 2. conditionals and start --------------------------------------------------------------------------------------------------
def test_conditionals():
    from gesture2vec_amd import ops
    c = PI.main_case()
    kk = max(PI.K_AFF, PI.K)
    idx, d2 = ops.tsne_place_neighbors(_dev(c["X"]), _dev(c["Z"]), kk)
    p = _host(ops.tsne_place_conditionals(d2, PI.K_AFF, PI.PERPLEXITY)).astype(np.float64)
    same = (_host(idx).astype(np.int64) == c["idx"]).all(1)
    assert p.shape == (len(same), PI.K_AFF)
    assert float(np.abs(p.sum(1) - 1.0).max()) <= 1e-6
    p64 = PR.conditionals(c["d2"][:, :PI.K_AFF], PI.PERPLEXITY)
    p32 = PR.conditionals(c["d2"][:, :PI.K_AFF].astype(np.float32), PI.PERPLEXITY)
    top = p64.max(1, keepdims=True)
    bound = max(4.0 * float((np.abs(p32 - p64) / top).max()), P_FLOOR)
    err = float((np.abs(p - p64) / top)[same].max())
    print(f"conditionals: {int((~same).sum())} of {len(same)} rows with another neighbour list; within {err:.2e} of the row maximum "
          f"(bound {bound:.2e}), row sums within {float(np.abs(p.sum(1) - 1.0).max()):.1e} of 1")
    assert (~same).mean() <= 0.02
    assert err <= bound


def test_start():
    from gesture2vec_amd import ops
    c, Yd, idxd, pd = _main_dev()
    ymax = float(np.abs(c["Y"]).max())
    med = _host(ops.tsne_place_init(Yd, idxd, None, "median", PI.K))
    assert np.array_equal(med, c["y0"]) and med.dtype == np.float32
    even = _host(ops.tsne_place_init(Yd, idxd, None, "median", PI.K - 1))
    want = PR.start(c["Y"], c["idx"], None, "median", PI.K - 1)
    assert (np.abs(even - want) <= np.spacing(np.abs(want))).all()
    wd = _host(ops.tsne_place_init(Yd, idxd, pd, "weighted"))
    ww = PR.start(c["Y"], c["idx"], c["p"], "weighted")
    print(f"weighted start within {float(np.abs(wd - ww).max()) / ymax:.2e} of max |Y|")
    assert float(np.abs(wd - ww).max()) <= 2.0 ** -22 * ymax


# ---- 3. gradient, KL and Z ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("yname", ["start", "spread"])
@pytest.mark.parametrize("ex", [1.0, 1.5])
def test_gradient_kl_and_z(yname, ex):
    from gesture2vec_amd import ops
    c, Yd, idxd, pd = _main_dev()
    y = c["y0"] if yname == "start" else (5.0 * np.random.RandomState(3).standard_normal(c["y0"].shape)).astype(np.float32)
    kl, g, Z = PR.kl_grad(c["Y"], c["idx"], c["p"], y, ex)
    kl32, g32, Z32 = PR.kl_grad(c["Y"], c["idx"], c["p"], y, ex, dtype=np.float32)
    gmax = float(np.abs(g).max())
    bg, bk, bz = 4.0 * float(np.abs(g32 - g).max()) / gmax, 4.0 * float(np.abs(kl32 - kl).max()), 4.0 * float((np.abs(Z32 - Z) / Z).max())
    yd = _dev(y)
    out = ops.tsne_place_descent(Yd, idxd, pd, yd, n_iter=0, exaggeration=ex)
    assert np.array_equal(_host(yd), y), "n_iter == 0 must not move y"
    eg = float(np.abs(_host(out["grad"]) - g).max()) / gmax
    ek, ez = float(np.abs(_host(out["kl"]) - kl).max()), float((np.abs(_host(out["zsum"]) - Z) / Z).max())
    print(f"{yname} y, exaggeration {ex}: grad within {eg:.2e} of max |g| (bound {bg:.2e}), KL within {ek:.2e} ({bk:.2e}), "
          f"Z within {ez:.2e} ({bz:.2e})")
    assert eg <= bg and ek <= bk and ez <= bz


# ---- 4. trajectories ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_iter", [25, 250])
def test_trajectory(n_iter):
    from gesture2vec_amd import ops
    c, Yd, idxd, pd = _main_dev()
    (y64, kl64, _, _), (y32, kl32, _, _) = _ref_runs(n_iter)
    scale = float(np.abs(c["Y"]).max())
    bound = 4.0 * float(np.abs(y32 - y64).max()) / scale
    yd = _dev(c["y0"])
    out = ops.tsne_place_descent(Yd, idxd, pd, yd, n_iter=n_iter, **STEP_KW)
    err = float(np.abs(_host(yd) - y64).max()) / scale
    ekl = float(np.abs(_host(out["kl"]) - kl64).max())
    print(f"{n_iter} steps: within {err:.2e} of the float64 trajectory (bound {bound:.2e}, max |Y| = {scale:.3e}); KL within "
          f"{ekl:.2e} (the restatement's float32 run: {float(np.abs(kl32 - kl64).max()):.2e})")
    assert err <= bound


# ---- 5. clip and grid -----------------------------------------------------------------------------------------------------------
def test_clip_and_grid():
    """M = 70001 rows (more than one pass of the descent's grid), 3 steps from starts that sit on fitted points of the map, where
    the gradient of most rows is longer than max_grad_norm; 192 rows against the restatement"""
    from gesture2vec_amd import ops
    c, Yd, _, _ = _main_dev()
    M, m = 70001, len(c["idx"])
    src = np.arange(M) % m
    idx, p = c["idx"][src], c["p"][src]
    rng = np.random.default_rng(11)
    on = idx[np.arange(M), rng.integers(0, PI.K_AFF, M)]          # each row starts on top of one of its own neighbours
    y0 = (c["Y"][on] + 1e-3 * rng.normal(size=(M, 2))).astype(np.float32)
    S = np.unique(np.concatenate([np.arange(64), np.arange(M - 64, M), rng.choice(M, 64, replace=False)]))
    _, g0, _ = PR.kl_grad(c["Y"], idx[S], p[S], y0[S], STEP_KW["exaggeration"])
    clipped = np.sqrt((g0 ** 2).sum(1)) > STEP_KW["max_grad_norm"]
    assert clipped.mean() >= 0.5, "the inputs do not engage the clip"
    y64 = PR.descend(c["Y"], idx[S], p[S], y0[S], n_iter=3, **STEP_KW)[0]
    y32 = PR.descend(c["Y"], idx[S], p[S], y0[S], n_iter=3, dtype=np.float32, **STEP_KW)[0]
    scale = float(np.abs(c["Y"]).max())
    bound = 4.0 * float(np.abs(y32 - y64).max()) / scale
    yd = _dev(y0)
    ops.tsne_place_descent(Yd, _dev(idx, np.int32), _dev(p), yd, n_iter=3, want=(), **STEP_KW)
    got = _host(yd)
    err = float(np.abs(got[S] - y64).max()) / scale
    print(f"M = {M}, 3 steps, {int(clipped.sum())} of {len(S)} checked rows clipped at the start: within {err:.2e} (bound {bound:.2e})")
    assert err <= bound
    assert np.isfinite(got).all() and (got != y0).any(1).all(), "every row must have moved"


# ---- 6. independence and determinism --------------------------------------------------------------------------------------------
def test_rows_are_independent():
    c = PI.main_case()
    t = _fitted_tsne(c["X"], c["Y"])
    zd = _dev(c["Z"])
    whole = t.transform(zd)
    kl_whole = t.transform_kl_.clone()
    assert whole.shape == (131, 2) and whole.is_cuda and t.transform_kl_.dtype == torch.float64
    a, kl_a = t.transform(zd[:1]), t.transform_kl_.clone()
    b, kl_b = t.transform(zd[1:]), t.transform_kl_.clone()
    assert torch.equal(torch.cat([a, b]), whole) and torch.equal(torch.cat([kl_a, kl_b]), kl_whole)
    small = t.transform(zd, batch_rows=64)
    assert torch.equal(small, whole) and torch.equal(t.transform_kl_, kl_whole)
    assert torch.equal(t.transform(zd), whole)
    given = t.transform(zd, initialization=np.array(c["y0"]))     # the median start, handed in as an array
    assert torch.equal(given, whole)


def test_both_layouts_same_bits():
    """g2v_tsne_place_descent runs few rows a workgroup each and many rows a lane each: the 131 rows alone, and as the first rows of
    70001, end with the same bits (25 steps, the clip engaged), and so do their KL, Z and gradient"""
    from gesture2vec_amd import ops
    c, Yd, idxd, pd = _main_dev()
    m, M = len(c["idx"]), 70001
    src = np.arange(M) % m
    rng = np.random.default_rng(12)
    y0 = (c["y0"][src] + 2.0 * rng.normal(size=(M, 2))).astype(np.float32)
    few, many = _dev(y0[:m]), _dev(y0)
    out_few = ops.tsne_place_descent(Yd, idxd, pd, few, n_iter=25, **STEP_KW)
    out_many = ops.tsne_place_descent(Yd, _dev(c["idx"][src], np.int32), _dev(c["p"][src]), many, n_iter=25, **STEP_KW)
    assert torch.equal(few, many[:m]) and not torch.equal(few, _dev(y0[:m]))
    for name in ("kl", "zsum", "grad"):
        assert torch.equal(out_few[name], out_many[name][:m]), name


# ---- 7. end to end --------------------------------------------------------------------------------------------------------------
def test_end_to_end():
    from gesture2vec_amd.embedding import LatentMap
    X, lx, Z, lz = PI.clusters(6, 100, 20, 16, 21)
    lm = LatentMap(sample_size=None).fit(_dev(X))
    assert lm.coords_.shape == (600, 2) and np.array_equal(_host(lm.rows_), np.arange(600))
    zd = _dev(Z)
    lm.transform(zd, n_iter=0)
    kl_start = _host(lm.tsne.transform_kl_)
    placed = _host(lm.transform(zd)).astype(np.float64)
    kl = _host(lm.tsne.transform_kl_)
    Y = _host(lm.coords_)
    centroids = np.stack([Y[lx == k].mean(0) for k in range(6)])
    nearest = ((placed[:, None, :] - centroids[None]) ** 2).sum(2).argmin(1)
    ref0 = PR.place(X, Y, Z, n_iter=0)
    ref = PR.place(X, Y, Z)
    fell, fell_ref = float((kl < kl_start).mean()), float((ref["kl"] < ref0["kl"]).mean())
    print(f"end to end: {float((nearest == lz).mean()):.3f} of the new rows nearest to their own cluster; mean KL {kl_start.mean():.4f} -> "
          f"{kl.mean():.4f} (restatement {ref0['kl'].mean():.4f} -> {ref['kl'].mean():.4f}); KL fell in {fell:.3f} of the rows "
          f"(restatement {fell_ref:.3f})")
    assert (nearest == lz).all()
    assert kl.mean() < kl_start.mean()
    assert fell >= fell_ref - 0.02
    back = pickle.loads(pickle.dumps(lm))                          # no device state in the pickle
    assert not back.coords_.is_cuda and not back.tsne.fit_rows_.is_cuda and not back.tsne.embedding_.is_cuda
    assert not back.tsne.transform_kl_.is_cuda and torch.equal(back.transform(zd), lm.transform(zd))

    every = LatentMap(sample_size=400, random_state=2, max_iter=250)
    xd = _dev(X)
    coords, fitted = every.fit_all(xd)
    assert coords.shape == (600, 2) and fitted.dtype == torch.bool and int(fitted.sum().item()) == 400
    assert np.array_equal(_host(every.rows_), np.random.RandomState(2).permutation(600)[:400])
    assert torch.equal(coords[every.rows_], every.coords_)
    assert torch.equal(coords[~fitted], every.transform(xd[~fitted].contiguous()))


# ---- 8. scripts/embed_latents.py ------------------------------------------------------------------------------------------------
def test_embed_latents_script_places(golden_dir, tmp_path):
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    import embed_latents
    from utils.train_utils import load_checkpoint_and_model
    ckpt = os.path.join(golden_dir, "plain_ae_ckpt.bin")
    args, _, _, _, pose_dim = load_checkpoint_and_model(ckpt, DEV, "autoencoder_vq")
    gen = torch.Generator().manual_seed(5)
    np.save(tmp_path / "real.npy", torch.randn(200, int(args.n_poses), pose_dim, generator=gen).numpy())
    np.save(tmp_path / "made.npy", torch.randn(37, int(args.n_poses), pose_dim, generator=gen).numpy())
    common = ["--checkpoint", ckpt, "--device", DEV, "--max-iter", "250"]
    fit = embed_latents.main(common + ["--chunks", str(tmp_path / "real.npy"), "--sample-rows", "120", "--seed", "4", "--place-rest",
                                       "--save-map", str(tmp_path / "map.pk"), "--out", str(tmp_path / "real.npz")])
    saved = np.load(tmp_path / "real.npz")
    sample = np.random.RandomState(4).permutation(200)[:120]
    assert saved["coords"].shape == (200, 2) and np.isfinite(saved["coords"]).all() and np.array_equal(saved["rows"], np.arange(200))
    assert saved["fitted"].sum() == 120 and saved["fitted"][sample].all() and np.array_equal(fit["coords"], saved["coords"])
    with open(tmp_path / "map.pk", "rb") as f:
        lm = pickle.load(f)
    assert np.array_equal(lm.coords_.numpy(), saved["coords"][sample])
    res = embed_latents.main(common + ["--chunks", str(tmp_path / "made.npy"), "--map", str(tmp_path / "map.pk"),
                                       "--out", str(tmp_path / "made.npz"), "--scatter-txt", str(tmp_path / "scatter.txt")])
    made = np.load(tmp_path / "made.npz")
    assert made["coords"].shape == (37, 2) and np.isfinite(made["coords"]).all() and made["codes"].shape == (37,)
    assert np.array_equal(res["coords"], made["coords"])
    lines = open(tmp_path / "scatter.txt").read().split("\n")
    assert lines[0] == "512" and len(lines) == 39 and lines[-1] == ""
    assert lines[1] == "{},{:.3f},{:.3f}".format(int(made["codes"][0]), made["coords"][0, 0], made["coords"][0, 1])
