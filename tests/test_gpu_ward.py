"""Device-side Ward clustering (csrc/ward.hip, gesture2vec_amd/agglomerative.py) against sklearn's recorded tree and labels
(tests/golden/ward.npz) and the float64 restatement (tests/_ward_ref.py): the distance matrix at tile edges, children_, labels_ and
distances_ of every fixture, the threshold fit, N = 2, cut(k), repeatability over calls and check_every, duplicate rows, the symmetry
of the matrix after the rounds, a row stride, the refusals and scripts/cluster_latents.py --algorithm ward.

Bounds.  Distances: a pair that is not near carries 8 E 2^-53 relative (the Gram form's E 2^-53 (n_i + n_j) against
d^2 >= (n_i + n_j) / 8), 3.5e-13 at E = 400, and a near pair the few ulps of a float64 sum of squares of differences; the bar is 1e-11.
Heights: a merge height is reached through at most N updates of a few ulps each, <= 10 N 2^-53 = 4e-13 at N = 300; the bar is 1e-9,
the margin left for the subtraction in the update.  children_ and labels_ are compared exactly: the fixture's rows keep every
decision (a row's two nearest neighbours, two consecutive heights) more than 1e-7 relative apart."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

import _ward_inputs as WI
import _ward_ref as WR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"

from gesture2vec_amd import ops  # noqa: E402
from gesture2vec_amd.agglomerative import AgglomerativeClustering as AC  # noqa: E402


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "ward.npz"))


def _dev(X):
    return torch.from_numpy(np.ascontiguousarray(X)).to(DEV)


def _rows(X):
    """the rows on the device with a row stride of whole 16-byte vectors, as the C entry wants them (fit pads by itself)"""
    N, E = X.shape
    pad = torch.zeros(N, (E + 3) // 4 * 4, device=DEV)
    pad[:, :E] = _dev(X)
    return pad[:, :E]


def _bits(t):
    return t.contiguous().view(torch.int64)


def _rel(got, want):
    return float(np.max(np.abs(got - want) / want))


# ---- 1. the distance matrix ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,E", [(63, 37), (64, 400), (65, 32), (257, 3)])
def test_distances_against_float64_from_differences(N, E):
    X = WI.blobs(N, E, 7 * N + E)
    X[N // 2] = X[1]                                              # a bitwise duplicate: 0 apart exactly
    want = WR.distances(X)
    n = (X.astype(np.float64) ** 2).sum(1)
    near = want ** 2 < 0.125 * (n[:, None] + n[None, :])
    off = ~np.eye(N, dtype=bool)
    assert (near & off).any() and (~near & off).any()             # both evaluations are exercised
    D = ops.ward_distances(_rows(X))
    torch.cuda.synchronize()
    assert D.dtype == torch.float64 and tuple(D.shape) == (N, N)
    got = D.cpu().numpy()
    assert np.all(np.isposinf(np.diag(got)))
    assert torch.equal(_bits(D), _bits(D.t()))                    # entry (i, j) and entry (j, i): the same bits
    assert got[N // 2, 1] == 0.0 and got[1, N // 2] == 0.0
    pos = off & (want > 0)
    err_far, err_near = _rel(got[pos & ~near], want[pos & ~near]), _rel(got[pos & near], want[pos & near])
    print(f"N={N} E={E}: distances off by {err_far:.1e} (Gram form, {int((pos & ~near).sum())} pairs), {err_near:.1e} (near pairs)")
    assert max(err_far, err_near) < 1e-11


def test_row_stride():
    """a column slice of a wider tensor (ld = 48 > E = 37) is read in place and gives the bits of the contiguous rows"""
    X = WI.blobs(129, 37, 9)
    wide = torch.randn(129, 48, device=DEV)
    wide[:, 4:41] = _dev(X)
    view = wide[:, 4:41]
    assert view.stride(0) == 48 and view.data_ptr() % 16 == 0 and not view.is_contiguous()
    pad = torch.zeros(129, 40, device=DEV)
    pad[:, :37] = view
    assert torch.equal(_bits(ops.ward_distances(view)), _bits(ops.ward_distances(pad[:, :37])))
    a, b = AC(4, compute_distances=True).fit(view), AC(4, compute_distances=True).fit(_dev(X))
    assert np.array_equal(a.children_, b.children_) and np.array_equal(a.distances_, b.distances_) and torch.equal(a.labels_, b.labels_)


# ---- 2. sklearn's recorded tree and labels ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", WI.FIXTURES)
def test_against_sklearn(fx, name):
    X, children, dist = fx[f"{name}_x"], fx[f"{name}_children"].astype(np.int64), fx[f"{name}_distances"]
    N = len(X)
    ks, labels = [int(k) for k in fx[f"{name}_ks"]], fx[f"{name}_labels"].astype(np.int64)
    xd = _dev(X)
    ac = AC(n_clusters=ks[0], compute_distances=True).fit(xd)
    err = _rel(ac.distances_, dist)
    want_rounds = WR.rounds(X)["rounds"]
    print(f"{name}: {ac.n_rounds_} rounds (restatement: {want_rounds}), heights off by {err:.1e} (relative)")
    assert ac.children_.dtype == np.int64 and np.array_equal(ac.children_, children)
    assert ac.distances_.dtype == np.float64 and err < 1e-9
    assert ac.labels_.dtype == torch.int64 and ac.labels_.is_cuda and np.array_equal(ac.labels_.cpu().numpy(), labels[0])
    assert (ac.n_clusters_, ac.n_leaves_, ac.n_connected_components_, ac.n_features_in_) == (ks[0], N, 1, X.shape[1])
    assert ac.n_rounds_ == want_rounds                            # the cached neighbours find the pairs a full rescan finds
    for k, want in zip(ks[1:], labels[1:]):
        assert np.array_equal(ac.cut(k).cpu().numpy(), want)
    fresh = AC(n_clusters=ks[2])
    assert fresh.fit_predict(xd) is fresh.labels_ and np.array_equal(fresh.labels_.cpu().numpy(), labels[2])
    assert fresh.distances_ is None                               # not asked for


def test_distance_threshold(fx):
    name = WI.THRESHOLD_ON
    X, t = fx[f"{name}_x"], float(fx["threshold_t"])
    ac = AC(n_clusters=None, distance_threshold=t).fit(_dev(X))
    assert ac.n_clusters_ == int(fx["threshold_n_clusters"]) == int(np.count_nonzero(ac.distances_ >= t)) + 1
    assert np.array_equal(ac.labels_.cpu().numpy(), fx["threshold_labels"].astype(np.int64))
    assert _rel(ac.distances_, fx[f"{name}_distances"]) < 1e-9
    assert AC(n_clusters=None, distance_threshold=0.0).fit(_dev(X)).n_clusters_ == len(X)
    assert AC(n_clusters=None, distance_threshold=1e30).fit(_dev(X)).n_clusters_ == 1


# ---- 3. N = 2, cut(k), pickling ----------------------------------------------------------------------------------------------------------
def test_two_rows():
    X = np.array([[0.0, 3.0, 0.0], [4.0, 0.0, 0.0]], dtype=np.float32)
    ac = AC(2, compute_distances=True).fit(_dev(X))
    assert ac.children_.tolist() == [[0, 1]] and ac.distances_.tolist() == [5.0] and ac.n_rounds_ == 1
    assert ac.labels_.cpu().tolist() == WR.cut(2, ac.children_, 2).tolist() and ac.cut(1).cpu().tolist() == [0, 0]


def test_cut_equals_a_fresh_fit(fx):
    X = fx["blobs_257x3_x"]
    xd = _dev(X)
    ac = AC(2).fit(xd)
    for k in (1, 2, 3, 16, 100, 256, 257):
        got = ac.cut(k)
        assert got.dtype == torch.int64 and got.is_cuda and torch.equal(got, AC(k).fit(xd).labels_)
        assert len(torch.unique(got)) == k
    with pytest.raises(ValueError, match="n_clusters"):
        ac.cut(258)
    again = pickle.loads(pickle.dumps(ac))
    assert not again.labels_.is_cuda and torch.equal(again.labels_, ac.labels_.cpu())
    assert np.array_equal(again.children_, ac.children_) and torch.equal(again.cut(16), ac.cut(16).cpu())


# ---- 4. the same bits ----------------------------------------------------------------------------------------------------------------------
def test_same_bits_on_every_call_and_for_every_check_every(fx):
    for name in ("blobs_300x400", "chain"):
        xd = _dev(fx[f"{name}_x"])
        runs = [AC(5, compute_distances=True, check_every=ce).fit(xd) for ce in (4, 4, 1, 64)]
        for r in runs[1:]:
            assert np.array_equal(r.children_, runs[0].children_)
            assert np.array_equal(r.distances_.view(np.int64), runs[0].distances_.view(np.int64))
            assert torch.equal(r.labels_, runs[0].labels_) and r.n_rounds_ == runs[0].n_rounds_
    assert runs[0].n_rounds_ > 2 * 4                              # the chain: check_every = 4 was outrun several times


def _valid_tree(children, dist, N):
    """every node is consumed once, a merge names only nodes made before it, heights do not decrease"""
    used = np.sort(children.reshape(-1))
    return (np.array_equal(used, np.arange(2 * N - 2)) and np.all(children[:, 0] < children[:, 1])
            and np.all(children.max(1) < N + np.arange(N - 1)) and np.all(np.diff(dist) >= 0))


def test_duplicate_rows():
    """Exact ties: a valid tree, the same bits on every call, duplicates merged at height 0 before anything else and therefore under
    one label for every k up to the number of distinct rows"""
    X = WI.blobs(130, 37, 3)
    X[[7, 70, 129]] = X[3]
    X[50] = X[49]
    groups, distinct = ([3, 7, 70, 129], [49, 50]), 130 - 4
    xd = _dev(X)
    a, b = AC(6, compute_distances=True).fit(xd), AC(6, compute_distances=True, check_every=1).fit(xd)
    assert np.array_equal(a.children_, b.children_) and np.array_equal(a.distances_.view(np.int64), b.distances_.view(np.int64))
    assert torch.equal(a.labels_, b.labels_)
    assert _valid_tree(a.children_, a.distances_, 130)
    assert np.all(a.distances_[:4] == 0.0) and a.distances_[4] > 0.0
    assert set(a.children_[:4].reshape(-1)[a.children_[:4].reshape(-1) < 130]) == {3, 7, 70, 129, 49, 50}
    for k in (2, 6, 40, distinct):
        lab = a.cut(k).cpu().numpy()
        assert len(np.unique(lab)) == k
        for g in groups:
            assert len(set(lab[g])) == 1, (k, g)


# ---- 5. the matrix after the rounds ------------------------------------------------------------------------------------------------------
def test_matrix_stays_bitwise_symmetric_and_idle_rounds_change_nothing(fx):
    X = fx["blobs_193x37_x"]
    N = len(X)
    D = ops.ward_distances(_rows(X))
    state = ops.ward_state(N, DEV)
    seen = []
    c = ops.ward_rounds(D, state, init=True, rounds=3).cpu().numpy()
    assert 0 < c[0] < N - 1 and c[1] == 3 and c[3] + c[2] == c[0]
    assert torch.equal(_bits(D), _bits(D.t()))
    for _ in range(N):
        c = ops.ward_rounds(D, state, init=False, rounds=1).cpu().numpy()
        seen.append(int(c[2]))
        assert torch.equal(_bits(D), _bits(D.t()))
        if c[0] == N - 1:
            break
    assert c[0] == N - 1 and min(seen) >= 1                       # every round with two clusters left merged at least one pair
    size = state["size"].cpu().numpy()
    assert size[0] == N and not size[1:].any() and int(state["sizes"].cpu().numpy().max()) == N
    before, log = D.clone(), (state["pairs"].clone(), state["heights"].clone())
    c2 = ops.ward_rounds(D, state, init=False, rounds=5).cpu().numpy()
    assert c2[0] == N - 1 and c2[1] == c[1] and c2[2] == 0        # one active cluster: nothing happens
    assert torch.equal(_bits(D), _bits(before)) and torch.equal(state["pairs"], log[0]) and torch.equal(state["heights"], log[1])


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from gesture2vec_amd._lib import G2VLibraryError
    with pytest.raises(G2VLibraryError, match="E <= 512"):
        ops.ward_distances(torch.zeros(8, 516, device=DEV))
    with pytest.raises(TypeError, match="fp32"):
        AC().fit(torch.zeros(8, 4, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="at least 2 rows"):
        AC().fit(torch.zeros(1, 4, device=DEV))
    with pytest.raises(ValueError, match="n_clusters = 9 exceeds the 8 rows"):
        AC(9).fit(torch.randn(8, 4, device=DEV))
    bad = torch.randn(8, 4, device=DEV)
    bad[3, 2] = float("nan")
    with pytest.raises(ValueError, match="NaN"):
        AC().fit(bad)


# ---- 7. scripts/cluster_latents.py --algorithm ward --------------------------------------------------------------------------------------
def test_cluster_latents_ward(golden_dir, tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import cluster_latents
    from gesture2vec_amd.silhouette import silhouette_score
    from utils.train_utils import load_checkpoint_and_model
    ckpt = os.path.join(golden_dir, "plain_ae_ckpt.bin")
    args, net, _, _, pose_dim = load_checkpoint_and_model(ckpt, DEV, "autoencoder_vq")
    net.eval()
    real = torch.randn(120, int(args.n_poses), pose_dim, generator=torch.Generator().manual_seed(5))
    np.save(tmp_path / "chunks.npy", real.numpy())
    latd = cluster_latents.latents_of(net, real.to(DEV), 65536)
    ref = WR.fit(latd.cpu().numpy())
    assert ref["nn_gap"] > WI.REL_GAP and ref["height_gap"] > WI.REL_GAP      # these latents decide nothing by rounding
    common = ["--checkpoint", ckpt, "--chunks", str(tmp_path / "chunks.npy"), "--device", DEV, "--algorithm", "ward"]
    out = tmp_path / "ward.npz"
    ac = cluster_latents.main(common + ["--n_clusters", "6", "--out", str(out)])
    printed = capsys.readouterr().out
    assert "Number of clusters: 6\n" in printed and f"rounds: {ref['rounds']}\n" in printed
    saved = np.load(out)
    assert np.array_equal(saved["children"], ref["children"]) and np.array_equal(saved["labels"], WR.cut(6, ref["children"], 120))
    assert _rel(saved["heights"], ref["distances"]) < 1e-9 and np.array_equal(ac.labels_.cpu().numpy(), saved["labels"])
    t = float(0.5 * (ref["distances"][-4] + ref["distances"][-3]))
    out_t = tmp_path / "ward_t.npz"
    cluster_latents.main(common + ["--distance-threshold", repr(t), "--out", str(out_t)])
    assert "Number of clusters: 4\n" in capsys.readouterr().out
    assert np.array_equal(np.load(out_t)["labels"], WR.cut(4, ref["children"], 120))
    curve = cluster_latents.main(common + ["--scan-k", "2:9:3"])
    printed = capsys.readouterr().out
    assert [k for k, _ in curve] == [2, 5, 8] and "wrote" not in printed
    for k, sil in curve:
        assert sil == silhouette_score(latd, WR.cut(k, ref["children"], 120)) and f"k = {k}: silhouette {sil!r}\n" in printed
