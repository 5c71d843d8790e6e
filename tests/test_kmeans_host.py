"""CPU-only tests of the k-means surface (gesture2vec_amd/kmeans.py): the float64 restatement the GPU tests are judged by reproduces
sklearn's recorded fits (tests/golden/kmeans.npz), the model pickles without device state, `from_centers`, and the refusals.  No
kernel is launched."""
import argparse
import os
import pickle
import sys

import numpy as np
import pytest
import torch

import _kmeans_inputs as KI
import _kmeans_ref as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "kmeans.npz"))


@pytest.mark.parametrize("name", list(KI.CASES))
def test_restatement_reproduces_the_recorded_sklearn_fit(fx, name):
    N, E, K, seed = KI.CASES[name]
    X, init = KI.make(N, E, K, seed)
    assert KI.sha(X) == str(fx[f"{name}_sha_x"]) and KI.sha(init) == str(fx[f"{name}_sha_init"]), "the seeded inputs moved"
    ref = KR.lloyd(X, init, track_gap=True)
    assert ref["n_iter"] == int(fx[f"{name}_n_iter"])
    assert np.array_equal(ref["labels"], fx[f"{name}_labels"].astype(np.int64))
    assert ref["relocated"] == 0 and ref["min_gap"] > 1e-5
    KI.check_centers(fx, name, ref["centers"], 1e-6 * float(np.abs(X).max()))
    assert abs(ref["inertia"] - float(fx[f"{name}_inertia"])) <= 1e-6 * ref["inertia"]     # (sklearn sums in fp32)


def test_restatement_relocation_rule():
    """A self-check of the yardstick (it touches tests/_kmeans_ref.py only; the device is held to it in tests/test_gpu_kmeans.py):
    three duplicated initial centres leave three clusters empty at the first step: they take the three farthest rows, farthest
    first, in ascending cluster id, and the donors lose them"""
    X, init = KI.make(500, 16, 12, 7)
    init = init.copy()
    init[[3, 7, 9]] = init[0]
    lab, _ = KR.assign(X, init)
    assert not np.isin([3, 7, 9], lab).any()
    u = KR.update(X, lab, init)
    d = ((X.astype(np.float64) - init.astype(np.float64)[lab]) ** 2).sum(axis=1)
    far = np.argsort(-d, kind="stable")[:3]
    assert u["relocated_rows"] == [int(r) for r in far]
    for k, r in zip((3, 7, 9), far):
        assert u["counts"][k] == 1 and np.array_equal(u["centers"][k], X[r])
    assert u["counts"].sum() == 500
    plain = KR.update(X, lab, init, relocate=False)
    donors = np.unique(lab[far])
    for k in donors:
        assert u["counts"][k] == plain["counts"][k] - int((lab[far] == k).sum())


def test_restatement_kmeans_pp_matches_the_record(fx):
    N, E, K, seed, rs_seed = KI.PP_CASE
    X, _ = KI.make(N, E, K, seed)
    assert KI.sha(X) == str(fx["pp_sha_x"])
    pp = KR.kmeans_pp(X, K, np.random.RandomState(rs_seed))
    assert pp["rows"] == fx["pp_rows"].tolist()
    assert pp["target_sep"] > 1e-6 and pp["pot_sep"] > 1e-6
    assert len(set(pp["rows"])) == K


def test_pickle_round_trip_carries_no_device_state(tmp_path):
    from gesture2vec_amd.kmeans import KMeans
    X, init = KI.make(200, 16, 5, 3)
    km = KMeans.from_centers(init)
    km.labels_ = np.arange(200, dtype=np.int32) % 5
    km.inertia_, km.n_iter_ = 12.5, 7
    km._dev = {"cuda:0": ("not", "picklable device state")}
    path = tmp_path / "clusters" / "kmeans_model.pk"
    path.parent.mkdir()
    with open(path, "wb") as f:
        pickle.dump(km, f)
    with open(path, "rb") as f:
        back = pickle.load(f)
    assert back._dev == {} and km._dev != {}
    assert np.array_equal(back.cluster_centers_, init) and back.cluster_centers_.dtype == np.float32
    assert np.array_equal(back.labels_, km.labels_) and back.inertia_ == 12.5 and back.n_iter_ == 7
    assert (back.n_clusters, back.max_iter, back.tol, back.check_every) == (5, 2500, 1e-4, 1)
    given = KMeans(n_clusters=5, init=torch.from_numpy(init))
    assert isinstance(pickle.loads(pickle.dumps(given)).init, np.ndarray)


def test_from_centers_and_constructor_defaults():
    from gesture2vec_amd.kmeans import KMeans
    km = KMeans()
    assert (km.n_clusters, km.init, km.n_init, km.max_iter, km.tol, km.random_state, km.check_every) == \
        (300, "k-means++", 1, 2500, 1e-4, 0, 1)
    c = np.arange(12, dtype=np.float64).reshape(3, 4)
    fc = KMeans.from_centers(c)
    assert fc.n_clusters == 3 and fc.cluster_centers_.dtype == np.float32 and np.array_equal(fc.cluster_centers_, c)
    assert np.array_equal(KMeans.from_centers(torch.from_numpy(c)).cluster_centers_, c)
    with pytest.raises(ValueError):
        KMeans.from_centers(np.zeros(4))
    with pytest.raises(ValueError):
        KMeans(n_clusters=0)


def test_package_does_not_import_sklearn():
    import subprocess
    code = "import sys; import gesture2vec_amd.kmeans, gesture2vec_amd.metrics, gesture2vec_amd.pipeline; print('sklearn' in sys.modules)"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, check=True).stdout
    assert out.strip() == "False"


def test_cpu_tensors_raise():
    from gesture2vec_amd.kmeans import KMeans
    X, init = KI.make(64, 16, 4, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KMeans(n_clusters=4, init=init).fit(torch.from_numpy(X))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KMeans.from_centers(init).predict_device(torch.from_numpy(X))
    with pytest.raises(RuntimeError, match="not fitted"):
        KMeans(n_clusters=4).predict_device(torch.from_numpy(X))


def test_chunks_to_codes_without_kmeans_still_raises():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from gesture2vec_amd.pipeline import chunks_to_codes
    from model.Autoencoder_VQVAE_model import Autoencoder_VQVAE
    a = argparse.Namespace(rep_learning_dim=40, hidden_size=200, n_layers=2, dropout_prob=0.0, autoencoder_vae="False",
                           autoencoder_vq="False", autoencoder_vq_components=512, autoencoder_vq_commitment_cost=0.25, n_pre_poses=1,
                           autoencoder_conditioned="True", autoencoder_att="False", autoencoder_fixed_weight="False", n_poses=20)
    net = Autoencoder_VQVAE(a, 40, 20)
    with pytest.raises(ValueError, match="no quantiser"):
        chunks_to_codes(net, torch.zeros(2, 20, 40))
    with pytest.raises(ValueError, match="no quantiser"):
        chunks_to_codes(net, torch.zeros(2, 20, 40), kmeans=None)


def test_new_exports_are_declared_and_bound():
    from gesture2vec_amd import _lib
    lib = _lib.load()
    for name in ("g2v_kmeans_update", "g2v_kmeans_update_workspace", "g2v_kmeans_commit", "g2v_kmeans_tolerance",
                 "g2v_kmeans_tolerance_workspace", "g2v_kmeans_pp_step", "g2v_kmeans_pp_workspace", "g2v_kmeans_pp_blocks"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.g2v_kmeans_update_workspace(4133, 400, 300) > 0
    assert lib.g2v_kmeans_update_workspace(100, 516, 3) == 0
    assert lib.g2v_kmeans_pp_blocks(1025) == 2
    rc = lib.g2v_kmeans_update(None, None, None, None, 4, 4, 4, 1, None, None, None, None, None, None, None, 0, None)
    assert rc == -1 and b"null" in lib.g2v_last_error()
