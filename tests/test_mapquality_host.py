"""CPU-only: the float64 restatement of trustworthiness and continuity (tests/_mapq_ref.py) against sklearn's recorded numbers
(tests/golden/mapquality.npz), the preconditions every recorded input has to meet, the declarations the feature adds, the refusals
of the public functions and the new options of the two scripts."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import _mapq_ref as MR
from _tsne_ref import sqdist, trustworthiness as tsne_ref_trustworthiness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("g2v_neighbor_ranks_ok", "g2v_neighbor_ranks_workspace", "g2v_neighbor_ranks")


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "mapquality.npz"))


@pytest.mark.parametrize("shape", MR.SHAPES, ids=MR.name_of)
def test_restatement_equals_the_recorded_sklearn_numbers(fx, shape):
    name, k = MR.name_of(shape), shape[2]
    X, Y = fx[f"{name}_x"], fx[f"{name}_y"]
    assert X.dtype == Y.dtype == np.float32 and X.shape == shape[:2] and Y.shape == (shape[0], shape[3]) and int(fx[f"{name}_k"]) == k
    ref = MR.map_quality(X, Y, k)
    print(f"{name}: trustworthiness {ref['trustworthiness']!r}, continuity {ref['continuity']!r}")
    assert abs(ref["trustworthiness"] - float(fx[f"{name}_trust"])) <= 1e-12
    assert abs(ref["continuity"] - float(fx[f"{name}_cont"])) <= 1e-12
    assert 0.5 < ref["trustworthiness"] < 0.95 and 0.5 < ref["continuity"] < 0.95         # a wrong rank has something to move
    assert (ref["penalty_t"] > 0).mean() > 0.9 and (ref["penalty_c"] > 0).mean() > 0.9
    if shape[0] <= 130:                                           # the suite's older restatement says the same
        assert abs(tsne_ref_trustworthiness(X, Y, k) - ref["trustworthiness"]) <= 1e-12


@pytest.mark.parametrize("shape", MR.SHAPES, ids=MR.name_of)
def test_preconditions_hold_on_the_generic_inputs(fx, shape):
    name, k = MR.name_of(shape), shape[2]
    X, Y = fx[f"{name}_x"], fx[f"{name}_y"]
    ax, ay = MR.selection_margin(X, k), MR.selection_margin(Y, k)
    me = np.arange(X.shape[0])
    bx = MR.closest_compared(sqdist(X), MR.nearest(sqdist(Y), k, True), me)
    by = MR.closest_compared(sqdist(Y), MR.nearest(sqdist(X), k, True), me)
    print(f"{name}: (a) {ax:.2f} / {ay:.2f} of the margin, (b) {bx:.2e} / {by:.2e} relative")
    assert ax > 1.0 and ay > 1.0
    assert bx > MR.REL_SEP and by > MR.REL_SEP


def test_preconditions_hold_on_the_placed_and_exact_inputs(fx):
    X, Y, Z, y, k = fx["placed_x"], fx["placed_y"], fx["placed_z"], fx["placed_yz"], int(fx["placed_k"])
    assert (X.shape, Y.shape, Z.shape, y.shape, k) == ((130, 40), (130, 2), (37, 40), (37, 2), 5)
    assert MR.selection_margin(X, k, Z) > 1.0 and MR.selection_margin(Y, k, y) > 1.0
    DX, DY = MR.cross_sqdist(Z, X), MR.cross_sqdist(y, Y)
    assert MR.closest_compared(DX, MR.nearest(DY, k, False)) > MR.REL_SEP
    assert MR.closest_compared(DY, MR.nearest(DX, k, False)) > MR.REL_SEP
    X, Y = fx["exact_x"], fx["exact_y"]
    gx, gy = MR.exact_grid()
    assert np.array_equal(X, gx) and np.array_equal(Y, gy)
    assert MR.exact_in_fp32(X) and MR.exact_in_fp32(Y)
    me = np.arange(X.shape[0])
    assert MR.closest_compared(sqdist(X), MR.nearest(sqdist(Y), MR.EXACT_K, True), me) > MR.REL_SEP
    assert MR.closest_compared(sqdist(Y), MR.nearest(sqdist(X), MR.EXACT_K, True), me) > MR.REL_SEP
    DX = sqdist(X)
    assert (np.sort(DX, axis=1)[:, MR.EXACT_K] == np.sort(DX, axis=1)[:, MR.EXACT_K + 1]).any()      # ties at the k boundary
    assert (Y[:8] == Y[0]).all() and (X[10] == X[3]).all()                                           # bitwise duplicates


def test_rules_of_the_restatement():
    D = np.array([[0.0, 1.0, 1.0, 4.0, 1.0]])
    # self = 0: the others in order (1, 2, 4, 3); ties to the lower index
    assert MR.ranks_from(D, np.array([[1, 2, 4, 3, 0, -1, 5]], np.int32), [0]).tolist() == [[1, 2, 3, 4, 0, 0, 0]]
    # no self: row 0 counts
    assert MR.ranks_from(D, np.array([[0, 1, 3]], np.int32)).tolist() == [[1, 2, 5]]
    assert MR.penalties(np.array([[1, 2, 3, 7]], np.int32), 2).tolist() == [6]
    X = np.arange(12, dtype=np.float32).reshape(6, 2) ** 2
    assert np.allclose(MR.k_distances(X, 1), 0.0)
    assert np.array_equal(MR.k_distances(X, 2), np.sort(MR.kneighbors_other(X, 1)[0][:, 0]))


def test_header_and_makefile_name_the_feature():
    from gesture2vec_amd import _lib
    for name in ENTRIES:
        assert name in _lib.EXPORTS, name
    mk = open(os.path.join(ROOT, "gesture2vec_amd", "csrc", "Makefile")).read()
    assert "map_quality.hip" in re.search(r"^SRCS\s*=(.*)$", mk, re.M)[1].split()
    C = _lib.C
    assert _lib._SIGS["g2v_neighbor_ranks"] == (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int,
                                                           C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                           C.c_size_t, C.c_void_p])
    assert _lib._SIGS["g2v_neighbor_ranks_ok"] == (C.c_int, [C.c_int64, C.c_int64, C.c_int, C.c_int])


def test_served_shapes_are_answered_without_a_device():
    from gesture2vec_amd import _lib
    lib = _lib.load()
    for N, M, d, k, ok in ((1, 1, 1, 1, 1), (2 ** 24 - 1, 2 ** 31 - 1, 512, 127, 1), (2 ** 24, 8, 8, 5, 0), (8, 2 ** 31, 8, 5, 0),
                           (8, 8, 513, 5, 0), (8, 8, 0, 5, 0), (8, 8, 8, 128, 0), (8, 8, 8, 0, 0), (0, 8, 8, 5, 0), (8, 0, 8, 5, 0)):
        assert lib.g2v_neighbor_ranks_ok(N, M, d, k) == ok, (N, M, d, k)
        assert (lib.g2v_neighbor_ranks_workspace(N, M, d, k) > 0) == bool(ok), (N, M, d, k)


def test_value_errors_come_before_anything_else():
    from gesture2vec_amd.embedding import continuity, kneighbors, map_quality, placement_quality, trustworthiness
    X, Y = torch.zeros(20, 6), torch.zeros(20, 2)
    for fn in (trustworthiness, continuity):
        with pytest.raises(ValueError, match=r"n_neighbors \(10\) should be less than n_samples / 2 \(10.0\)"):
            fn(X, Y, n_neighbors=10)
    with pytest.raises(ValueError, match="should be less than n_samples / 2"):
        map_quality(X, Y, n_neighbors=12)
    with pytest.raises(ValueError, match="should be less than n_samples / 2"):
        map_quality(torch.zeros(300, 6), torch.zeros(300, 2), n_neighbors=5, sample_size=10, random_state=0)
    with pytest.raises(ValueError, match="should be less than n_samples / 2"):
        placement_quality(X, Y, torch.zeros(3, 6), torch.zeros(3, 2), n_neighbors=10)
    with pytest.raises(ValueError, match="metric must be 'euclidean', got 'cosine'"):
        trustworthiness(X, Y, n_neighbors=5, metric="cosine")
    big, bigy = torch.zeros(300, 6), torch.zeros(300, 2)
    for call in (lambda: trustworthiness(big, bigy, n_neighbors=128), lambda: continuity(big, bigy, n_neighbors=128),
                 lambda: map_quality(big, bigy, n_neighbors=128), lambda: placement_quality(big, bigy, X, Y, n_neighbors=128)):
        with pytest.raises(ValueError, match="exceeds 127"):
            call()
    for k in (0, 2.5):
        with pytest.raises(ValueError, match="positive integer"):
            trustworthiness(X, Y, n_neighbors=k)
    with pytest.raises(ValueError, match="same number of rows"):
        trustworthiness(X, Y[:10])
    with pytest.raises(TypeError):
        trustworthiness(X, Y, 5)                                  # n_neighbors is keyword-only, as in sklearn
    assert callable(kneighbors)


def test_api_refuses_cpu_tensors():
    from gesture2vec_amd import _lib, ops
    from gesture2vec_amd.dbscan import k_distances
    from gesture2vec_amd.embedding import continuity, kneighbors, map_quality, placement_quality, trustworthiness
    X, Y = torch.zeros(20, 6), torch.zeros(20, 2)
    for call in (lambda: trustworthiness(X, Y), lambda: continuity(X, Y), lambda: map_quality(X, Y),
                 lambda: placement_quality(X, Y, X[:3], Y[:3]), lambda: kneighbors(X, 3), lambda: kneighbors(X, 3, queries=X[:2]),
                 lambda: k_distances(X, 4)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(_lib.G2VLibraryError, match="no CPU path"):
        ops.neighbor_ranks(torch.zeros(20, 8), torch.zeros(20, 8), torch.zeros(20, 3, dtype=torch.int32))


def test_scripts_name_the_new_options():
    for script, opts in (("embed_latents.py", ("--quality", "--place-rest")), ("cluster_latents.py", ("--k-distances", "--algorithm"))):
        run = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script), "--help"], capture_output=True, text=True,
                             timeout=300)
        assert run.returncode == 0, run.stderr
        for opt in opts:
            assert opt in run.stdout, (script, opt)
