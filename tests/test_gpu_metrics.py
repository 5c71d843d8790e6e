"""GPU: device-side evaluation statistics (g2v_moments_accumulate, g2v_code_histogram) and gesture2vec_amd.metrics on top of them,
against float64 numpy, the reference's own Frechet values (tests/golden/metrics.npz) and the same quantities computed on the host
from chunk_latents / chunks_to_codes outputs.

Moments bound: |dS2_ij| <= 1e-6 * sum_n |x~_ni| |x~_nj| (x~ = x - shift in float64), the same for S1.  Derivation: the largest measured
fp32-MFMA chain error is 3.5e-7 * sum |a b| (K = 4096), plus 1.2e-7 for the one fp32 rounding of each shifted operand, doubled."""
import argparse
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _metrics_inputs as MI

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-6
PAD = {1: 0, 17: 5, 1000: 4, 4096: 0, 65536 + 3: 8}            # row stride = E + PAD[N]; 5: rows that are not 16-byte aligned


def _data(N, E, seed, pad=0):
    x = MI.latent_set(seed, N, E, 0.1, 0.3)
    buf = torch.zeros(N, E + pad, device=DEV)
    buf[:, :E] = torch.from_numpy(x)
    if pad:
        buf[:, E:] = float("nan")                                # the padding columns must never be read into a sum
    shift = x[:256].mean(0).astype(np.float32)
    return x, buf[:, :E], shift


def _accumulate(view, shift, acc=None):
    from gesture2vec_amd import ops
    E = view.shape[1]
    if acc is None:
        acc = (torch.zeros(E, dtype=torch.float64, device=DEV), torch.zeros(E, E, dtype=torch.float64, device=DEV))
    ops.moments_accumulate(view, torch.from_numpy(shift).to(DEV), acc[0], acc[1])
    return acc


def _reference(x, shift):
    d = x.astype(np.float64) - shift.astype(np.float64)
    a = np.abs(d)
    return d.sum(0), d.T @ d, a.sum(0), a.T @ a


def _ratio(got, ref, mag):
    err = np.abs(got - ref)
    assert np.all(err[mag == 0] == 0)
    return float((err[mag > 0] / mag[mag > 0]).max()) if (mag > 0).any() else 0.0


@pytest.mark.parametrize("N", [1, 17, 1000, 4096, 65536 + 3])
@pytest.mark.parametrize("E", [64, 80, 100, 128, 400, 512, 399, 3])
def test_moments_against_float64_numpy(E, N):
    x, view, shift = _data(N, E, seed=E + N, pad=PAD[N])
    assert view.stride(0) == E + PAD[N]
    s1, s2 = _accumulate(view, shift)
    torch.cuda.synchronize()
    s1, s2 = s1.cpu().numpy(), s2.cpu().numpy()
    r1, r2, m1, m2 = _reference(x, shift)
    q1, q2 = _ratio(s1, r1, m1), _ratio(s2, r2, m2)
    print(f"E={E} N={N} ld={view.stride(0)}: max |dS1| / sum|x~| = {q1:.3e}, max |dS2| / sum|x~||x~| = {q2:.3e}")
    assert np.array_equal(s2, s2.T), "S2 is not bitwise symmetric"
    assert q1 <= BOUND and q2 <= BOUND, (q1, q2)


def test_moments_are_deterministic_additive_and_mergeable():
    from gesture2vec_amd.metrics import LatentMoments
    E, cuts = 400, (0, 1000, 1000 + 4096 + 7, 1000 + 4096 + 7 + 20000)
    x, view, shift = _data(cuts[-1], E, seed=5)
    a, b = _accumulate(view, shift), _accumulate(view, shift)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "two runs on the same input differ"
    # three batches in sequence into one accumulator, and three LatentMoments merged, against one call over the concatenation
    seq = None
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        seq = _accumulate(view[lo:hi], shift, seq)
    r1, r2, m1, m2 = _reference(x, shift)
    assert _ratio(seq[0].cpu().numpy(), r1, m1) <= BOUND and _ratio(seq[1].cpu().numpy(), r2, m2) <= BOUND
    assert _ratio(a[1].cpu().numpy(), r2, m2) <= BOUND
    parts = [LatentMoments(E, DEV, shift=shift).update(view[lo:hi]) for lo, hi in zip(cuts[:-1], cuts[1:])]
    n, mu, cov = parts[0].merge(parts[1]).merge(parts[2]).finalize()
    n1, mu1, cov1 = LatentMoments(E, DEV, shift=shift).update(view).finalize()
    x64 = x.astype(np.float64)
    assert n == n1 == cuts[-1]
    # mean and covariance inherit the sums' bound: d mean = dS1 / n, d cov = (dS2 - ...) / (n - 1)
    tol_mu = BOUND * m1 / n
    tol_cov = 2.1 * BOUND * m2 / (n - 1)
    for got_mu, got_cov in ((mu, cov), (mu1, cov1)):
        assert np.all(np.abs(got_mu - x64.mean(0)) <= tol_mu)
        assert np.all(np.abs(got_cov - np.cov(x64, rowvar=False)) <= tol_cov)
    assert np.all(np.abs(mu - mu1) <= tol_mu) and np.all(np.abs(cov - cov1) <= tol_cov)
    # a first update without a shift fixes it to the mean of the first <= 256 rows
    auto = LatentMoments(E, DEV).update(view[:1000])
    assert np.abs(auto.shift.cpu().numpy() - x[:256].astype(np.float64).mean(0)).max() <= 1e-6
    with pytest.raises(ValueError, match="different shifts"):
        auto.merge(parts[1])


def test_moments_workspace_and_unsupported_width():
    import ctypes
    from gesture2vec_amd import _lib
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    N, E = 5000, 400
    x, view, shift = _data(N, E, seed=3)
    sh = torch.from_numpy(shift).to(DEV)
    nb = int(lib.g2v_moments_workspace(N, E))
    ws = torch.full((nb // 4 + 64,), float("nan"), device=DEV)           # dirty workspace: nothing is trusted across calls
    s1 = torch.zeros(E, dtype=torch.float64, device=DEV)
    s2 = torch.zeros(E, E, dtype=torch.float64, device=DEV)
    assert lib.g2v_moments_accumulate(p(view), E, p(sh), p(s1), p(s2), N, E, p(ws), nb, st) == 0
    ref = _accumulate(view, shift)
    assert torch.equal(s1, ref[0]) and torch.equal(s2, ref[1])
    before = s2.clone()
    assert lib.g2v_moments_accumulate(p(view), E, p(sh), p(s1), p(s2), N, E, p(ws), nb - 256, st) == -3
    wide = torch.zeros(8, 513, device=DEV)
    assert lib.g2v_moments_workspace(8, 513) == 0
    assert lib.g2v_moments_accumulate(p(wide), 513, p(sh), p(s1), p(s2), 8, 513, p(ws), nb, st) == -4
    torch.cuda.synchronize()
    assert torch.equal(s2, before), "a refused call touched the accumulators"


@pytest.mark.parametrize("N", [1, 4097, 2 ** 20])
def test_histogram_equals_bincount(N):
    from gesture2vec_amd import metrics, ops
    K = MI.HIST_K
    ids = MI.code_ids(N, N)
    d = torch.from_numpy(ids).to(DEV)
    assert np.array_equal(metrics.code_histogram(d, K), np.bincount(ids, minlength=K))
    counts = ops.code_histogram(d, K)
    counts = ops.code_histogram(d, K, counts)                             # accumulates
    assert np.array_equal(counts.cpu().numpy()[:K], 2 * np.bincount(ids, minlength=K)) and int(counts[K]) == 0
    bad = ids.copy()
    bad[::3] = (-1, K, 2 ** 40, -2 ** 50)[N % 4]                          # out of range: slot K, never an address
    n_bad = len(bad[::3])
    db = torch.from_numpy(bad).to(DEV)
    c = ops.code_histogram(db, K).cpu().numpy()
    keep = np.ones(N, bool)
    keep[::3] = False
    assert c[K] == n_bad and np.array_equal(c[:K], np.bincount(ids[keep], minlength=K))
    with pytest.raises(ValueError, match="outside"):
        metrics.code_histogram(db, K)


def make_args(**kw):
    d = dict(rep_learning_dim=40, hidden_size=200, n_layers=2, dropout_prob=0.0, autoencoder_vae="False", autoencoder_vq="True",
             autoencoder_vq_components=512, autoencoder_vq_commitment_cost=0.25, n_pre_poses=1, autoencoder_conditioned="True",
             autoencoder_att="False", autoencoder_fixed_weight="False", n_poses=20, loss_l1_weight=5.0, loss_cont_weight=0.1,
             loss_var_weight=0.5, learning_rate=5e-4, epochs=10)
    d.update(kw)
    return argparse.Namespace(**d)


def _net(vq="True", seed=3):
    from gesture2vec_amd.model.Autoencoder_VQVAE_model import Autoencoder_VQVAE
    torch.manual_seed(seed)
    net = Autoencoder_VQVAE(make_args(autoencoder_vq=vq), 40, 20).to(DEV)
    net.train(False)
    return net


def _chunk_sets():
    g = torch.Generator().manual_seed(11)
    real = torch.randn(8192, 20, 40, generator=g)
    gen = torch.randn(6000, 20, 40, generator=g) * 1.1 + 0.05
    return real.to(DEV), gen.to(DEV)


def _host_metrics(net, real, gen):
    """the same quantities from chunk_latents / chunks_to_codes outputs copied to the host: float64 numpy moments, np.bincount"""
    from gesture2vec_amd import metrics as M
    from gesture2vec_amd.pipeline import chunk_latents, chunks_to_codes
    lat, hist = [], []
    for x in (real, gen):
        if net.vq:
            z, codes = chunks_to_codes(net, x)
            hist.append(np.bincount(codes.cpu().numpy(), minlength=512))
        else:
            z = chunk_latents(net, x)
        lat.append(z.cpu().numpy().astype(np.float64))
    out = {"frechet": M.frechet_distance(lat[0].mean(0), np.cov(lat[0], rowvar=False), lat[1].mean(0), np.cov(lat[1], rowvar=False))}
    if net.vq:
        out.update(hellinger=M.hellinger(*hist), wasserstein=M.wasserstein(*hist), perplexity_real=M.histogram_perplexity(hist[0]),
                   perplexity_generated=M.histogram_perplexity(hist[1]))
    return out


def test_gesture_metrics_end_to_end():
    from gesture2vec_amd.metrics import gesture_metrics
    net = _net()
    real, gen = _chunk_sets()
    m = gesture_metrics(net, real, gen)
    ref = _host_metrics(net, real, gen)
    print("gesture_metrics:", m, "host:", ref)
    assert set(m) == {"frechet", "hellinger", "perplexity_real", "perplexity_generated", "wasserstein", "n_real", "n_generated"}
    assert (m["n_real"], m["n_generated"]) == (8192, 6000)
    assert abs(m["frechet"] - ref["frechet"]) <= 1e-4 * abs(ref["frechet"])
    for k in ("hellinger", "wasserstein", "perplexity_real", "perplexity_generated"):
        assert abs(m[k] - ref[k]) <= 1e-12 * abs(ref[k]), (k, m[k], ref[k])
    streamed = gesture_metrics(net, real, gen, batch_rows=3000)            # three / two batches per set
    assert abs(streamed["frechet"] - ref["frechet"]) <= 1e-4 * abs(ref["frechet"])
    assert (streamed["n_real"], streamed["n_generated"]) == (8192, 6000)


def test_gesture_metrics_without_a_quantiser_and_on_the_cpu():
    from gesture2vec_amd.metrics import gesture_metrics
    net = _net(vq="False")
    real, gen = _chunk_sets()
    m = gesture_metrics(net, real, gen)
    ref = _host_metrics(net, real, gen)
    assert abs(m["frechet"] - ref["frechet"]) <= 1e-4 * abs(ref["frechet"])
    assert all(m[k] is None for k in ("hellinger", "wasserstein", "perplexity_real", "perplexity_generated"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gesture_metrics(net, real.cpu(), gen)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gesture_metrics(net, real, gen.cpu())


@pytest.mark.parametrize("case", sorted(MI.FRECHET_CASES))
def test_reference_frechet_through_the_device_moments(golden_dir, case):
    from gesture2vec_amd.metrics import LatentMoments, frechet_distance
    fx = np.load(os.path.join(golden_dir, "metrics.npz"))
    A, B = MI.frechet_inputs(case)
    assert [MI.sha256(A), MI.sha256(B)] == list(fx[f"frechet/{case}/sha256"])
    stats = []
    for x in (A, B):
        _, mu, cov = LatentMoments(x.shape[1], DEV).update(torch.from_numpy(x).to(DEV)).finalize()
        stats += [mu, cov]
    got, ref = frechet_distance(*stats), float(fx[f"frechet/{case}/value"])
    print(f"frechet {case} through the device moments: got {got!r} ref {ref!r} rel {abs(got - ref) / abs(ref):.3e}")
    assert abs(got - ref) <= 1e-4 * abs(ref)


def test_evaluate_metrics_cli(tmp_path):
    from gesture2vec_amd.metrics import gesture_metrics
    net = _net(seed=8)
    ck = os.path.join(tmp_path, "vq_checkpoint.bin")
    torch.save({"args": make_args(), "epoch": 1, "lang_model": None, "pose_dim": 40,
                "gen_dict": {k: v.cpu() for k, v in net.state_dict().items()}}, ck)
    real, gen = _chunk_sets()
    real, gen = real[:3000], gen[:2500]
    np.save(os.path.join(tmp_path, "real.npy"), real.cpu().numpy())
    np.save(os.path.join(tmp_path, "gen.npy"), gen.cpu().numpy())
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "evaluate_metrics.py"), "--checkpoint", ck,
                        "--real", os.path.join(tmp_path, "real.npy"), "--generated", os.path.join(tmp_path, "gen.npy")],
                       cwd=os.path.join(ROOT, "scripts"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l.strip() for l in r.stdout.splitlines()]
    order = ["Perplexity: ", "hell_dist --> ", "Frechet Distance --> ", "wasserstein_distance -> "]
    found = [next(i for i, l in enumerate(lines) if l.startswith(p)) for p in order]
    assert found == sorted(found), "the four lines are not in the reference's Metrics.txt order"
    vals = [float(lines[i][len(p):]) for i, p in zip(found, order)]
    m = gesture_metrics(net, real, gen)
    for got, key in zip(vals, ("perplexity_generated", "hellinger", "frechet", "wasserstein")):
        assert abs(got - m[key]) <= 1e-12 * abs(m[key]), (key, got, m[key])
