"""Joint angles from generated clips on the device (csrc/clip_angles.hip, gesture2vec_amd/generate.py) against scipy 1.15.3's
recorded values (tests/golden/clip_angles.npz) and the float64 restatements of tests/_clip_angles_ref.py.

Bars, from the number formats alone:
* angles: 2e-5 degrees, modulo 360.  The kernel computes in float64 and rounds ONCE to float32: at most half an ulp of a value
  below 256, 180 * 2^-24 = 1.07e-5 degrees, doubled.  The inputs of the angle-by-angle comparison are the fixture's 512 noisy
  matrices (|X| < 80 degrees and determinant > 0 under both methods, asserted where the fixture is made and again in
  tests/test_clip_angles_host.py) and 12 exact rotations that reach every Markley branch; every row of a call is compared.
  "procrustes" is held to scipy's recorded angles and to the restatement, "markley" to the restatement (scipy 1.10.1 is not
  installed where the fixture is recorded).
* at the lock (X = +-90 degrees) Z and Y are not separately determined: the rotation Rz Rx Ry rebuilt from the float32 angles is
  compared entrywise at 1e-6 (three angles, each off by at most 1.9e-7 rad).
* spline: 2e-5 for data within [-180, 180], the same single rounding.
* clip_angles end to end: 1.07e-5 * (1 + |S|_inf), S the spline's operator at the clip's length taken from the restatement: the
  rounding of the angles carried through the spline plus the rounding of its output.

Largest errors on the MI355X: angles 7.6e-6 degrees (both methods, against scipy and the restatement); rebuilt lock rotations 1.2e-7;
spline 7.6e-6 against the restatement, 4.9e-6 against scipy, 7.3e-6 against polyfit at p = 0; clip_angles 1.1e-5 (bar 2.4e-5)."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

import _clip_angles_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANGLE_BAR = 2e-5
SPLINE_BAR = 2e-5
ROUND = 180.0 * 2.0 ** -24
NAN_BITS = 0x7FC00000


@pytest.fixture(scope="module")
def G():
    from gesture2vec_amd import _lib, generate
    assert _lib.load().g2v_device_ok() == 1, "no gfx950 device visible"
    return generate


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "clip_angles.npz"))


@pytest.fixture(scope="module")
def pool(fx):
    """the matrices every conversion case draws from (float32), their references per method, computed once"""
    m = np.concatenate([fx["noisy"], fx["exact"].astype(np.float32)])
    ref = {method: R.euler_zxy(m, method) for method in R.METHODS}
    scipy_zxy = np.concatenate([fx["noisy_zxy"], np.full((12, 3), np.nan)])          # recorded for the noisy rows only
    return m, ref, scipy_zxy


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- conversion -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", R.METHODS)
@pytest.mark.parametrize("J,N", [(1, 1), (1, 63), (1, 64), (1, 65), (15, 130), (2, 4097)])
def test_angles_match_scipy_and_the_restatement(pool, J, N, method):
    from gesture2vec_amd import ops
    m, ref, scipy_zxy = pool
    idx = (np.arange(N * J) * 129 + 7 * N) % m.shape[0]                 # 129 and 524 are coprime: a long call visits every row
    if N * J >= m.shape[0]:
        assert np.unique(idx).size == m.shape[0]
    frames = _dev(m[idx].reshape(N, 9 * J))
    out, bad = ops.rotmat_to_euler(frames, J, ops.ROT_METHODS[method])
    assert out.shape == (N, 3 * J) and out.dtype == torch.float32 and int(bad.item()) == 0
    got = out.cpu().numpy().reshape(N * J, 3)
    err = R.angle_diff(got, ref[method][idx])
    print(f"{method} J = {J} N = {N}: {err.max():.2e} degrees off the restatement")
    assert err.max() <= ANGLE_BAR
    if method == "procrustes":
        rec = ~np.isnan(scipy_zxy[idx, 0])
        err_s = R.angle_diff(got[rec], scipy_zxy[idx][rec])
        print(f"   {err_s.max():.2e} degrees off scipy's recorded angles ({int(rec.sum())} rows)")
        assert rec.any() and err_s.max() <= ANGLE_BAR
    assert (np.abs(got[:, 1]) <= 90.0).all() and (np.abs(got) <= 180.0).all()
    out2, _ = ops.rotmat_to_euler(frames, J, ops.ROT_METHODS[method])
    assert _same(out, out2)


@pytest.mark.parametrize("method", R.METHODS)
def test_every_markley_branch(fx, method):
    from gesture2vec_amd import ops
    m = fx["exact"].astype(np.float32)
    branch = R.markley_branch(m)
    assert set(branch.tolist()) == {0, 1, 2, 3} and all((branch == k).sum() >= 2 for k in range(4))
    if method == "procrustes":
        assert set(R.markley_branch(R.procrustes(m)).tolist()) == {0, 1, 2, 3}
    out, bad = ops.rotmat_to_euler(_dev(m.reshape(1, -1)), m.shape[0], ops.ROT_METHODS[method])
    err = R.angle_diff(out.cpu().numpy().reshape(-1, 3), R.euler_zxy(m, method))
    assert int(bad.item()) == 0 and err.max() <= ANGLE_BAR, err.max(axis=1)
    assert R.angle_diff(out.cpu().numpy().reshape(-1, 3), fx["exact_zxy"]).max() <= 1e-4        # float32 entries: 6e-8 rad each


def _lock_rows():
    exact = (R.zxy_matrix(np.array([(z, x, 0) for x in (90, -90) for z in (0, 90, 180, -90)], dtype=np.float64)).round() + 0.0)
    exact = exact.astype(np.float32)
    near = []
    for k in (1, 2, 4):
        shrunk = exact.copy()
        for _ in range(k):
            shrunk = np.nextafter(shrunk, np.float32(0))                # every +-1 entry k ulps towards zero ...
        near.append(shrunk + np.where(exact == 0, np.float32(k * 2.0 ** -24), np.float32(0)))       # ... every zero k ulps up
        tilt = exact.copy()
        tilt[:, 2, 1] = np.where(exact[:, 2, 1] > 0, 1, -1) * np.float32(1 - k * 2.0 ** -24)       # only sin X moves
        near.append(tilt)
    return exact, np.concatenate(near).astype(np.float32)


@pytest.mark.parametrize("method", R.METHODS)
def test_lock_rows(method):
    from gesture2vec_amd import ops
    exact, near = _lock_rows()
    assert np.array_equal(np.abs(exact).sum(axis=(1, 2)), np.full(8, 3.0)) and (np.abs(exact[:, 2, 1]) == 1).all()
    m = np.concatenate([exact, near])
    out, bad = ops.rotmat_to_euler(_dev(m.reshape(-1, 9)), 1, ops.ROT_METHODS[method])
    got = out.cpu().numpy()
    assert int(bad.item()) == 0 and not np.isnan(got).any()
    assert (got[:8, 2] == 0).all() and (np.abs(got[:8, 1]) == 90).all()
    assert R.angle_diff(got[:8, 0], [0, 90, 180, -90, 0, 90, 180, -90]).max() == 0
    ref = R.euler_zxy(m, method)
    assert (ref[:8, 2] == 0).all()
    err = np.abs(R.zxy_matrix(got) - R.zxy_matrix(ref)).max(axis=(1, 2))
    print(f"{method}: rebuilt rotations of {m.shape[0]} lock rows within {err.max():.2e}")
    assert err.max() <= 1e-6


@pytest.mark.parametrize("method", R.METHODS)
def test_non_positive_determinants(G, pool, method):
    from gesture2vec_amd import ops
    m = pool[0][:30].copy().reshape(10, 3, 3, 3)
    clean, _ = ops.rotmat_to_euler(_dev(m.reshape(10, 27)), 3, ops.ROT_METHODS[method])
    m[2, 1] = 0.0
    m[7, 2] = np.diag([1.0, 1.0, -1.0]).astype(np.float32) + np.float32(0.01) * m[7, 2]
    frames = _dev(m.reshape(10, 27))
    out, bad = ops.rotmat_to_euler(frames, 3, ops.ROT_METHODS[method])
    assert int(bad.item()) == 2
    nan = torch.isnan(out).cpu().numpy()
    want = np.zeros((10, 9), dtype=bool)
    want[2, 3:6] = want[7, 6:9] = True
    assert np.array_equal(nan, want)
    keep = torch.from_numpy(~want).to(DEV)
    assert torch.equal(_bits(out)[keep], _bits(clean)[keep])             # the neighbours keep their bits
    out, bad = ops.rotmat_to_euler(frames, 3, ops.ROT_METHODS[method], bad=bad)
    assert int(bad.item()) == 4                                          # the counter is added to: the caller clears it
    with pytest.raises(ValueError, match="2 of 30 matrices"):
        G.rotmat_to_euler(frames, nearest=method)
    from gesture2vec_amd import _lib
    lib = _lib.load()
    sentinel = torch.full((10, 9), 7.0, device=DEV)
    for args in ((0, 3, 0), (10, 0, 0), (10, 3, 2), (10, 3, -1)):
        rc = lib.g2v_rotmat_to_euler(frames.data_ptr(), sentinel.data_ptr(), bad.data_ptr(), args[0], args[1], args[2],
                                     torch.cuda.current_stream().cuda_stream)
        assert rc == -1, args
    torch.cuda.synchronize()
    assert (sentinel == 7.0).all() and int(bad.item()) == 4


# ---- spline -----------------------------------------------------------------------------------------------------------------------
SPLINE_CASES = [(2, 1, 1), (3, 1, 45), (4, 64, 1), (5, 13, 5), (6, 4, 45), (34, 1, 45), (34, 5, 13), (340, 4, 45), (340, 1, 1),
                (4099, 1, 3)]
_spline_cache = {}


def _spline_case(fx, F, B, Cn):
    """y (B, F, Cn) float32 within [-180, 180]; where the fixture has this F its 4 columns are the first columns of the call"""
    key = (F, B, Cn)
    if key not in _spline_cache:
        cols = R.spline_data(F, B * Cn, 77 * F + B)
        rec = None
        if f"spline_y_{F}" in fx.files:
            k = min(4, B * Cn)
            cols[:, :k] = fx[f"spline_y_{F}"][:, :k]
            rec = fx[f"spline_s_{F}"][:, :k]
        assert np.abs(cols).max() <= 180.0
        y = np.ascontiguousarray(cols.reshape(F, B, Cn).transpose(1, 0, 2))
        _spline_cache[key] = (y, R.smoothing_spline(y, 0.5, axis=1), rec)
    return _spline_cache[key]


def _ws_bytes(B, F, Cn):
    from gesture2vec_amd import _lib
    return int(_lib.load().g2v_smoothing_spline_workspace(B, F, Cn))


@pytest.mark.parametrize("F,B,Cn", SPLINE_CASES)
def test_spline_values(G, fx, F, B, Cn):
    from gesture2vec_amd import ops
    y, ref, rec = _spline_case(fx, F, B, Cn)
    assert _ws_bytes(B, F, Cn) == 8 * (F - 2) * (3 + B * Cn)
    yd = _dev(y)
    out = G.smoothing_spline(yd, 0.5)
    got = out.cpu().numpy()
    assert got.shape == (B, F, Cn) and got.dtype == np.float32
    err = np.abs(got - ref).max()
    print(f"F = {F}, B = {B}, Cn = {Cn}: {err:.2e} off the restatement")
    assert err <= SPLINE_BAR
    if rec is not None:
        cols = got.transpose(1, 0, 2).reshape(F, B * Cn)[:, :rec.shape[1]]
        err_s = np.abs(cols - rec).max()
        print(f"   {err_s:.2e} off scipy's make_smoothing_spline")
        assert err_s <= SPLINE_BAR
    if F == 2:
        assert _same(out, yd)
    assert _same(G.smoothing_spline(yd, 1.0), yd)                        # p = 1: y, bit for bit
    assert _same(G.smoothing_spline(yd, 0.5), out)                       # the same call twice
    # a workspace full of NaN patterns, and one of exactly the size asked for
    need = _ws_bytes(B, F, Cn)
    ws = torch.full((need // 4 + 1,), float("nan"), device=DEV).view(torch.uint8)[:max(need, 1)]
    assert _same(ops.smoothing_spline(yd, 0.5, ws=ws), out)
    inplace = yd.clone()
    assert ops.smoothing_spline(inplace, 0.5, out=inplace) is inplace and _same(inplace, out)      # out may be y itself
    if F <= 64:                                                          # p = 0: the least-squares straight line
        x = np.arange(F, dtype=np.float64)
        cols = y.transpose(1, 0, 2).reshape(F, B * Cn).astype(np.float64)
        slope, offset = np.polyfit(x, cols, 1)                           # (per column)
        line = np.outer(x, slope) + offset
        got0 = G.smoothing_spline(yd, 0.0).cpu().numpy().transpose(1, 0, 2).reshape(F, B * Cn)
        err0 = np.abs(got0 - line).max()
        print(f"   p = 0: {err0:.2e} off polyfit")
        assert err0 <= SPLINE_BAR


def test_spline_refusals_write_nothing(fx):
    from gesture2vec_amd import _lib
    lib = _lib.load()
    B, F, Cn = 2, 34, 5
    y = _dev(_spline_case(fx, 34, 5, 13)[0][:2, :, :5])
    need = _ws_bytes(B, F, Cn)
    ws = torch.zeros(need + 8, dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 8 == 0
    out = torch.full((B, F, Cn), 7.0, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def call(smooth=0.5, b=B, f=F, cn=Cn, wsp=ws.data_ptr(), nbytes=need, yp=y.data_ptr(), op=out.data_ptr()):
        return lib.g2v_smoothing_spline(yp, op, smooth, b, f, cn, wsp, nbytes, st)

    assert call(nbytes=need - 1) == _lib.ERR_WORKSPACE and call(nbytes=0) == _lib.ERR_WORKSPACE
    assert call(smooth=1.0, nbytes=need - 8) == _lib.ERR_WORKSPACE       # whatever smooth is
    for kw in (dict(smooth=-1e-9), dict(smooth=1.0 + 1e-9), dict(smooth=float("nan")), dict(b=0), dict(f=1), dict(f=0), dict(cn=0),
               dict(yp=None), dict(op=None), dict(wsp=None), dict(wsp=ws.data_ptr() + 4)):
        assert call(**kw) == _lib.ERR_ARG, kw
    assert call(f=(1 << 20) + 1) == _lib.ERR_UNSUPPORTED and call(b=1 << 16, cn=1 << 15) == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert not (out == 7.0).any()


def test_a_clip_does_not_depend_on_its_batch(G, fx):
    y = _dev(_spline_case(fx, 34, 5, 13)[0])
    whole = G.smoothing_spline(y, 0.5)
    assert _same(G.smoothing_spline(y[:1].contiguous(), 0.5), whole[:1])
    assert _same(G.smoothing_spline(y[3:].contiguous(), 0.5), whole[3:])


# ---- end to end -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", R.METHODS)
def test_clip_angles_is_conversion_then_spline(G, pool, method):
    B, F, J = 3, 68, 15
    m = pool[0]
    idx = (np.arange(B * F * J) * 131 + 5) % 512                         # the noisy rows
    frames = m[idx].reshape(B, F, 9 * J)
    raw = R.frames_to_angles(frames, method)
    assert (180.0 - np.abs(raw)).min() > 1e-3                            # no angle where a rounding could flip +-180
    want = R.smoothing_spline(raw, 0.5, axis=1)
    gain = np.abs(R.smoothing_spline(np.eye(F), 0.5)).sum(axis=1).max()  # |S|_inf at this length
    got = G.clip_angles(_dev(frames), nearest=method)
    assert got.shape == (B, F, 3 * J)
    err = np.abs(got.cpu().numpy() - want).max()
    print(f"{method}: clip_angles within {err:.2e} (bar {ROUND * (1 + gain):.2e}, |S|_inf = {gain:.3f})")
    assert err <= ROUND * (1 + gain)
    unsmoothed = G.clip_angles(_dev(frames), nearest=method, spline=None)
    assert _same(unsmoothed, G.rotmat_to_euler(_dev(frames), nearest=method))
    assert np.abs(unsmoothed.cpu().numpy() - raw).max() <= ANGLE_BAR
    assert _same(got, G.smoothing_spline(unsmoothed, 0.5))


def test_generate_gestures_script_writes_the_angles(G, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import generate_gestures
    from gesture2vec_amd.model.Autoencoder_VQVAE_model import Autoencoder_VQVAE
    J, T, K = 5, 34, 8
    args = argparse.Namespace(rep_learning_dim=9 * J, hidden_size=32, n_layers=2, dropout_prob=0.0, autoencoder_vae="False",
                              autoencoder_vq="True", autoencoder_vq_components=K, autoencoder_vq_commitment_cost=0.25, n_pre_poses=1,
                              autoencoder_conditioned="True", autoencoder_att="False", autoencoder_fixed_weight="False", n_poses=T,
                              loss_l1_weight=5.0, loss_cont_weight=0.1, loss_var_weight=0.5, learning_rate=5e-4, epochs=10,
                              data_mean=np.tile(np.eye(3).reshape(-1), J).tolist(), data_std=[0.05] * (9 * J))
    torch.manual_seed(12)
    net = Autoencoder_VQVAE(args, 9 * J, T)
    ck = os.path.join(tmp_path, "vq_checkpoint.bin")
    torch.save({"args": args, "epoch": 1, "lang_model": None, "pose_dim": 9 * J, "gen_dict": net.state_dict()}, ck)
    out, ang = os.path.join(tmp_path, "clips.npy"), os.path.join(tmp_path, "angles.npy")
    common = ["--autoencoder-checkpoint", ck, "--codebook", "--route", "chain", "--device", DEV, "--out", out, "--angles-out", ang]
    generate_gestures.main(common)
    clips = np.load(out)
    assert clips.shape == (K, T, 9 * J) and np.load(ang).shape == (K, T, 3 * J)
    assert (np.linalg.det(clips.reshape(K, T, J, 3, 3).astype(np.float64)) > 0).all()
    cd = _dev(clips)
    assert _same(_dev(np.load(ang)), G.clip_angles(cd))                  # the defaults: markley, smooth = 0.5
    generate_gestures.main(common + ["--rotation-fit", "procrustes", "--spline-smooth", "0.9"])
    assert np.array_equal(np.load(out), clips)
    assert _same(_dev(np.load(ang)), G.clip_angles(cd, nearest="procrustes", spline=0.9))
    generate_gestures.main(common + ["--spline-smooth", "none"])
    assert _same(_dev(np.load(ang)), G.clip_angles(cd, spline=None))
