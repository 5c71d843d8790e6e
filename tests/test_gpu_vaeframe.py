"""GPU parity of the frame-level variational autoencoder (VAE_Network; autoencoder_vq "False", autoencoder_vae "True"): both routes
against the reference's golden vectors (tests/golden/vaeframe.npz, within the stored bars, with the recorded masks and noise), the
fused step and the operator kernels against the float64 restatement (tests/_vaeframe_ref.py) at the shapes where their tiling can go
wrong, the drawn noise, determinism, the surface and the trainer.

Where no recorded bar exists (the restatement is the yardstick) the bound is worked out from the number format.  A sum of n fp32
terms in any order is off by at most n 2^-24 of its sum of |terms|, which stays within ~4 x the largest element of the result at
these sizes and N(0, 1) inputs; the device's expf is good to 1 ulp and its tanhf to 2 ulp (2^-23 and 2^-22 relative).
  STEP_TOL  the longest chain of sums behind a compared value of the fused step is the encoder gradient's: h (D = 135), mean or
            logvar (L <= 45), c (L), out (L), dc (D), dz (L), dh (2 L), dWe (B <= 155, the largest admitted batch):
            135 + 45 + 45 + 45 + 135 + 45 + 90 + 155 = 695 terms -> 4 x 695 x 2^-24 = 1.66e-4; tanh forward and backward and the two
            exponentials add 2 x 2^-22 + 2 x 2^-23 = 7e-7 -> 1.7e-4 of the largest element.
  BIG_TOL   the same chain on the staged route at (1024, 135, 200): 135 + 5 x 200 + 135 + 200 + 1024 = 2494 terms -> 5.9e-4 + 7e-7
            -> 6e-4.
  OP_TOL    the elementwise operators: at most six roundings and two exponentials behind an element: 4 x 6 x 2^-24 + 2 x 2^-23 =
            1.7e-6 -> 2e-6.  KL_TOL: the KL mean of n <= 4097 elements is a tree: 4 per thread, 6 + 2 levels per workgroup, 5
            partials, 8 + 2 levels of the finish = 27 sums deep, each term three roundings and an exponential:
            4 x 30 x 2^-24 + 2^-23 = 7.3e-6 -> 8e-6.
  ENC_TOL   encode: one contraction of length 135 and a tanh: 4 x 135 x 2^-24 + 2^-22 = 3.3e-5 -> 3.5e-5.  DEC_TOL: decode, a
            contraction of length 40: 9.6e-6 -> 1e-5; generate, two of them: 2e-5."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _vaeframe_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = argparse.Namespace(autoencoder_vq="False", autoencoder_vae="True")
STEP_TOL, BIG_TOL, OP_TOL, KL_TOL, ENC_TOL, DEC_TOL = 1.7e-4, 6e-4, 2e-6, 8e-6, 3.5e-5, 1e-5


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "vaeframe.npz"))


def tensors(state):
    return {k: torch.from_numpy(np.array(v)) for k, v in state.items()}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def build(state, shape, route, lr=5e-4):
    from gesture2vec_amd.flat import FlatClipAdam
    from gesture2vec_amd.model.DAE_model import VAE_Network
    B, D, L = shape
    net = VAE_Network(D, L)
    net.load_state_dict(tensors(state), strict=True)
    net = net.to(DEV)
    net.train(True)
    net.route = route
    return net, FlatClipAdam(net.parameters(), lr=lr, betas=(0.5, 0.999))


def observe(net, route, seen):
    """the forward values of every training iteration, without touching the product"""
    if route == "staged":
        orig = net._staged

        def staged(*a, **kw):
            r = orig(*a, **kw)
            seen.update(out=r[0].detach().squeeze(2), logvar=r[1].detach(), mean=r[2].detach(), latent=r[3].detach())
            return r
        net._staged = staged
        return
    orig = net.fused_step

    def fused_step(x, target, grads, **kw):
        res = orig(x, target, grads, want_latent=True, want_stats=True, want_out=True)
        seen.update({k: res[k] for k in R.FORWARD}, fused_calls=seen.get("fused_calls", 0) + 1)
        return res
    net.fused_step = fused_step


_RUNS = {}


def run_case(fx, tag, route):
    """the recorded iterations of case `tag` on `route`, once per module -> (net, [per step dict], final state_dict on the CPU, case)"""
    from gesture2vec_amd.train_eval.train_seq2seq import train_iter_DAE
    if (tag, route) in _RUNS:
        return _RUNS[(tag, route)]
    case = R.load_case(fx, tag)
    net, optim = build(case["state0"], case["shape"], route, case["lr"])
    seen, steps = {}, []
    observe(net, route, seen)
    for i, ((noisy, original), mask, eps) in enumerate(zip(case["data"], case["masks"], case["eps"]), 1):
        net.set_dropout_mask(dev(mask))
        net.set_latent_noise(dev(eps))
        loss = train_iter_DAE(ARGS, 1, noisy.to(DEV), original.to(DEV), net, optim)
        assert set(loss) == {"loss"} and isinstance(loss["loss"], float)
        step = dict(loss=loss["loss"], **{k: seen[k].cpu().numpy() for k in R.FORWARD})
        if i == 1:
            step["grads"] = {k: dict(net.named_parameters())[k].grad.detach().cpu().numpy().copy() for k in R.TRAINABLE}
        steps.append(step)
    if route == "fused":
        assert seen["fused_calls"] == case["steps"]
    else:
        assert "fused_calls" not in seen
    final = {k: v.detach().cpu().numpy().copy() for k, v in net.state_dict().items()}
    _RUNS[(tag, route)] = (net, steps, final, case)
    return _RUNS[(tag, route)]


class Bars:
    def __init__(self, fx):
        self.fx, self.bad = fx, []

    def check(self, name, got, ref=None, bar=None):
        ref = R.stored(self.fx, name) if ref is None else ref
        bar = float(self.fx["bar/" + name]) if bar is None else bar
        d = R.distance(R.pack(got) if not isinstance(got, dict) else got, ref)
        print(f"{name}: distance {d:.3e} bar {bar:.3e}")
        if not d <= bar:
            self.bad.append((name, d, bar))

    def whole(self, name, got, ref, bar):
        self.check(name, {"": np.asarray(got)}, ref={"": np.asarray(ref)}, bar=bar)

    def done(self):
        assert not self.bad, self.bad


# ---- 1. the recorded iterations --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["staged", "fused"])
@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_iterations_match_the_reference_golden(fx, tag, route):
    net, steps, final, case = run_case(fx, tag, route)
    bars = Bars(fx)
    for i, st in enumerate(steps, 1):
        s = f"{tag}/s{i}/"
        bars.check(s + "loss", st["loss"])
        for k in R.FORWARD:
            bars.check(s + k, st[k])
        if i == 1:
            for k in R.TRAINABLE:
                bars.check(s + "grad/" + k, st["grads"][k])
    assert list(final) == list(R.STATE_KEYS)
    for k in R.STATE_KEYS:
        bars.check(f"{tag}/wN/{k}", final[k])
    bars.done()


# ---- 2. the fused step against float64 ----------------------------------------------------------------------------------------------
def largest_batch(D, L):
    from gesture2vec_amd import ops
    B = 128
    while ops.vaeframe_plan(B + 1, D, L, True)[1]:
        B += 1
    assert ops.vaeframe_plan(B, D, L, True)[1] and not ops.vaeframe_plan(B + 1, D, L, True)[1]
    return B


STEP_SHAPES = [(2, 135, 40), (16, 135, 40), (17, 135, 45), (128, 135, 40), (37, 20, 8), "largest",
               (3, 7, 5)]      # the last: every dimension inside one partial tile, none a multiple of 4


@pytest.mark.parametrize("shape", STEP_SHAPES, ids=str)
def test_fused_step_against_float64(shape):
    from gesture2vec_amd import ops
    if shape == "largest":
        shape = (largest_batch(135, 40), 135, 40)
        assert shape[0] >= 128
    state, x, t, keep, eps = R.random_problem(shape, 1)
    res = R.step(R.f64(state), x.astype(np.float64), t.astype(np.float64), keep.astype(np.float64), eps.astype(np.float64))
    T = {k: v.to(DEV) for k, v in tensors(state).items()}
    order = ("encoder.0", "VAE_fc_mean", "VAE_fc_std", "VAE_fc_decoder", "decoder.0")
    names = [f"{m}.{p}" for m in order for p in ("weight", "bias")]
    grads = [torch.full_like(T[k], float("nan")) for k in names]

    def call():
        S = {k: v.clone() for k, v in T.items()}
        out = ops.vaeframe_step(dev(x), dev(t), dev(keep), 2.0, [S[k] for k in names], 12.5, grads, eps=dev(eps), want_latent=True,
                                want_stats=True, want_out=True)
        torch.cuda.synchronize()
        return S, out, [g.clone() for g in grads]

    S, o, g1 = call()
    bars = Bars(None)
    sc = o["scalars"].cpu().numpy()
    for name, got, ref in (("mse", sc[0], res["mse"]), ("kl", sc[1], res["kl"]), ("loss", sc[2], res["loss"])):
        bars.whole(name, got, ref, STEP_TOL)
    for k in R.FORWARD:
        bars.whole(k, o[k].cpu().numpy(), res[k], STEP_TOL)
    for k, g in zip(names, g1):
        assert bool(torch.isfinite(g).all()), k           # the NaN fill is fully overwritten
        bars.whole("grad " + k, g.cpu().numpy(), res["grads"][k], STEP_TOL)
    for k in names:
        assert torch.equal(S[k], T[k]), k                 # the step moves no weight
    bars.done()
    S2, o2, g2 = call()                                   # the same input gives the same bits
    assert all(torch.equal(o[k], o2[k]) for k in ("scalars", "latent", "mean", "logvar", "out"))
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))


# ---- 3. the operator kernels against float64 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 255, 256, 257, 4097])
def test_operator_kernels_against_float64(n):
    from gesture2vec_amd import ops
    rng = np.random.default_rng(n)
    L = next(w for w in (3, 17, 257, 2, 1) if n % w == 0)      # (1, 1), (1, 3), (85, 3), (128, 2), (1, 257), (241, 17): L % 4 != 0
    shape = (n // L, L)
    assert shape[0] * shape[1] == n and shape[1] % 4 != 0
    mean, logvar, eps, dz, gm, gl, y = (rng.standard_normal(shape).astype(np.float32) for _ in range(7))
    y = np.tanh(y)
    gkl = np.float32(0.7)
    m64, l64, e64, d64 = (a.astype(np.float64) for a in (mean, logvar, eps, dz))
    bars = Bars(None)
    z, used, kl = ops.reparam_fwd(dev(mean), dev(logvar), eps=dev(eps))
    bars.whole("z", z.cpu().numpy(), m64 + np.exp(l64 / 2) * e64, OP_TOL)
    bars.whole("kl", kl.cpu().numpy()[0], (np.exp(l64) - l64 - 1 + m64 ** 2).mean(), KL_TOL)
    assert torch.equal(used.cpu(), torch.from_numpy(eps))
    z0, used0, kl0 = ops.reparam_fwd(dev(mean), dev(logvar), sample=False)
    assert used0 is None and torch.equal(z0.cpu(), torch.from_numpy(mean)) and torch.equal(kl0, kl)      # z = mean bit for bit
    dm, dl = ops.reparam_bwd(dev(dz), dev(np.array([gkl])), dev(mean), dev(logvar), dev(eps), g_mean=dev(gm), g_logvar=dev(gl))
    c = float(gkl) / n
    bars.whole("dmean", dm.cpu().numpy(), d64 + 2 * c * m64 + gm, OP_TOL)
    bars.whole("dlogvar", dl.cpu().numpy(), d64 * 0.5 * np.exp(l64 / 2) * e64 + c * (np.exp(l64) - 1) + gl, OP_TOL)
    dm0, dl0 = ops.reparam_bwd(dev(dz), None, dev(mean), dev(logvar), None)                              # no kl gradient, no noise
    assert torch.equal(dm0.cpu(), torch.from_numpy(dz)) and not bool(dl0.any())
    bars.whole("tanh_bwd", ops.tanh_bwd(dev(dz), dev(y)).cpu().numpy(), d64 * (1 - y.astype(np.float64) ** 2), OP_TOL)
    bars.done()


def test_staged_gradients_at_the_genea_shape():
    from gesture2vec_amd import functional as Fn
    shape = (1024, 135, 200)
    state, x, t, keep, eps = R.random_problem(shape, 2)
    res = R.step(R.f64(state), x.astype(np.float64), t.astype(np.float64), keep.astype(np.float64), eps.astype(np.float64))
    net, _ = build(state, shape, "auto")
    assert net.resolve(1024, True) == "staged"
    net.set_dropout_mask(dev(keep)); net.set_latent_noise(dev(eps))
    out, logvar, mean = net(dev(x).unsqueeze(2))
    loss = Fn.mse_loss(out, dev(t).unsqueeze(2)) + 12.5 * net.last_kl[0]
    loss.backward()
    bars = Bars(None)
    bars.whole("loss", loss.item(), res["loss"], BIG_TOL)
    bars.whole("out", out.detach().squeeze(2).cpu().numpy(), res["out"], BIG_TOL)
    bars.whole("logvar", logvar.detach().cpu().numpy(), res["logvar"], BIG_TOL); bars.whole("mean", mean.detach().cpu().numpy(), res["mean"], BIG_TOL)
    for k in R.TRAINABLE:
        bars.whole("grad " + k, dict(net.named_parameters())[k].grad.cpu().numpy(), res["grads"][k], BIG_TOL)
    bars.done()


# ---- 4. the drawn noise ---------------------------------------------------------------------------------------------------------------
def drawn_by_step(shape, seed, counter):
    from gesture2vec_amd import ops
    state, x, t, keep, _ = R.random_problem(shape, 4)
    T = {k: v.to(DEV) for k, v in tensors(state).items()}
    order = ("encoder.0", "VAE_fc_mean", "VAE_fc_std", "VAE_fc_decoder", "decoder.0")
    names = [f"{m}.{p}" for m in order for p in ("weight", "bias")]
    grads = [torch.full_like(T[k], float("nan")) for k in names]
    o = ops.vaeframe_step(dev(x), dev(t), dev(keep), 2.0, [T[k] for k in names], 12.5, grads, seed=seed, offset_counter=counter,
                          want_stats=True)
    assert all(bool(torch.isfinite(g).all()) for g in grads)
    return o


def test_drawn_noise_is_one_stream_for_the_three_kernels():
    from gesture2vec_amd import ops
    B, L, seed = 16, 48, 11
    assert ops.vae_latent_ok(B, L)
    counters = [torch.full((1,), 5, dtype=torch.int64, device=DEV) for _ in range(3)]
    e_step = drawn_by_step((B, 135, L), seed, counters[0])["eps"]
    mean = torch.randn(B, L, device=DEV)
    e_op = ops.reparam_fwd(mean, torch.zeros_like(mean), seed=seed, offset_counter=counters[1])[1]
    w, b = torch.randn(L, L, device=DEV) / 7, torch.zeros(L, device=DEV)
    e_chunk = ops.vae_latent_fwd(torch.randn(1, B, L, device=DEV), w, b, w, b, seed=seed, offset_counter=counters[2], want_hf=False)["eps"]
    assert torch.equal(e_step, e_op) and torch.equal(e_step, e_chunk.view(B, L))
    assert [int(c) for c in counters] == [6, 6, 6]                                   # the counter advances by exactly 1
    again = drawn_by_step((B, 135, L), seed, counters[0])["eps"]
    assert int(counters[0]) == 7 and not torch.equal(again, e_step)                   # a second call draws different noise
    assert torch.equal(again, ops.reparam_fwd(mean, torch.zeros_like(mean), seed=seed, offset_counter=counters[1])[1])


def test_drawn_noise_is_standard_normal_and_fills_odd_shapes():
    from gesture2vec_amd import ops
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    e = drawn_by_step((128, 135, 40), 3, counter)["eps"].double().cpu().numpy().reshape(-1)
    n = e.size
    assert n == 5120 and abs(e.mean()) < 5 / np.sqrt(n) and abs(e.var() - 1) < 5 * np.sqrt(2 / n), (e.mean(), e.var())
    # B L = 765 is no multiple of 4: every element written (the buffer starts as NaN inside ops) and finite, the same as the operator's
    o = drawn_by_step((17, 135, 45), 3, counter)
    assert o["eps"].shape == (17, 45) and bool(torch.isfinite(o["eps"]).all()) and bool(torch.isfinite(o["logvar"]).all())
    counter2 = torch.ones(1, dtype=torch.int64, device=DEV)
    nan = torch.full((17, 45), float("nan"), device=DEV)
    assert torch.equal(o["eps"], ops.reparam_fwd(nan, nan, seed=3, offset_counter=counter2)[1])


# ---- 5. eval mode and the surface ---------------------------------------------------------------------------------------------------------
def test_eval_forward_surface_and_reference_checkpoint(fx, golden_dir):
    from gesture2vec_amd.model.DAE_model import VAE_Network
    net = VAE_Network(135, 40)
    assert {k: list(v.shape) for k, v in net.state_dict().items()} == json.loads(str(fx["e/state_dict"]))
    ckpt = torch.load(os.path.join(golden_dir, "vaeframe_ckpt.bin"), map_location="cpu", weights_only=False)
    net.load_state_dict(ckpt["gen_dict"], strict=True)
    net = net.to(DEV)
    net.train(False)
    case = R.load_case(fx, "a")
    x = case["data"][-1][0].to(DEV)
    bars = Bars(fx)
    with torch.no_grad():
        net.set_latent_noise(dev(fx["a/eval/eps"]))
        out, logvar, mean = net(x)                                                   # logvar first
        assert out.shape == (128, 135, 1) and logvar.shape == mean.shape == (128, 40)
        bars.check("a/eval/out", out.squeeze(2).cpu().numpy()); bars.check("a/eval/mean", mean.cpu().numpy())
        bars.check("a/eval/logvar", logvar.cpu().numpy())
        net.set_latent_noise(dev(fx["a/latent/eps"]))
        got = net(x, get_latent=True)
        assert len(got) == 2 and got[0].shape == (128, 135, 1) and got[1].shape == (128, 40) and not got[1].requires_grad
        bars.check("a/latent/out", got[0].squeeze(2).cpu().numpy()); bars.check("a/latent/latent", got[1].cpu().numpy())
        # the noise is added in eval mode too; sample=False is the forward with eps = 0, bit for bit
        net.set_latent_noise(None)
        a, b = net(x)[0], net(x)[0]
        assert not torch.equal(a, b)
        net.set_latent_noise(torch.zeros(128, 40, device=DEV))
        zero = net(x)[0]
        net.set_latent_noise(None)
        assert torch.equal(net.reconstruct(x, sample=False), zero) and net.reconstruct(x).shape == (128, 135, 1)
        assert not torch.equal(net.reconstruct(x), zero)
        # the row-wise pieces against float64
        s64 = R.f64({k: v.numpy() for k, v in ckpt["gen_dict"].items()})
        x64 = x.squeeze(2).double().cpu().numpy()
        f64 = R.infer(s64, x64, np.zeros((128, 40)))
        for rows in (x, x.squeeze(2), x[:1], x[:17].squeeze(2)):
            lat = net.encode(rows)
            bars.whole("encode", lat.cpu().numpy(), f64["latent"][:lat.shape[0]], ENC_TOL)
        assert torch.equal(net.encode(x)[:1], net.encode(x[:1]))
        c = torch.randn(33, 40, device=DEV)
        c64 = c.double().cpu().numpy()
        bars.whole("decode", net.decode(c).cpu().numpy(), c64 @ s64["decoder.0.weight"].T + s64["decoder.0.bias"], DEC_TOL)
        gen = (c64 @ s64["VAE_fc_decoder.weight"].T + s64["VAE_fc_decoder.bias"]) @ s64["decoder.0.weight"].T + s64["decoder.0.bias"]
        bars.whole("generate", net.generate(c).cpu().numpy(), gen, 2 * DEC_TOL)
    bars.done()


def test_rep_model_of_part_b_and_clip_helpers(fx, golden_dir):
    """a VAE_Network where the Part b dataset and the clip generators take a frame model: encode on any rows, decode back"""
    from gesture2vec_amd.model.DAE_model import DAE_Network, VAE_Network
    net = VAE_Network(135, 40).to(DEV)
    net.train(False)
    dae = DAE_Network(135, 40).to(DEV)
    clips = torch.randn(3, 34, 135, device=DEV)
    with torch.no_grad():
        lat = net.encode(clips.reshape(-1, 135)).view(3, 34, 40)
        back = net.decode(lat.reshape(-1, 40)).view(3, 34, 135)
        assert lat.shape == dae.encode(clips.reshape(-1, 135)).view(3, 34, 40).shape and back.shape == clips.shape
        assert bool(torch.isfinite(back).all()) and float(lat.abs().max()) <= 1.0
        from gesture2vec_amd.generate import finish_clips
        done = finish_clips(net, lat, None, None, n_poses=34)
        plain = finish_clips(None, back, None, None, n_poses=34)
        assert done.shape == (3, 34, 135) and torch.equal(done, plain)        # finish_clips decodes through dae.decode


# ---- 6. refusals on the device --------------------------------------------------------------------------------------------------------------
def test_routes_and_refusals_on_the_device():
    from gesture2vec_amd.train_eval.train_seq2seq import train_iter_DAE
    net, optim = build(R.random_state(135, 40, 0), (16, 135, 40), "fused")
    x = torch.randn(16, 135, 1, device=DEV)
    with pytest.raises(RuntimeError, match="fused_step"):
        net(x)
    with pytest.raises(ValueError, match="B >= 2"):
        train_iter_DAE(ARGS, 1, x[:1], x[:1], net, optim)
    assert np.isfinite(train_iter_DAE(ARGS, 1, x, x, net, optim)["loss"])
    big, opt2 = build(R.random_state(135, 200, 0), (1024, 135, 200), "fused")
    xb = torch.randn(1024, 135, 1, device=DEV)
    with pytest.raises(ValueError, match="LDS"):
        train_iter_DAE(ARGS, 1, xb, xb, big, opt2)
    big.route = "auto"                                  # the plan lets it fall to the staged route
    before = big.decoder[0].weight.detach().clone()
    assert np.isfinite(train_iter_DAE(ARGS, 1, xb, xb, big, opt2)["loss"]) and not torch.equal(before, big.decoder[0].weight)
    with pytest.raises(NotImplementedError, match="VAE_Network"):
        train_iter_DAE(argparse.Namespace(autoencoder_vq="True", autoencoder_vae="True"), 1, x, x, net, optim)


# ---- 7. the trainer -------------------------------------------------------------------------------------------------------------------------
def test_train_dae_script_vae_branch(tmp_path):
    """scripts/train_DAE.py --config=config/DAE_VAE_synthetic.yml --synthetic: a few batches an epoch, the checkpoint, the loader"""
    out = os.path.join(tmp_path, "run_dae_vae")
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "train_DAE.py"), "--config", os.path.join(ROOT, "config", "DAE_VAE_synthetic.yml"),
           "--synthetic", "--synthetic_batches", "3", "--epochs", "20", "--model_save_path", out, "--name", "t"]
    r = subprocess.run(cmd, cwd=os.path.join(ROOT, "scripts"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    path = os.path.join(out, "t_H40_checkpoint_020.bin")
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    assert set(ckpt) == {"args", "epoch", "lang_model", "pose_dim", "gen_dict"} and list(ckpt["gen_dict"]) == list(R.STATE_KEYS)
    assert all(bool(torch.isfinite(v).all()) for v in ckpt["gen_dict"].values())
    with open(os.path.join(out, "train_DAE.log")) as f:
        log = f.read()
    import re
    losses = [float(v) for v in re.findall(r"loss: ([-+.\w]+)", log)]
    assert len(losses) >= 20 and np.isfinite(losses).all(), losses[:5]
    assert not os.path.exists(os.path.join(out, "plots"))                # the curves are the VQ mode's
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import utils.train_utils
    from gesture2vec_amd.model.DAE_model import VAE_Network
    loaded = utils.train_utils.load_checkpoint_and_model(path, DEV, "DAE")
    gen = [v for v in loaded if isinstance(v, VAE_Network)]
    assert len(gen) == 1 and all(torch.equal(v.cpu(), ckpt["gen_dict"][k]) for k, v in gen[0].state_dict().items())
