"""GPU parity of the frame-level quantised autoencoder (VQ_Frame, autoencoder_vq "True"): both routes against the reference's golden
vectors (tests/golden/vqframe.npz: every id equal, everything else within the stored bars), the fused step and the grid kernel
against the float64 restatement (tests/_vqframe_ref.py) at the shapes where their tiling can go wrong, determinism, and the trainer.

Where no recorded bar exists (the restatement is the yardstick) the bound is worked out from the number format:
  the longest chain of fp32 sums behind any compared quantity is y (a contraction of length D <= 135), BatchNorm's two batch sums
  (2 B), out (L <= 45), dz (D) and one weight gradient (B), B <= 353 at the largest admitted batch: 135 + 706 + 45 + 135 + 353 = 1374
  terms.  A sum of n terms in any order is off by at most n 2^-24 of its sum of |terms|, which stays within ~4 x the largest element
  of the result at these sizes and N(0, 1) inputs: 4 x 1374 x 2^-24 = 3.3e-4 -> 4e-4 of the largest element (STEP_TOL).  A real
  mistake is far above it: biased for unbiased variance is 0.8 % at B = 128, a dropped scale a factor of 2.
  The grid kernel's latent is ONE contraction of length 135 and the eval BatchNorm: 4 x 135 x 2^-24 = 3.2e-5 -> 4e-5; its output adds
  a contraction of length L <= 200 on top: 4 x 200 x 2^-24 + 3.2e-5 = 8e-5 -> 1e-4."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _vqframe_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = argparse.Namespace(autoencoder_vq="True", autoencoder_vae="False")
STEP_TOL, LATENT_TOL, OUT_TOL = 4e-4, 4e-5, 1e-4


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "vqframe.npz"))


def tensors(state):
    return {k: torch.from_numpy(np.array(v)) for k, v in state.items()}


def build(state, shape, route, lr):
    from gesture2vec_amd.flat import FlatClipAdam
    from gesture2vec_amd.model.DAE_model import VQ_Frame
    B, D, L, K = shape
    net = VQ_Frame(D, L, False, K)
    net.load_state_dict(tensors(state), strict=True)
    net = net.to(DEV)
    net.train(True)
    net.route = route
    return net, FlatClipAdam(net.parameters(), lr=lr, betas=(0.5, 0.999))


def observe(net, route, seen):
    """ids and latent of every training forward, without touching the product: a hook on the quantiser (staged), the step's own
    outputs (fused)"""
    if route == "staged":
        net.vq_layer.register_forward_hook(lambda m, i, o: seen.update(z=i[0].detach().clone(), ids=o[3].argmax(1)))
        return
    orig = net.fused_step

    def fused_step(x, target, grads, **kw):
        res = orig(x, target, grads, want_latent=True)
        seen.update(ids=res[1], z=res[2], fused_calls=seen.get("fused_calls", 0) + 1)
        return res
    net.fused_step = fused_step


_RUNS = {}


def run_case(fx, tag, route):
    """the recorded iterations of case `tag` on `route`, once per module -> (net, [per step dict], final state_dict on the CPU)"""
    from gesture2vec_amd.train_eval.train_seq2seq import train_iter_DAE
    if (tag, route) in _RUNS:
        return _RUNS[(tag, route)]
    case = R.load_case(fx, tag)
    net, optim = build(case["state0"], case["shape"], route, case["lr"])
    seen, steps = {}, []
    observe(net, route, seen)
    for i, ((noisy, original), mask) in enumerate(zip(case["data"], case["masks"]), 1):
        net.set_dropout_mask(torch.from_numpy(mask.copy()).to(DEV))
        loss, perplexity = train_iter_DAE(ARGS, 1, noisy.to(DEV), original.to(DEV), net, optim)
        assert isinstance(loss["loss"], float) and torch.is_tensor(perplexity)
        step = dict(loss=loss["loss"], perplexity=float(perplexity.detach()), ids=seen["ids"].cpu().numpy(), latent=seen["z"].cpu().numpy())
        if i == 1:
            step["grads"] = {k: dict(net.named_parameters())[k].grad.detach().cpu().numpy().copy() for k in R.TRAINABLE}
        steps.append(step)
    if route == "fused":
        assert seen["fused_calls"] == case["steps"]
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

    def done(self):
        assert not self.bad, self.bad


@pytest.mark.parametrize("route", ["staged", "fused"])
@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_iterations_match_the_reference_golden(fx, tag, route):
    net, steps, final, case = run_case(fx, tag, route)
    res64, _ = R.restate_case(case)
    bars = Bars(fx)
    for i, st in enumerate(steps, 1):
        s = f"{tag}/s{i}/"
        assert np.array_equal(st["ids"], fx[s + "ids"]), (s, int((st["ids"] != fx[s + "ids"]).sum()))      # every row
        bars.check(s + "loss", st["loss"]); bars.check(s + "perplexity", st["perplexity"]); bars.check(s + "latent", st["latent"])
        if i == 1:
            for k in R.TRAINABLE:
                if k == "encoder.0.bias":      # exactly zero but for rounding: the restatement's bound for an fp32 sum, no relative bar
                    print(s + "grad/" + k, float(np.abs(st["grads"][k]).max()), float(res64[0]["dbe_bound"].min()))
                    assert np.all(np.abs(st["grads"][k]) <= res64[0]["dbe_bound"])
                else:
                    bars.check(s + "grad/" + k, st["grads"][k])
    assert list(final) == list(R.STATE_KEYS)
    for k in R.STATE_KEYS:
        if k == "bachnorm.num_batches_tracked":
            assert int(final[k]) == case["steps"] == int(fx[f"{tag}/wN/{k}"])
        else:
            bars.check(f"{tag}/wN/{k}", final[k])
    if tag == "a":
        net.train(False)
        with torch.no_grad():
            out, latent, enc = net(case["data"][-1][0].to(DEV), Inference=True)
        net.train(True)
        assert out.shape == (128, 135, 1) and enc.shape == (128, 80) and bool((enc.sum(1) == 1).all())
        assert np.array_equal(enc.argmax(1).cpu().numpy(), fx["a/eval/ids"])
        bars.check("a/eval/out", out.squeeze(2).cpu().numpy()); bars.check("a/eval/latent", latent.cpu().numpy())
    bars.done()


def test_fused_against_staged_on_the_same_masks(fx):
    _, fused, f_final, _ = run_case(fx, "a", "fused")
    _, staged, s_final, _ = run_case(fx, "a", "staged")
    bars = Bars(fx)
    for i, (f, s) in enumerate(zip(fused, staged), 1):
        t = f"a/s{i}/"
        assert np.array_equal(f["ids"], s["ids"])
        for k in ("loss", "perplexity", "latent"):
            bars.check(t + k, f[k], ref=R.pack(s[k]))
        if i == 1:
            for k in R.TRAINABLE:
                if k != "encoder.0.bias":
                    bars.check(t + "grad/" + k, f["grads"][k], ref=R.pack(s["grads"][k]))
    for k in R.STATE_KEYS:
        if k != "bachnorm.num_batches_tracked":
            bars.check("a/wN/" + k, f_final[k], ref=R.pack(s_final[k]))
    bars.done()


def test_state_dict_and_reference_checkpoint_round_trip(fx, golden_dir, tmp_path):
    from gesture2vec_amd.model.DAE_model import VQ_Frame
    net = VQ_Frame(135, 40, False, 80)
    assert {k: list(v.shape) for k, v in net.state_dict().items()} == json.loads(str(fx["e/state_dict"]))       # case e
    ckpt = torch.load(os.path.join(golden_dir, "vqframe_ckpt.bin"), map_location="cpu", weights_only=False)
    net.load_state_dict(ckpt["gen_dict"], strict=True)
    net = net.to(DEV)
    net.train(False)
    case = R.load_case(fx, "a")
    x = case["data"][-1][0].to(DEV)
    with torch.no_grad():
        out, latent, enc = net(x, Inference=True)
    assert np.array_equal(enc.argmax(1).cpu().numpy(), fx["a/eval/ids"])
    assert np.array_equal(net.codes(x).cpu().numpy(), fx["a/eval/ids"])
    bars = Bars(fx)
    bars.check("a/eval/out", out.squeeze(2).cpu().numpy()); bars.check("a/eval/latent", latent.cpu().numpy())
    bars.check("a/eval/latent", net.encode(x).cpu().numpy())
    bars.done()
    path = os.path.join(tmp_path, "ckpt.bin")
    torch.save({"gen_dict": net.state_dict()}, path)
    back = torch.load(path, map_location="cpu", weights_only=False)["gen_dict"]
    assert list(back) == list(ckpt["gen_dict"]) and all(torch.equal(back[k], ckpt["gen_dict"][k]) for k in back)


def random_state(shape, seed):
    B, D, L, K = shape
    rng = np.random.default_rng(seed)
    f = lambda a: np.asarray(a, np.float32)      # noqa: E731
    state = {"encoder.0.weight": f(rng.standard_normal((L, D)) / np.sqrt(D)), "encoder.0.bias": f(0.1 * rng.standard_normal(L)),
             "bachnorm.weight": f(1 + 0.1 * rng.standard_normal(L)), "bachnorm.bias": f(0.1 * rng.standard_normal(L)),
             "bachnorm.running_mean": f(0.1 * rng.standard_normal(L)), "bachnorm.running_var": f(1 + 0.2 * rng.random(L)),
             "bachnorm.num_batches_tracked": np.int64(0), "vq_layer._ema_w": f(rng.standard_normal((K, L))),
             "vq_layer._ema_cluster_size": f(np.zeros(K)), "vq_layer.pre_linear.weight": f(rng.standard_normal((L, L))),
             "vq_layer.pre_linear.bias": f(rng.standard_normal(L)), "vq_layer._embedding.weight": f(rng.standard_normal((K, L))),
             "decoder.0.weight": f(rng.standard_normal((D, L)) / np.sqrt(L)), "decoder.0.bias": f(0.1 * rng.standard_normal(D))}
    return {k: state[k] for k in R.STATE_KEYS}


def decided_problem(shape):
    """(state, x, t, keep, float64 result, float64 state after) with every row decided: seeds are searched, on the CPU"""
    B, D, L, K = shape
    for seed in range(50):
        state = R.warm_quantiser(random_state(shape, seed), B, seed)
        rng = np.random.default_rng(100 + seed)
        x, t = rng.standard_normal((B, D)).astype(np.float32), rng.standard_normal((B, D)).astype(np.float32)
        keep = (rng.random((B, D)) < 0.5).astype(np.uint8)
        res, new = R.step(R.f64(state), x.astype(np.float64), t.astype(np.float64), keep.astype(np.float64))
        if np.all(res["margin"] >= res["bound"]):
            return state, x, t, keep, res, new
    raise AssertionError(f"no seed below 50 leaves every row of {shape} decided")


def largest_batch(D, L, K):
    from gesture2vec_amd import ops
    B = 2
    while ops.vqframe_plan(2 * B, D, L, K, True)[1]:
        B *= 2
    step = B // 2
    while step:
        if ops.vqframe_plan(B + step, D, L, K, True)[1]:
            B += step
        step //= 2
    assert ops.vqframe_plan(B, D, L, K, True)[1] and not ops.vqframe_plan(B + 1, D, L, K, True)[1]
    return B


STEP_SHAPES = [(2, 135, 40, 80), (16, 135, 40, 80), (100, 135, 45, 100), (128, 135, 40, 1), (128, 135, 40, 128), "largest",
               (37, 20, 8, 5), (3, 7, 5, 3)]      # the last: every dimension inside one partial tile, none a multiple of 4


@pytest.mark.parametrize("shape", STEP_SHAPES, ids=str)
def test_fused_step_against_float64(shape):
    from gesture2vec_amd import ops
    if shape == "largest":
        shape = (largest_batch(135, 40, 80), 135, 40, 80)
        assert shape[0] >= 256
    state, x, t, keep, res, new = decided_problem(shape)
    T = {k: v.to(DEV) for k, v in tensors(state).items()}
    grads = [torch.full_like(T[k], float("nan")) for k in R.TRAINABLE]

    def call():
        S = {k: v.clone() for k, v in T.items()}
        out = ops.vqframe_step(torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV), torch.from_numpy(keep).to(DEV), 2.0,
                               S["encoder.0.weight"], S["encoder.0.bias"], S["bachnorm.weight"], S["bachnorm.bias"],
                               S["bachnorm.running_mean"], S["bachnorm.running_var"], 0.1, S["decoder.0.weight"], S["decoder.0.bias"],
                               S["vq_layer._embedding.weight"], S["vq_layer._ema_w"], S["vq_layer._ema_cluster_size"], 0.25, 0.99,
                               1e-5, grads, want_latent=True, want_out=True)
        torch.cuda.synchronize()
        return S, out, [g.clone() for g in grads]

    S, (scalars, ids, latent, out), g1 = call()
    assert np.array_equal(ids.cpu().numpy(), res["ids"])
    bars = Bars(None)
    sc = scalars.cpu().numpy()
    for name, got, ref in (("rec", sc[0], res["rec"]), ("loss_vq", sc[1], res["loss_vq"]), ("perplexity", sc[2], res["perplexity"]),
                           ("latent", latent.cpu().numpy(), res["latent"]), ("out", out.cpu().numpy(), res["out"])):
        bars.check(name, {"": np.asarray(got)}, ref={"": np.asarray(ref)}, bar=STEP_TOL)
    for k, g in zip(R.TRAINABLE, g1):
        if k == "encoder.0.bias":
            assert np.all(np.abs(g.cpu().numpy()) <= res["dbe_bound"]), (np.abs(g.cpu().numpy()).max(), res["dbe_bound"].min())
        else:
            bars.check("grad " + k, {"": g.cpu().numpy()}, ref={"": res["grads"][k]}, bar=STEP_TOL)
    for k in ("bachnorm.running_mean", "bachnorm.running_var", "vq_layer._ema_w", "vq_layer._ema_cluster_size",
              "vq_layer._embedding.weight"):
        bars.check(k, {"": S[k].cpu().numpy()}, ref={"": new[k]}, bar=STEP_TOL)
    for k in R.TRAINABLE + ("vq_layer.pre_linear.weight", "vq_layer.pre_linear.bias"):
        assert torch.equal(S[k], T[k]), k      # the step moves no trainable tensor and never touches pre_linear
    bars.done()
    # the same input gives the same bits
    S2, (scalars2, ids2, latent2, out2), g2 = call()
    assert torch.equal(scalars, scalars2) and torch.equal(ids, ids2) and torch.equal(latent, latent2) and torch.equal(out, out2)
    assert all(torch.equal(a, b) for a, b in zip(g1, g2)) and all(torch.equal(S[k], S2[k]) for k in S)


_INFER = {}


def infer_problem(D, L, K):
    """state, 1000 decided rows and the float64 forward, once per shape"""
    if (D, L, K) not in _INFER:
        for seed in range(50):
            state = random_state((2, D, L, K), seed)
            x = np.random.default_rng(200 + seed).standard_normal((1000, D)).astype(np.float32)
            e = R.infer(R.f64(state), x.astype(np.float64))
            if np.all(e["margin"] >= e["bound"]):
                break
        else:
            raise AssertionError("no seed below 50 leaves all 1000 rows decided")
        from gesture2vec_amd.model.DAE_model import VQ_Frame
        net = VQ_Frame(D, L, False, K)
        net.load_state_dict(tensors(state), strict=True)
        net = net.to(DEV)
        net.train(False)
        net.route = "fused"
        xd = torch.from_numpy(x).to(DEV)
        with torch.no_grad():
            out, latent, enc = net(xd.unsqueeze(2), Inference=True)
        _INFER[(D, L, K)] = (net, xd, e, out.squeeze(2), latent, enc.argmax(1))
    return _INFER[(D, L, K)]


@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("dims", [(135, 40, 80), (135, 200, 100)], ids=str)
def test_grid_kernel_against_float64(dims, N):
    from gesture2vec_amd import ops
    net, xd, e, out_all, latent_all, ids_all = infer_problem(*dims)
    d = net.decoder[0]
    ids, latent, out = ops.vqframe_infer(xd[:N].contiguous(), *net._infer_args(), w_dec=d.weight.data, b_dec=d.bias.data,
                                         want_latent=True, want_out=True)
    assert ids.dtype == torch.int64 and np.array_equal(ids.cpu().numpy(), e["ids"][:N])
    bars = Bars(None)
    bars.check("latent", {"": latent.cpu().numpy()}, ref={"": e["latent"][:N]}, bar=LATENT_TOL)
    bars.check("out", {"": out.cpu().numpy()}, ref={"": e["out"][:N]}, bar=OUT_TOL)
    bars.done()
    # a frame's bits do not depend on what else is in the call
    assert torch.equal(ids, ids_all[:N]) and torch.equal(latent, latent_all[:N]) and torch.equal(out, out_all[:N])
    assert torch.equal(net.codes(xd[:N]), ids) and torch.equal(net.encode(xd[:N].unsqueeze(2)), latent)
    if N == 1000:       # the staged route decides the same ids
        net.route = "staged"
        assert torch.equal(net.codes(xd), ids)
        net.route = "fused"


def test_skip_vq_on_the_staged_route():
    from gesture2vec_amd import functional as Fn
    shape = (37, 20, 8, 5)
    state, x, t, keep, _, _ = decided_problem(shape)
    res, _ = R.step(R.f64(state), x.astype(np.float64), t.astype(np.float64), keep.astype(np.float64), skip_vq=True)
    net, _ = build(state, shape, "auto", 5e-4)
    net.skip_vq = True
    net.set_dropout_mask(torch.from_numpy(keep).to(DEV))
    out, loss_vq, perplexity = net(torch.from_numpy(x).to(DEV).unsqueeze(2))
    assert float(loss_vq) == 0 and float(perplexity) == 0 and out.shape == (37, 20, 1)
    (Fn.mse_loss(out, torch.from_numpy(t).to(DEV).unsqueeze(2)) + loss_vq).backward()
    bars = Bars(None)
    bars.check("out", {"": out.detach().squeeze(2).cpu().numpy()}, ref={"": res["out"]}, bar=STEP_TOL)
    for k in R.TRAINABLE:
        if k != "encoder.0.bias":
            bars.check("grad " + k, {"": dict(net.named_parameters())[k].grad.cpu().numpy()}, ref={"": res["grads"][k]}, bar=STEP_TOL)
    bars.done()
    assert torch.equal(net.vq_layer._embedding.weight.cpu(), torch.from_numpy(state["vq_layer._embedding.weight"]))


def test_routes_and_refusals_on_the_device():
    from gesture2vec_amd.train_eval.train_seq2seq import train_iter_DAE
    shape = (16, 135, 40, 80)
    state = random_state(shape, 0)
    net, optim = build(state, shape, "fused", 5e-4)
    x = torch.randn(16, 135, 1, device=DEV)
    with pytest.raises(RuntimeError, match="fused_step"):
        net(x)
    with pytest.raises(ValueError, match="B >= 2"):
        train_iter_DAE(ARGS, 1, x[:1], x[:1], net, optim)
    big, opt2 = build(random_state((1024, 135, 200, 100), 0), (1024, 135, 200, 100), "fused", 5e-4)
    xb = torch.randn(1024, 135, 1, device=DEV)
    with pytest.raises(ValueError, match="LDS"):
        train_iter_DAE(ARGS, 1, xb, xb, big, opt2)
    big.route = "auto"                                  # the plan lets it fall to the staged route
    loss, perplexity = train_iter_DAE(ARGS, 1, xb, xb, big, opt2)
    assert np.isfinite(loss["loss"]) and 1.0 <= float(perplexity) <= 100.0
    with pytest.raises(NotImplementedError, match="VAE_Network"):
        train_iter_DAE(argparse.Namespace(autoencoder_vq="True", autoencoder_vae="True"), 1, x, x, net, optim)


def test_train_dae_script_vq_branch(tmp_path):
    """scripts/train_DAE.py --config=config/DAE_VQ_synthetic.yml --synthetic: a few batches an epoch, the checkpoint and the curves"""
    out = os.path.join(tmp_path, "run_dae_vq")
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "train_DAE.py"), "--config", os.path.join(ROOT, "config", "DAE_VQ_synthetic.yml"),
           "--synthetic", "--synthetic_batches", "3", "--epochs", "20", "--model_save_path", out, "--name", "t"]
    r = subprocess.run(cmd, cwd=os.path.join(ROOT, "scripts"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    ckpt = torch.load(os.path.join(out, "t_H40_checkpoint_020.bin"), map_location="cpu", weights_only=False)
    assert set(ckpt) == {"args", "epoch", "lang_model", "pose_dim", "gen_dict"} and list(ckpt["gen_dict"]) == list(R.STATE_KEYS)
    assert int(ckpt["gen_dict"]["bachnorm.num_batches_tracked"]) == 2 * 3 * 19      # two training forwards per batch
    curves = np.load(os.path.join(out, "plots", "Error_Epoch(20).npz"))
    assert curves["recon_error"].shape == curves["perplexity"].shape == (3 * 19,)
    assert np.isfinite(curves["recon_error"]).all() and (curves["perplexity"] >= 1.0 - 1e-6).all()
    assert np.load(os.path.join(out, "plots", "Error_Epoch(1).npz"))["perplexity"].shape == (0,)
