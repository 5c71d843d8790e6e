"""CPU-only checks of the frame-level variational autoencoder (VAE_Network): the float64 restatement (tests/_vaeframe_ref.py) against
the recorded golden (tests/golden/vaeframe.npz) within the stored bars and against central differences, g2v_vaeframe_plan's answers,
the exports, init_model's dispatch and the refusals by name."""
import argparse
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _vaeframe_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "vaeframe.npz"))


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_golden_is_within_its_bars_of_the_restatement(fx, tag):
    case = R.load_case(fx, tag)
    res, final = R.restate_case(case)
    worst = []

    def check(name, value):
        d, bar = R.distance(R.stored(fx, name), R.pack(value)), float(fx["bar/" + name])
        if not d <= bar:
            worst.append((name, d, bar))

    for i, r in enumerate(res, 1):
        s = f"{tag}/s{i}/"
        check(s + "loss", r["loss"])
        for k in R.FORWARD:
            check(s + k, r[k])
        if i == 1:
            for k in R.TRAINABLE:
                check(s + "grad/" + k, r["grads"][k])
    for k in R.STATE_KEYS:
        check(f"{tag}/wN/{k}", final[k])
    if tag == "a":
        x = case["data"][-1][0].squeeze(2).numpy().astype(np.float64)
        e = R.infer(final, x, fx["a/eval/eps"].astype(np.float64))
        for k in ("out", "mean", "logvar"):
            check("a/eval/" + k, e[k])
        e = R.infer(final, x, fx["a/latent/eps"].astype(np.float64))
        check("a/latent/out", e["out"]); check("a/latent/latent", e["latent"])
    assert not worst, worst
    assert all(float(fx[k]) >= 1e-6 for k in fx.files if k.startswith("bar/"))
    # the recorded loss is the total: mse + 12.5 kl, and the noise is standard normal, one array per forward
    assert abs(res[0]["loss"] - (res[0]["mse"] + 12.5 * res[0]["kl"])) < 1e-12
    assert fx[f"{tag}/s1/eps"].shape == (case["shape"][0], case["shape"][2])


@pytest.mark.parametrize("shape", [(5, 7, 3), (9, 6, 4)])
def test_restated_gradients_are_central_differences(shape):
    B, D, L = shape
    state, x, t, keep, eps = R.random_problem(shape, 3)
    state = R.f64(state)
    x, t, keep, eps = (np.asarray(a, np.float64) for a in (x, t, keep, eps))
    res = R.step(state, x, t, keep, eps)
    rng = np.random.default_rng(0)
    for k in R.TRAINABLE:
        flat = state[k].reshape(-1)
        for idx in rng.choice(flat.size, size=min(flat.size, 6), replace=False):
            old, h = flat[idx], 1e-6
            flat[idx] = old + h
            up = R.step(state, x, t, keep, eps)["loss"]
            flat[idx] = old - h
            down = R.step(state, x, t, keep, eps)["loss"]
            flat[idx] = old
            num, ana = (up - down) / (2 * h), res["grads"][k].reshape(-1)[idx]
            assert abs(num - ana) <= 1e-7 * max(1.0, abs(ana)), (k, idx, num, ana)
    # the reference's own expression of the loss (train_seq2seq.py:224-230)
    lv, mu = res["logvar"], res["mean"]
    assert abs(res["loss"] - (res["mse"] + 5 * (-2.5 * np.mean(np.mean(1 + lv - np.exp(lv) - mu ** 2, 1))))) < 1e-12


def test_plan_answers():
    from gesture2vec_amd import _lib, ops
    lib = _lib.load()
    for L in (8, 40, 45):
        for B in range(2, 129):
            route, fused_ok, why = ops.vaeframe_plan(B, 135, L, True)
            assert fused_ok and route in ("fused", "staged"), (B, L, why)
            assert lib.g2v_vaeframe_workspace(B, 135, L) >= 4 * B * 135
            assert 0 < lib.g2v_vaeframe_step_lds(B, 135, L) <= 160 * 1024
    # the LDS layout is the limit and nothing else: six (B, ld(L)) row arrays + 32 floats, ld(n) = n rounded up to 4 mod 8
    for L, ld in ((40, 44), (45, 52)):
        B = 128
        while ops.vaeframe_plan(B + 1, 135, L, True)[1]:
            B += 1
        floats = lambda b: 6 * b * ld + 32      # noqa: E731
        assert floats(B) * 4 <= 160 * 1024 < floats(B + 1) * 4 and lib.g2v_vaeframe_step_lds(B, 135, L) == floats(B) * 4
        assert lib.g2v_vaeframe_step_lds(B + 1, 135, L) == 0 and lib.g2v_vaeframe_workspace(B + 1, 135, L) == 0
        route, fused_ok, why = ops.vaeframe_plan(B + 1, 135, L, True)
        assert route == "staged" and not fused_ok and "LDS" in why
        assert ops.vaeframe_plan(B, 1000, L, True)[1]           # D does not enter the layout
    route, fused_ok, why = ops.vaeframe_plan(1024, 135, 200, True)
    assert route == "staged" and not fused_ok and "LDS" in why
    for B in (1, 0, -3):
        route, fused_ok, why = ops.vaeframe_plan(B, 135, 40, True)
        assert route == "" and not fused_ok and "refused" in why
    assert ops.vaeframe_plan(128, 135, 40, False)[:2] == ("staged", False)      # eval mode has no fused kernel
    # `auto` is never the fused step where the kernel does not admit the shape
    for B in (2, 16, 128, 155, 156, 200, 1024):
        for L in (40, 45, 200):
            route, fused_ok, _ = ops.vaeframe_plan(B, 135, L, True)
            assert route in ("fused", "staged") and (fused_ok or route != "fused")


def test_exports_state_dict_and_dispatch(fx):
    from gesture2vec_amd import functional as Fn, ops
    from gesture2vec_amd.model.DAE_model import DAE_Network, VAE_Network, VQ_Frame
    for name in ("vaeframe_plan", "vaeframe_step", "tanh_bwd", "reparam_fwd", "reparam_bwd"):
        assert callable(getattr(ops, name))
    assert callable(Fn.reparam) and issubclass(Fn.ReparamFn, torch.autograd.Function)
    net = VAE_Network(135, 40)
    want = json.loads(str(fx["e/state_dict"]))
    assert {k: list(v.shape) for k, v in net.state_dict().items()} == want and list(net.state_dict()) == list(want) == list(R.STATE_KEYS)
    assert (net.vae, net.dropout.p, net.route, net.rng_seed) == (True, 0.5, "auto", 0) and not list(net.buffers())
    assert [p is q for p, q in zip(net.trainable(), net.parameters())] == [True] * 10
    for name in ("set_dropout_mask", "set_latent_noise", "fused_step", "encode", "decode", "reconstruct", "generate", "resolve"):
        assert callable(getattr(net, name))
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import train_DAE
    from model.DAE_model import VAE_Network as shim
    assert shim is VAE_Network
    args = argparse.Namespace(autoencoder_vq="False", autoencoder_vae="True", input_motion_dim=135, hidden_size=40,
                              autoencoder_vq_components=80)
    assert type(train_DAE.init_model(args, None, 135, "cpu")[0]) is VAE_Network
    args.autoencoder_vae = "False"
    assert type(train_DAE.init_model(args, None, 135, "cpu")[0]) is DAE_Network
    args.autoencoder_vq = "True"
    assert type(train_DAE.init_model(args, None, 135, "cpu")[0]) is VQ_Frame
    args.autoencoder_vae = "True"
    with pytest.raises(NotImplementedError, match=r"VQ_Frame\(vae=True\)"):
        train_DAE.init_model(args, None, 135, "cpu")
    import yaml
    with open(os.path.join(ROOT, "config", "DAE_VAE_synthetic.yml")) as f, open(os.path.join(ROOT, "config", "DAE_VQ_synthetic.yml")) as g:
        a, b = yaml.safe_load(f), yaml.safe_load(g)
    assert (a["autoencoder_vq"], a["autoencoder_vae"]) == ("False", "True")
    assert {k for k in a if a[k] != b[k]} == {"name", "model_save_path", "autoencoder_vq", "autoencoder_vae"}


def test_refusals_by_name():
    from gesture2vec_amd.flat import FlatClipAdam  # noqa: F401
    from gesture2vec_amd.model.DAE_model import VAE_Network
    from gesture2vec_amd.train_eval.train_seq2seq import train_iter_DAE
    net = VAE_Network(135, 40)
    net.train(True)
    for mode in (True, False):
        net.train(mode)
        with pytest.raises(ValueError, match="at least 2 frames"):
            net(torch.zeros(1, 135, 1))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            net(torch.zeros(4, 135, 1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net.encode(torch.zeros(4, 135))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net.reconstruct(torch.zeros(4, 135, 1), sample=False)
    with pytest.raises(ValueError, match="B >= 2"):
        net.resolve(1, True)
    net.route = "fused"
    with pytest.raises(ValueError, match="LDS"):
        net.resolve(1024, True)
    net.route = "sideways"
    with pytest.raises(ValueError, match="route"):
        net.resolve(4, True)
    both = argparse.Namespace(autoencoder_vq="True", autoencoder_vae="True")
    with pytest.raises(TypeError, match="FlatClipAdam"):
        train_iter_DAE(both, 1, None, None, net, None)
