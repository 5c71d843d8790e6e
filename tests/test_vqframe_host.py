"""CPU-only checks of the frame-level quantised autoencoder (VQ_Frame): the float64 restatement (tests/_vqframe_ref.py) against a
literal torch float64 form, against the recorded golden (tests/golden/vqframe.npz) within the stored bars, g2v_vqframe_plan's
answers, and the refusals by name."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _vqframe_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "vqframe.npz"))


def literal_torch(state, x, t, keep):
    """nn.Linear, nn.BatchNorm1d and the quantiser written out as the reference writes it, in float64, under autograd"""
    D, L = state["encoder.0.weight"].shape[1], state["encoder.0.weight"].shape[0]
    K = state["vq_layer._embedding.weight"].shape[0]
    enc, bn, dec = torch.nn.Linear(D, L).double(), torch.nn.BatchNorm1d(L).double(), torch.nn.Linear(L, D).double()
    T = {k: torch.tensor(np.asarray(v, np.float64)) for k, v in state.items()}
    with torch.no_grad():
        enc.weight.copy_(T["encoder.0.weight"]); enc.bias.copy_(T["encoder.0.bias"])
        bn.weight.copy_(T["bachnorm.weight"]); bn.bias.copy_(T["bachnorm.bias"])
        bn.running_mean.copy_(T["bachnorm.running_mean"]); bn.running_var.copy_(T["bachnorm.running_var"])
        dec.weight.copy_(T["decoder.0.weight"]); dec.bias.copy_(T["decoder.0.bias"])
    E, ema_w, cs = T["vq_layer._embedding.weight"], T["vq_layer._ema_w"], T["vq_layer._ema_cluster_size"]
    x, t = torch.tensor(x), torch.tensor(t)
    z = bn(enc(x * torch.tensor(keep) / 0.5))
    dist = torch.sum(z ** 2, dim=1, keepdim=True) + torch.sum(E ** 2, dim=1) - 2 * torch.matmul(z, E.t())
    ids = torch.argmin(dist, dim=1)
    enc1h = torch.zeros(x.shape[0], K, dtype=torch.float64)
    enc1h.scatter_(1, ids.unsqueeze(1), 1)
    q = torch.matmul(enc1h, E)
    cs = cs * 0.99 + (1 - 0.99) * enc1h.sum(0)
    n = cs.sum()
    cs = (cs + 1e-5) / (n + K * 1e-5) * n
    ema_w = ema_w * 0.99 + (1 - 0.99) * torch.matmul(enc1h.t(), z.detach())
    loss_vq = 0.25 * torch.nn.functional.mse_loss(q.detach(), z)
    qs = z + (q - z).detach()
    pr = enc1h.mean(0)
    perplexity = torch.exp(-torch.sum(pr * torch.log(pr + 1e-10)))
    out = dec(qs)
    rec = torch.nn.functional.mse_loss(out, t)
    (rec + loss_vq).backward()
    grads = {"encoder.0.weight": enc.weight.grad, "encoder.0.bias": enc.bias.grad, "bachnorm.weight": bn.weight.grad,
             "bachnorm.bias": bn.bias.grad, "decoder.0.weight": dec.weight.grad, "decoder.0.bias": dec.bias.grad}
    return dict(rec=rec, loss_vq=loss_vq, perplexity=perplexity, ids=ids, latent=z, out=out, grads=grads,
                state={"bachnorm.running_mean": bn.running_mean, "bachnorm.running_var": bn.running_var,
                       "vq_layer._ema_cluster_size": cs, "vq_layer._ema_w": ema_w, "vq_layer._embedding.weight": ema_w / cs.unsqueeze(1)})


@pytest.mark.parametrize("shape", [(37, 20, 8, 5), (16, 33, 12, 9), (2, 7, 3, 1)])
def test_restatement_is_the_literal_torch_form(shape):
    B, D, L, K = shape
    rng = np.random.default_rng(5)
    state = {"encoder.0.weight": rng.standard_normal((L, D)) / np.sqrt(D), "encoder.0.bias": 0.1 * rng.standard_normal(L),
             "bachnorm.weight": 1 + 0.1 * rng.standard_normal(L), "bachnorm.bias": 0.1 * rng.standard_normal(L),
             "bachnorm.running_mean": 0.1 * rng.standard_normal(L), "bachnorm.running_var": 1 + 0.1 * rng.random(L),
             "bachnorm.num_batches_tracked": np.float64(3), "vq_layer._embedding.weight": rng.standard_normal((K, L)),
             "vq_layer._ema_w": rng.standard_normal((K, L)), "vq_layer._ema_cluster_size": rng.random(K) + 0.5,
             "decoder.0.weight": rng.standard_normal((D, L)) / np.sqrt(L), "decoder.0.bias": 0.1 * rng.standard_normal(D)}
    x, t = rng.standard_normal((B, D)), rng.standard_normal((B, D))
    keep = (rng.random((B, D)) < 0.5).astype(np.float64)
    res, new = R.step(R.f64(state), x, t, keep)
    lit = literal_torch(state, x, t, keep)

    def close(a, b, what):
        a, b = np.asarray(a, np.float64), b.detach().numpy()
        assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max()), what

    assert np.array_equal(res["ids"], lit["ids"].numpy())
    for k in ("rec", "loss_vq", "perplexity", "latent", "out"):
        close(res[k], lit[k], k)
    for k in R.TRAINABLE:
        close(res["grads"][k], lit["grads"][k], "grad " + k)
    for k, v in lit["state"].items():
        close(new[k], v, k)
    assert new["bachnorm.num_batches_tracked"] == 4
    assert np.all(np.abs(res["grads"]["encoder.0.bias"]) <= res["dbe_bound"])      # exactly zero but for rounding


@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
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
        assert np.array_equal(fx[s + "ids"], r["ids"]), s
        assert np.all(r["margin"] >= r["bound"]) and np.allclose(fx[s + "margin"], r["margin"], rtol=1e-9, atol=1e-12), s
        check(s + "loss", r["rec"]); check(s + "perplexity", r["perplexity"]); check(s + "latent", r["latent"])
        if i == 1:
            for k in R.TRAINABLE:
                if k == "encoder.0.bias":
                    assert np.all(np.abs(fx[s + "grad/" + k]) <= r["dbe_bound"])
                else:
                    check(s + "grad/" + k, r["grads"][k])
    for k in R.STATE_KEYS:
        if k == "bachnorm.num_batches_tracked":
            assert int(fx[f"{tag}/wN/{k}"]) == case["steps"] == int(final[k])
        else:
            check(f"{tag}/wN/{k}", final[k])
    if tag == "a":
        e = R.infer(final, case["data"][-1][0].squeeze(2).numpy().astype(np.float64))
        assert np.array_equal(fx["a/eval/ids"], e["ids"]) and np.all(e["margin"] >= e["bound"])
        check("a/eval/out", e["out"]); check("a/eval/latent", e["latent"])
    assert not worst, worst
    assert all(float(fx[k]) >= 1e-6 for k in fx.files if k.startswith("bar/"))


def test_second_step_of_a_fresh_model_collapses(fx):
    """the reference's behaviour, reproduced: after the first update an unused code is ~1e5 away, the batch falls onto one code"""
    assert float(fx["c/s1/perplexity"]) > 2.0 and float(fx["c/s2/perplexity"]) == 1.0
    assert float(fx["c/s2/loss"]) > 10 * float(fx["c/s1/loss"])


def test_plan_answers():
    from gesture2vec_amd import _lib, ops
    lib = _lib.load()
    for L in (40, 45):
        for K in (1, 80, 128):
            for B in (2, 16, 100, 128, 256):
                route, fused_ok, why = ops.vqframe_plan(B, 135, L, K, True)
                assert fused_ok and route in ("fused", "staged"), (B, L, K, why)
                assert lib.g2v_vqframe_workspace(B, 135, L, K, 1) >= 4 * B * 135
                assert 0 < lib.g2v_vqframe_step_lds(B, 135, L, K) <= 160 * 1024
    # the LDS layout is the limit: 2 B ld(L) + D ld(L) + K ld(L) + L + 2 K + 48 + B / 2 floats, ld(n) = n rounded up to 4 mod 8
    B = 256
    while ops.vqframe_plan(B + 1, 135, 45, 128, True)[1]:
        B += 1
    floats = lambda b: 2 * b * 52 + 135 * 52 + 128 * 52 + 45 + 2 * 128 + 48 + (b + 1) // 2      # noqa: E731
    assert floats(B) * 4 <= 160 * 1024 < floats(B + 1) * 4 and lib.g2v_vqframe_step_lds(B, 135, 45, 128) == floats(B) * 4
    assert lib.g2v_vqframe_step_lds(B + 1, 135, 45, 128) == 0 and lib.g2v_vqframe_workspace(B + 1, 135, 45, 128, 1) == 0
    route, fused_ok, why = ops.vqframe_plan(1024, 135, 200, 100, True)
    assert route == "staged" and not fused_ok and "LDS" in why
    assert ops.vqframe_plan(128, 135, 300, 80, True)[1] is False and ops.vqframe_plan(128, 135, 40, 257, True)[1] is False
    for B in (1, 0, -3):
        route, fused_ok, why = ops.vqframe_plan(B, 135, 40, 80, True)
        assert route == "" and not fused_ok and "refused" in why
    # eval: the grid kernel serves any number of rows, D, L <= 256, K up to what the GENEA config asks for and beyond
    for N in (1, 63, 1000, 1 << 20):
        assert ops.vqframe_plan(N, 135, 200, 100, False)[1] and ops.vqframe_plan(N, 135, 40, 80, False)[1]
    assert not ops.vqframe_plan(64, 257, 40, 80, False)[1] and not ops.vqframe_plan(64, 135, 257, 80, False)[1]
    assert lib.g2v_vqframe_workspace(1000, 135, 200, 100, 0) >= 400
    # `auto` is one of the two routes wherever a route exists, and FUSED only where the kernel admits the shape
    for args in ((128, 135, 40, 80, True), (1024, 135, 200, 100, True), (1 << 20, 135, 40, 80, False)):
        route, fused_ok, _ = ops.vqframe_plan(*args)
        assert route in ("fused", "staged") and (route != "fused" or fused_ok)


def test_refusals_by_name(fx):
    import argparse
    from gesture2vec_amd.model.DAE_model import VQ_Frame
    with pytest.raises(NotImplementedError, match=r"VQ_Frame\(vae=True\)"):
        VQ_Frame(135, 40, True, 80)
    net = VQ_Frame(135, 40, False, 80)
    assert {k: list(v.shape) for k, v in net.state_dict().items()} == json.loads(str(fx["e/state_dict"]))
    assert list(net.state_dict()) == list(json.loads(str(fx["e/state_dict"])))
    assert (net.skip_vq, net.vq_components, net.commitment_cost, net.vae, net.dropout.p) == (False, 80, 0.25, False, 0.5)
    net.train(True)
    with pytest.raises(ValueError, match="at least 2 frames"):
        net(torch.zeros(1, 135, 1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(torch.zeros(4, 135, 1))
    net.train(False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net.codes(torch.zeros(4, 135))
    net.route = "sideways"
    with pytest.raises(ValueError, match="route"):
        net.resolve(4, False)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    import train_DAE
    args = argparse.Namespace(autoencoder_vq="True", autoencoder_vae="True", input_motion_dim=135, hidden_size=40,
                              autoencoder_vq_components=80)
    with pytest.raises(NotImplementedError, match="VAE_Network"):
        train_DAE.init_model(args, None, 135, "cpu")
    args.autoencoder_vae = "False"
    assert isinstance(train_DAE.init_model(args, None, 135, "cpu")[0], VQ_Frame)
