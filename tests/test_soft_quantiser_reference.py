"""Host side of the soft quantiser tests (tests/_soft_inputs.py): the staged float64 reference against the plain oracle, and the
conditions every case of tests/test_gpu_soft_quantiser.py must meet on the reference alone -- finite in fp32, a rounding noise floor
(fp32 oracle against float64) that its bounds are built from, and few near-tie rows for the assign() check."""
import pytest
import torch

import _soft_inputs as S
from _f64 import as64, default64
from oracle import g2v_oracle as O


@pytest.mark.parametrize("name", ["sep-257x100x70", "sep-33x64x48", "fused-17x128x1024", "sep-517x400x512-peaked", "sep-1x400x512"])
@pytest.mark.parametrize("g_scale", [S.G_SCALE, S.G_LOSS])
def test_staged_reference_equals_the_plain_oracle_in_float64(name, g_scale):
    """forward values, and with g_scale == g_loss every gradient of L = sum(quant dh) + g_loss loss by plain autograd, to 1e-12;
    with g_scale != g_loss the same against L = sum(quant dh) + g_scale q_latent + g_loss beta e_latent written out on the oracle's
    outputs"""
    inp = S.make_inputs(S.ALL_CASES[name])
    st = S.staged(inp, torch.float64, g_scale=g_scale)
    with default64():
        t = as64(inp)
        x = t["x"].clone().requires_grad_(True)
        sd = {k: v.clone().requires_grad_(True) for k, v in S.state_dict(t, "vq.").items()}
        fw = O.vq_gssoft_forward(x, sd, "vq.", S.BETA)
        N, E = x.shape
        for k in ("flat", "dist", "probs", "quant", "perplexity"):
            assert S.relerr(st[k], fw[k == "quant" and "quantized" or k]) <= 1e-12, k
        assert abs(float(st["mse"]) * (1 + S.BETA) - float(fw["loss"].detach())) <= 1e-12 * float(fw["loss"].detach())
        assert abs(float(st["loss_vq"]) - float(fw["loss"].detach())) <= 1e-12 * float(fw["loss"].detach())
        q = fw["probs"] @ sd["vq._embedding.weight"]
        assert S.relerr(st["q"], q) <= 1e-12
        assert S.relerr(st["dq"], g_scale * 2 * (q - x) / (N * E)) <= 1e-12
        if g_scale == S.G_LOSS:
            L = (fw["quantized"] * t["dh"]).sum() + S.G_LOSS * fw["loss"]
        else:
            L = ((fw["quantized"] * t["dh"]).sum() + g_scale * ((q - x.detach()) ** 2).mean()
                 + S.G_LOSS * S.BETA * ((q.detach() - x) ** 2).mean())
        L.backward()
        for k, ref in (("gz", x.grad), ("g_mean_w", sd["vq.mean_layer.weight"].grad), ("g_mean_b", sd["vq.mean_layer.bias"].grad),
                       ("g_logvar_w", sd["vq.logvar_layer.weight"].grad), ("g_logvar_b", sd["vq.logvar_layer.bias"].grad),
                       ("g_embedding", sd["vq._embedding.weight"].grad)):
            assert S.relerr(st[k], ref) <= 1e-12, (k, S.relerr(st[k], ref))
        assert sd["vq.pre_linear.weight"].grad is None and sd["vq.pre_linear.bias"].grad is None


def test_staged_intermediate_gradients_are_the_chain_rule_pieces():
    """dd, dlogvar, rowsum and dflat are not outputs of plain autograd on the oracle: tie them to what is -- dflat = 2 flat rowsum -
    2 dd W + dlogvar W_logvar, gz = dh + g_loss beta 2 (x - q) / (N E) + dflat W_mean, and the parameter gradients built from them."""
    name = "sep-257x100x70"
    inp, st = S.reference(name)
    t = as64(inp)
    N, E = t["x"].shape
    W, flat = t["codebook"], st["flat"]
    assert S.relerr(st["rowsum"], st["dd"].sum(1)) <= 1e-13
    dflat = 2 * flat * st["rowsum"][:, None] - 2 * st["dd"] @ W + st["dlogvar"] @ t["w_logvar"]
    assert S.relerr(st["dflat"], dflat) <= 1e-12
    gz = t["dh"] + S.G_LOSS * S.BETA * 2 * (t["x"] - st["q"]) / (N * E) + st["dflat"] @ t["w_mean"]
    assert S.relerr(st["gz"], gz) <= 1e-12
    assert S.relerr(st["g_logvar_w"], st["dlogvar"].t() @ flat) <= 1e-12
    assert S.relerr(st["g_logvar_b"], st["dlogvar"].sum(0)) <= 1e-12
    assert S.relerr(st["g_mean_w"], st["dflat"].t() @ t["x"]) <= 1e-12
    gW = 2 * W * st["dd"].sum(0)[:, None] - 2 * st["dd"].t() @ flat + st["probs"].t() @ st["dq"]
    assert S.relerr(st["g_embedding"], gW) <= 1e-12
    s = torch.exp(-2 * st["logvar"])
    g = -800 * st["dd"] / s                      # d L / d log prob_k of the kernels' derivation (csrc/vq.hip: vq_soft_bwd_kernel)
    assert S.relerr(st["dlogvar"], g * (1 + st["dist"] * s / 400)) <= 1e-11


@pytest.mark.parametrize("name", list(S.ALL_CASES))
def test_case_is_finite_in_fp32_and_has_a_noise_floor(name):
    inp, ref = S.reference(name)
    o32 = S.staged(inp, torch.float32, g_scale=S.g_scale_of(name))
    for k in S.OUTPUTS:
        assert bool(torch.isfinite(o32[k]).all()), f"{k}: the fp32 oracle is not finite"
    s = torch.exp(-2 * ref["logvar"])
    prob = torch.exp(-ref["dist"] * s / 800) / torch.sqrt(s)
    assert float(prob.sum(1).min()) > 1e-30
    e32 = S.noise(name)
    print(name, "perplexity %.1f" % float(ref["perplexity"]), " ".join(f"{k}={v:.2e}" for k, v in e32.items()))
    for k, v in e32.items():
        # fp32 rounding of well-conditioned sums: far below every tolerance the fused-versus-separate test uses
        assert 0.0 <= v <= 0.2 * S.CAP[k], (k, v)
    assert int(S.near_tie_rows(ref["probs"]).sum()) <= ref["probs"].shape[0] // 100      # the assign() check's condition


def test_peaked_regime_spreads_the_smoothness():
    """the peaked cases are there for the s-dependent factors: s = exp(-2 logvar) must span orders of magnitude in them and stay near 1
    in the flat ones, with a perplexity well inside (1, K)"""
    _, flat = S.reference("sep-517x400x512")
    _, peaked = S.reference("sep-517x400x512-peaked")
    sf, sp = torch.exp(-2 * flat["logvar"]), torch.exp(-2 * peaked["logvar"])
    assert float(sf.max() / sf.min()) < 20 and float(sp.quantile(0.99) / sp.quantile(0.01)) > 1e3
    assert 100 < float(peaked["perplexity"]) < 400 and float(flat["perplexity"]) > 400


def test_bounds_come_from_the_reference_alone():
    fl = S.floors()
    for name in S.ALL_CASES:
        for k in S.OUTPUTS:
            b = S.bound(name, k)
            assert b <= S.CAP[k] and b >= min(fl[k], S.CAP[k]) and b <= max(S.MARGIN * S.noise(name)[k], fl[k])
