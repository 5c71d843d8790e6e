"""Host side of the loss / optimiser kernel tests (tests/_loss_inputs.py): the float64 references against the fixtures, the plain
oracle and torch itself, and the conditions every case of tests/test_gpu_loss_path.py must meet on the reference alone -- finite,
a clip decision out of rounding reach, and noise floors (fp32 reference against float64) under the caps its bounds are built from."""
import math
import os

import numpy as np
import pytest
import torch

import _loss_inputs as L
from oracle import g2v_oracle as O


# ------------------------------------------------------------------------------------------------ custom_loss
def test_custom_loss_in_fp32_reproduces_the_golden_fixture(golden_dir):
    """loss and gradient of tests/golden/custom_loss.npz at the tolerance of test_oracle_golden.py::test_custom_loss_matches_reference"""
    fx = np.load(os.path.join(golden_dir, "custom_loss.npz"))
    w = tuple(float(x) for x in fx["weights"])
    for tag in ("a", "b"):
        out, tgt = torch.from_numpy(fx[f"{tag}/output"].copy()), torch.from_numpy(fx[f"{tag}/target"].copy())
        r = L.custom_loss(out, tgt, w, 1.0, torch.float32)
        np.testing.assert_allclose(float(r["total"]), float(fx[f"{tag}/loss"]), rtol=1e-6)
        np.testing.assert_allclose(r["dy"].numpy(), fx[f"{tag}/grad"], rtol=1e-5, atol=1e-9)
        r64 = L.custom_loss(out, tgt, w, 1.0, torch.float64)
        np.testing.assert_allclose(float(r64["total"]), float(fx[f"{tag}/loss"]), rtol=1e-6)
        np.testing.assert_allclose(r64["dy"].numpy(), fx[f"{tag}/grad"], rtol=1e-5, atol=1e-9)


@pytest.mark.parametrize("name", ["1x1x1", "7x9x40", "3x34x85-g3", "5x20x135-s1000", "2x34x128-w123", "3x33x135-s0.001-g3"])
def test_custom_loss_agrees_with_the_plain_oracle_where_no_column_is_zero(name):
    """in float64, on the case's inputs with the planted zero column replaced (oracle.custom_loss takes sqrt(sum(o^2)), whose
    gradient at a zero column is NaN); the terms add up and mse is the plain mean square"""
    c = L.CL_CASES[name]
    out, tgt = (t.double() for t in L.cl_inputs(name))
    pl = L.cl_planted(c)
    if pl:
        b, d = pl["zero_col"]
        out[b, :, d] = 0.25 * c.scale
    r = L.custom_loss(out, tgt, c.weights, c.g_scale)
    o = out.clone().requires_grad_(True)
    v = O.custom_loss(o, tgt, *c.weights)
    (g,) = torch.autograd.grad(v, o)
    assert abs(float(r["total"]) - float(v.detach())) <= 1e-12 * L.cl_total_scale(r)
    assert L.relerr(r["dy"], c.g_scale * g) <= 1e-12
    assert float(r["total"]) == float(r["l1"] + r["cont"] + r["var"])
    assert abs(float(r["mse"]) - float(torch.nn.functional.mse_loss(out, tgt))) <= 1e-13 * float(r["mse"])
    assert float(r["l1"]) >= 0 and float(r["cont"]) >= 0 and float(r["var"]) <= 0


@pytest.mark.parametrize("name", list(L.CL_CASES))
def test_custom_loss_case_is_finite_and_carries_its_edge_values(name):
    c = L.CL_CASES[name]
    out, tgt = L.cl_inputs(name)
    ref = L.cl_reference(name)
    assert all(bool(torch.isfinite(v).all()) for v in ref.values())
    B, T, D = c[:3]
    assert T * B * D < 2 ** 24                                  # n is exact in fp32 (cl_scalar_bounds)
    pl = L.cl_planted(c)
    if pl is None:
        assert T == 1 and float(ref["cont"]) == 0.0
        return
    b, d = pl["zero_col"]
    assert bool((out[b, :, d] == 0).all())
    n, (w1, _, _) = T * B * D, c.weights
    # on the zero column every cont sign and the norm term vanish: dy = g_scale c1 sign(0 - target), loss_grad_const of its signs
    want = c.g_scale * (w1 / n) * torch.sign(-tgt[b, :, d].double())
    assert L.relerr(ref["dy"][b, :, d], want) <= 1e-14 and float(want.abs().min()) > 0
    b, d = pl["const_col"]
    assert bool((out[b, :, d] == out[b, 0, d]).all()) and float(out[b, 0, d]) != 0
    b, t, nd = pl["repeat"]
    assert t >= 1 and bool((out[b, t, :nd] == out[b, t - 1, :nd]).all())
    b, t, d = pl["equal"]
    assert float(out[b, t, d]) == float(tgt[b, t, d])
    e = L.cl_noise(name)
    print(name, " ".join(f"{k}={v:.2e}" for k, v in e.items()))
    sb = L.cl_scalar_bounds(c)
    for k in ("l1", "cont", "var", "mse", "total"):
        assert e[k] <= sb[k], (k, e[k], sb[k])                  # torch's own fp32 sums stay inside the a-priori bound


# ------------------------------------------------------------------------------------------------ MSE
@pytest.mark.parametrize("name", list(L.MSE_CASES))
def test_mse_reference_is_torchs(name):
    n, gs = L.MSE_CASES[name]
    y, t = (x.double() for x in L.mse_inputs(name))
    ref = L.mse_reference(name)
    yl = y.clone().requires_grad_(True)
    loss = torch.nn.functional.mse_loss(yl, t)
    (g,) = torch.autograd.grad(loss, yl)
    assert abs(float(ref["loss"]) - float(loss.detach())) <= 1e-13 * float(loss.detach())
    assert L.relerr(ref["dy"], gs * g) <= 1e-13
    assert bool(torch.isfinite(ref["dy"]).all()) and math.isfinite(float(ref["loss"]))
    nz = ref["dy"][ref["dy"] != 0].abs()
    assert n < 2 ** 24 and float(nz.min()) > 1e-30              # n exact in fp32; no non-zero element near the subnormal range
    o32 = L.mse(*L.mse_inputs(name), gs, torch.float32)
    assert abs(float(o32["loss"]) - float(ref["loss"])) <= L.mse_loss_bound(n) * float(ref["loss"])
    assert 0 < L.mse_loss_bound(n) < 1e-5


# ------------------------------------------------------------------------------------------------ clip + Adam
@pytest.mark.parametrize("name", [n for n in L.ADAM_CASES if not n.startswith(("100003", "2097155"))] + ["100003-gs0.125-clipped"])
def test_adam_reference_agrees_with_the_oracle_and_with_torch_optim(name):
    """at the betas the C ABI carries (fp32 values of (0.5, 0.999), held as doubles), which are within fp32 rounding of the caller's"""
    assert all(abs(a - b) <= L.U * b for a, b in zip(L.BETAS_ABI, L.BETAS)) and L.BETAS_ABI[0] == 0.5
    c = L.ADAM_CASES[name]
    p0, grads = L.adam_inputs(name)
    ref = L.adam_reference(name)
    # oracle.clip_grad_norm + oracle.adam_step in float64
    params, state = {"w": p0.double()}, {}
    for k, g in enumerate(grads):
        clipped, total = O.clip_grad_norm({"w": g.double() * c.grad_scale}, L.MAX_NORM)
        O.adam_step(params, clipped, state, L.LR, L.BETAS_ABI, L.EPS)
        assert abs(float(total) - float(ref["gnorm"][k])) <= 1e-13 * max(float(total), 1e-300)
    assert state["w"]["step"] == ref["step"] == L.ADAM_STEPS
    for k, v in (("p", params["w"]), ("m", state["w"]["m"]), ("v", state["w"]["v"])):
        assert L.relerr(ref[k], v) <= 1e-12, k
    # a real torch.optim.Adam behind torch.nn.utils.clip_grad_norm_
    w = torch.nn.Parameter(p0.double())
    opt = torch.optim.Adam([w], lr=L.LR, betas=L.BETAS_ABI, eps=L.EPS)
    for k, g in enumerate(grads):
        w.grad = g.double() * c.grad_scale
        total = torch.nn.utils.clip_grad_norm_([w], L.MAX_NORM)
        assert abs(float(total) - float(ref["gnorm"][k])) <= 1e-13 * max(float(total), 1e-300)
        opt.step()
    st = opt.state[w]
    assert int(st["step"]) == ref["step"]
    for k, v in (("p", w.detach()), ("m", st["exp_avg"]), ("v", st["exp_avg_sq"])):
        assert L.relerr(ref[k], v) <= 1e-12, k


@pytest.mark.parametrize("name", list(L.ADAM_CASES))
def test_adam_case_is_finite_with_its_clip_decision_out_of_rounding_reach(name):
    c = L.ADAM_CASES[name]
    ref = L.adam_reference(name)                       # (asserts the clip-ratio condition itself)
    assert all(bool(torch.isfinite(ref[k]).all()) for k in ("p", "m", "v", "gnorm"))
    ratios = L.clip_ratios(name)
    lo, hi = L.CLIP_BAND
    assert len(ratios) == L.ADAM_STEPS and all(not lo <= r <= hi for r in ratios)
    want = L.ADAM_REGIMES[c.regime]
    assert all(abs(r - w) <= 1e-6 * max(w, 1e-3) for r, w in zip(ratios, want))
    if c.regime == "clipped":
        assert any(r > 1 for r in ratios) and any(r < 1 for r in ratios)
    if c.regime == "unclipped":
        assert all(r < 1 for r in ratios)
    p0, grads = L.adam_inputs(name)
    if c.regime == "zero-first":
        one = L.clip_adam(p0, grads[:1], c.grad_scale)
        assert bool((grads[0] == 0).all()) and torch.equal(one["p"], p0.double()) and float(one["v"].abs().max()) == 0
    if c.regime == "zero-init":
        assert float(p0.abs().max()) == 0 and 0.1 * L.LR < float(ref["p"].abs().max()) < 10 * L.LR       # p is the updates alone
    e = L.adam_noise(name)
    assert e["gnorm"] <= L.gnorm_bound(c.n), (e["gnorm"], L.gnorm_bound(c.n))


# ------------------------------------------------------------------------------------------------ cross entropy
@pytest.mark.parametrize("name", list(L.CE_CASES))
def test_cross_entropy_reference_is_torchs_and_the_case_holds_its_regimes(name):
    M, K = L.CE_CASES[name]
    z, t = L.ce_inputs(name)
    ref = L.ce_reference(name)
    assert math.isfinite(float(ref["loss"])) and bool(torch.isfinite(ref["grad"]).all()) and bool(torch.isfinite(z).all())
    # written out: mean_r (lse_r - z_r,t), gradient (softmax - onehot) / M
    zd = z.double()
    lse = torch.logsumexp(zd, 1)
    assert abs(float((lse - zd[torch.arange(M), t]).mean()) - float(ref["loss"])) <= 1e-13 * max(float(ref["loss"]), 1.0)
    g = torch.softmax(zd, 1)
    g[torch.arange(M), t] -= 1
    assert L.relerr(ref["grad"], g / M) <= 1e-13
    assert int(t.min()) == 0 or M == 1
    assert int(t.max()) == K - 1
    pl = L.ce_planted(M, K)
    if pl:
        r = pl["far_target"]
        assert abs(float(zd[r].max() - zd[r, t[r]]) - 1e4) < 1.0 and float(zd[r].max()) > 100     # exp(z) itself overflows fp32
        assert abs(float(ref["grad"][r, t[r]]) + 1.0 / M) <= 1e-15
        assert float(z[pl["pm80"]].max()) > 75 and float(z[pl["pm80"]].min()) < -75
        assert float(z[pl["equal"]].max()) == float(z[pl["equal"]].min())
    e = L.ce_noise(name)
    assert e["loss"] <= L.ce_loss_bound(name), (e["loss"], L.ce_loss_bound(name))


# ------------------------------------------------------------------------------------------------ the bounds
def test_floors_are_finite_and_under_the_caps():
    """the fp32 reference alone stays inside every bound it defines"""
    fl = L.floors()
    assert set(fl) == set(L.CAP)
    for k, v in fl.items():
        print(f"floor {k} = {v:.3e} (cap {L.CAP[k]:.0e})")
        assert math.isfinite(v) and 0 < v <= 0.2 * L.CAP[k], (k, v)
    for out, cases in (("dy", L.CL_CASES), ("ce_grad", L.CE_CASES), ("p", L.ADAM_CASES), ("m", L.ADAM_CASES), ("v", L.ADAM_CASES)):
        for name in cases:
            b, e32 = L.bound(name, out), L.noise_of(name, out)
            assert e32 <= b <= L.CAP[out] and b >= min(fl[out], L.CAP[out]) and b <= max(L.MARGIN * e32, fl[out])


def test_scalar_bounds_are_a_few_hundred_roundings_at_most():
    for c in L.CL_CASES.values():
        assert all(0 < v < 1e-5 for v in L.cl_scalar_bounds(c).values())
    assert all(0 < L.gnorm_bound(n) < 2e-6 for n in L.ADAM_SIZES)
    assert L.gamma(1) == L.U and abs(L.gamma(100) - 100 * L.U) < 1e-10
