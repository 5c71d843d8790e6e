"""CPU-only: the float64 restatement of the decoder rollout pair (tests/_dec_ref.py) against the oracle's decoder_step, and the
conditions every case of DEC_F64_CASES (tests/_dec_route_shapes.py) must meet before tests/test_gpu_dec_rollout_f64.py may hold a
kernel to it: few and harmless ambiguous ReLU elements, the named route, and every bound under its cap.  No kernel is launched."""
import pytest
import torch

import _dec_ref as R
import _dec_route_shapes as DS
from oracle import g2v_oracle as O


def _oracle(inp, dtype, n_pre, conditioned, training, p, grad):
    """the rollout built on O.decoder_step, as _oracle_rollout of tests/test_gpu_ops.py has it"""
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in inp["sd"].items()}
    names = [R.PRE + k for k in R.PARAMS]
    for k in names:
        sd[k] = sd[k].clone().requires_grad_(grad)
    tgt = inp["target"].to(dtype).transpose(0, 1)
    bn = {"running_mean": sd[R.PRE + "pre_linear.1.running_mean"].clone(), "running_var": sd[R.PRE + "pre_linear.1.running_var"].clone(),
          "num_batches_tracked": torch.zeros((), dtype=torch.int64)}
    outs, dec_in, hidden = [tgt[0]], tgt[0], inp["h_init"].to(dtype)
    for t in range(1, inp["T"]):
        il = inp["keep_l0"][t - 1] if (training and p > 0) else None
        y, hidden = O.decoder_step(dec_in, hidden, sd, 2, training, inp["keep95"][t - 1], p, il, bn, conditioned=conditioned)
        outs.append(y)
        dec_in = tgt[t] if t < n_pre else y
    y = torch.stack(outs)
    grads = None
    if grad:
        grads = dict(zip(names, torch.autograd.grad((y * inp["gy"].to(dtype)).sum(), [sd[k] for k in names], allow_unused=True)))
    return y.detach(), bn, grads


@pytest.mark.parametrize("T,B,D,H,p,n_pre,conditioned,training", [
    (5, 9, 7, 12, 0.0, 1, True, True), (6, 20, 40, 52, 0.2, 3, True, True), (4, 8, 3, 8, 0.2, 1, False, True),
    (4, 6, 135, 64, 0.2, 1, True, False), (2, 1, 1, 4, 0.0, 1, True, True)])
def test_restatement_agrees_with_the_oracle_decoder_step(T, B, D, H, p, n_pre, conditioned, training):
    """(unconditioned: every row's u is b_pre, so the batch variance is 0 and 1 / sqrt(eps) = 316 multiplies whatever rounding the
    mean of B equal numbers leaves in u - mean.  The restatement takes the mean of u - b_pre, which is exact there; the oracle's
    is exact where B is a power of two, hence B = 8.)"""
    inp = R.inputs(T, B, D, H, p, seed=3, training=training)
    mode = dict(n_pre=n_pre, conditioned=conditioned, training=training, p=p)
    y_o, bn_o, _ = _oracle(inp, torch.float32, grad=False, **mode)
    r32 = R.rollout(inp, torch.float32, **mode)
    assert float(R.step_err(r32["y"], y_o, "y").max()) <= 1e-6
    for k in ("running_mean", "running_var"):
        assert float(R.step_err(r32[k], bn_o[k], k).max()) <= 1e-6, k
    if not training:
        assert torch.equal(r32["running_mean"], inp["sd"][R.PRE + "pre_linear.1.running_mean"])
        return
    _, _, g_o = _oracle(inp, torch.float64, grad=True, **mode)
    g_r = R.rollout(inp, torch.float64, grad=True, **mode)["params"]
    scale = max(float(g.abs().max()) for g in g_o.values() if g is not None)
    for k, g in g_o.items():      # (1e-10 of the largest parameter gradient: an identically zero one has no scale of its own)
        g = torch.zeros_like(g_r[k]) if g is None else g
        assert float((g_r[k] - g).abs().max()) <= 1e-10 * scale, k


def test_forced_mask_equal_to_the_plain_pattern_reproduces_the_plain_backward():
    inp = R.inputs(6, 20, 40, 52, 0.2, seed=1)
    mode = dict(n_pre=3, conditioned=True, training=True, p=0.2)
    plain = R.rollout(inp, torch.float64, grad=True, **mode)
    forced = R.rollout(inp, torch.float64, relu_mask=plain["a_pre"] > 0, grad=True, **mode)
    for k in R.FWD_ARRAYS + R.GRADS:
        assert torch.equal(plain[k], forced[k]), k
    for k, g in plain["params"].items():
        assert torch.equal(g, forced["params"][k]), k


def test_b1_and_unconditioned_slices_are_exactly_zero_in_the_reference():
    """what the device test relies on where a reference slice has no scale: du at B = 1, xin without conditioning"""
    g = R.rollout(R.inputs(3, 1, 1, 4, 0.0, seed=14), torch.float64, grad=True, n_pre=1, conditioned=True, training=True, p=0.0)
    assert float(g["du"].abs().max()) == 0.0 and float(g["dbn"].abs().max()) > 0.0
    f = R.rollout(R.inputs(4, 5, 3, 8, 0.2, seed=0), torch.float64, n_pre=1, conditioned=False, training=True, p=0.2)
    assert float(f["xin"].abs().max()) == 0.0
    assert torch.equal(f["bn_stats"][:, 1], torch.zeros_like(f["bn_stats"][:, 1]))      # every row's u is b_pre: the variance is exactly 0


def test_check_passes_the_float32_restatement_and_catches_planted_defects():
    """R.check, the assertion of the device test, on a stand-in for a kernel: the float32 restatement passes every array; the same
    arrays with one hidden-unit tile of one late step off by 1e-5, and with the BatchNorm sums of a ragged 4-row tile scaled by
    16 / rows, do not."""
    case = next(c for c in DS.DEC_F64_CASES if c["id"] == "PERSIST*1-6x20x135x64-long")
    ref = R.reference(case)
    f32 = R.rollout(ref["inp"], torch.float32, **ref["mode"])
    for k in ("y", "u", "a", "h0", "h1", "x1", "gates0", "gates1", "bn_stats"):
        assert R.check("float32", k, f32[k], ref["f64"][k], ref["e32"][k])[0], k
    off = f32["h1"].clone()
    off[4, :, 16:32] *= 1 + 1e-5                                   # one 16-unit tile, one step
    assert not R.check("planted tile", "h1", off, ref["f64"]["h1"], ref["e32"]["h1"])[0]
    u = f32["u"][2]
    c = u - ref["inp"]["sd"][R.PRE + "pre_linear.0.bias"]
    s1 = c[:16].sum(0) + c[16:].sum(0) * (16 / 4)                  # rows 16..19: the ragged tile's sums mis-scaled
    stats = f32["bn_stats"].clone()
    stats[2, 0] = s1 / 20 + ref["inp"]["sd"][R.PRE + "pre_linear.0.bias"]
    assert not R.check("planted ragged tile", "bn_stats", stats, ref["f64"]["bn_stats"], ref["e32"]["bn_stats"])[0]


@pytest.mark.parametrize("case", DS.DEC_F64_CASES, ids=lambda c: c["id"])
def test_case_meets_the_conditions_of_its_reference(case):
    fl = ("UNALIGNED",) if case["unaligned"] else ()
    q = dict(persistent=case["level"], cus=256, flags=fl)
    assert DS.route_name(case["T"], case["B"], case["D"], case["H"], training=bool(case["training"]), **q) == case["route"]
    if case["training"]:
        assert DS.route_name(case["T"], case["B"], case["D"], case["H"], backward=True, **q) == case["route_bwd"]
    ref = R.reference(case)
    n, amb = ref["ambiguous"].numel(), int(ref["ambiguous"].sum())
    assert amb * 10000 <= n, f"{amb} ambiguous ReLU elements of {n} (tau {ref['tau']:.1e}): take the next seed"
    assert ref["pattern32_differs"] == 0, "the float32 ReLU pattern differs from the float64 one outside the ambiguous elements"
    if case["B"] == 1:      # (the seeds of the B = 1 cases are chosen for this, tests/_dec_route_shapes.py)
        assert float(ref["f64"]["a"].abs().amax(dim=(1, 2)).min()) > 0 and (not case["conditioned"] or float(ref["f64"]["xin"].abs().max()) > 0)
    for k, e32 in ref["e32"].items():
        worst = float((R.MARGIN * torch.clamp(e32, min=2 * R.U)).max())
        assert worst < R.cap_of(k), f"{k}: 8 e32 = {worst:.2e} reaches the cap {R.cap_of(k):.0e}: shorten the case"


def test_cases_meet_every_route_in_both_directions():
    assert {c["route"].split("*")[0] for c in DS.DEC_F64_CASES} == set(DS.ROUTES)
    assert {c["route_bwd"].split("*")[0] for c in DS.DEC_F64_CASES if c["route_bwd"]} == set(DS.ROUTES)
    assert {c["route"] for c in DS.DEC_F64_CASES} >= {"PERSIST*1", "PERSIST*2", "PERSIST*3"}
    assert {c["route_bwd"] for c in DS.DEC_F64_CASES} >= {"PERSIST*1", "PERSIST*2", "PERSIST*3"}
