"""CPU-only: the float64 restatement of the part d code rollout (tests/_code_ref.py) against the oracle's t2e_forward / attn_weights
and the recorded tests/golden/t2e_noatt.npz / t2e_att.npz, its autograd gradients against torch.autograd.gradcheck, and the
conditions every case of CODE_F64_CASES (tests/_t2e_route_shapes.py) must meet before tests/test_gpu_code_rollout_f64.py may hold
a kernel to it: the named routes, the argmax gap at every free-running step and row, no ReLU decision differing away from zero.
No kernel is launched."""
import os

import numpy as np
import pytest
import torch

import _code_ref as C
import _t2e_route_shapes as TS
from oracle import g2v_oracle as O

PRE = "decoder.decoder."
ORACLE_NAMES = {"emb": "embedding.weight", "w_pre": "pre_linear.0.weight", "b_pre": "pre_linear.0.bias", "bn_w": "pre_linear.1.weight",
                "bn_b": "pre_linear.1.bias", "w_ih0": "gru.weight_ih_l0", "w_hh0": "gru.weight_hh_l0", "b_ih0": "gru.bias_ih_l0",
                "b_hh0": "gru.bias_hh_l0", "w_ih1": "gru.weight_ih_l1", "w_hh1": "gru.weight_hh_l1", "b_ih1": "gru.bias_ih_l1",
                "b_hh1": "gru.bias_hh_l1", "w_out": "out.weight", "b_out": "out.bias", "w_attn": "attn.attn.weight",
                "b_attn": "attn.attn.bias", "v_attn": "attn.v"}


@pytest.mark.parametrize("name,att", [("t2e_noatt", False), ("t2e_att", True)])
@pytest.mark.parametrize("training", [True, False])
def test_restatement_agrees_with_the_oracle_and_the_recorded_outputs(golden_dir, name, att, training):
    """the decoder of O.t2e_forward on the recorded weights, inputs and masks in float64: logits, attention weights, running
    statistics; and the reference's own recorded outputs of the first training step, to what float32 recorded them at"""
    fx = np.load(os.path.join(golden_dir, name + ".npz"))
    B, Tw, S, H, L, K, _, _ = [int(v) for v in fx["cfg"]]
    p = float(fx["cfg_f"][0])
    f64 = lambda t: t.double() if t.is_floating_point() else t
    sd = {k[3:]: f64(torch.from_numpy(fx[k].copy())) for k in fx.files if k.startswith("w0/")}
    ids, lengths, codes = (torch.from_numpy(fx[k].copy()) for k in ("ids", "lengths", "codes"))
    masks = {k: torch.from_numpy(fx[f"s1/mask_{k}"].copy()) for k in ("emb", "dec_l0", "enc_l0")}
    cfg = dict(n_layers=L, dropout_prob=p, n_pre_poses=1, att=att)
    with torch.no_grad():
        r = O.t2e_forward(sd, ids, lengths, codes, cfg, training, masks if training else {})
    S1 = S - 1
    inp = {"S1": S1, "B": B, "H": H, "K": K, "Tw": Tw, "att": att, "p": p, "tie": None,
           "w": {k: sd[PRE + v] for k, v in ORACLE_NAMES.items() if PRE + v in sd},
           "running_mean": sd[PRE + "pre_linear.1.running_mean"], "running_var": sd[PRE + "pre_linear.1.running_var"],
           "codes": codes.t().contiguous(), "h_init": r["encoder_hidden"][:2], "keep_emb": masks["emb"], "keep_l0": masks["dec_l0"],
           "enc": r["encoder_outputs"] if att else None}
    if att:
        inp["enc_proj"] = inp["enc"] @ inp["w"]["w_attn"][:, H:].t()
    got = C.rollout(inp, torch.float64, n_pre=1, training=training)
    want = r["outputs"].transpose(0, 1)[1:]
    assert float((got["logits"] - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert torch.equal(got["ids"][1:], want[:-1].argmax(2)), "the greedy feedback differs from the oracle's"
    if att:
        for t, w in enumerate(r["attn"]):
            assert float((got["attw"][t] - w).abs().max()) <= 1e-13
            assert float((got["attw"][t] - O.attn_weights(got["h1"][t], inp["enc"], inp["w"]["w_attn"], inp["w"]["b_attn"],
                                                          inp["w"]["v_attn"])).abs().max()) <= 1e-13
    for k in ("running_mean", "running_var"):      # (the oracle's two-pass variance against the kernels' one-pass form, in float64)
        assert float((got[k] - r["bn"][k]).abs().max()) <= 1e-12, k
    if training:
        np.testing.assert_allclose(got["logits"].transpose(0, 1).numpy(), fx["s1/outputs"][:, 1:], rtol=1e-4, atol=2e-6)


@pytest.mark.parametrize("att", [False, True])
def test_autograd_gradients_pass_gradcheck(att):
    """3 x 16 x 8: the loss sum <logits, d_logits> along the greedy trajectory and the ReLU pattern of the float64 run, as a function
    of every weight, the initial state and the encoder outputs"""
    inp = C.make_inputs(3, 3, 16, 8, 4 if att else 0, att, 0.2, seed=5)
    if att:      # unrounded, so that the value the rollout is handed IS the product a finite difference moves
        inp["enc_proj"] = inp["enc"].double() @ inp["w"]["w_attn"][:, 16:].double().t()
    f64 = C.rollout(inp, torch.float64)
    names = C.WEIGHTS + (C.ATT_WEIGHTS if att else ())
    leaves = [inp["w"][k].double().requires_grad_() for k in names] + [inp["h_init"].double().requires_grad_()]
    if att:
        leaves.append(inp["enc"].double().requires_grad_())

    def loss(*xs):
        cur = dict(inp, w=dict(zip(names, xs[:len(names)])), h_init=xs[len(names)])
        if att:
            cur["enc"] = xs[-1]
        return _differentiable_loss(cur, f64["ids"], f64["a_pre"] > 0)

    assert torch.autograd.gradcheck(loss, leaves, eps=1e-6, atol=1e-7, rtol=1e-5)
    g = C.rollout(inp, torch.float64, ids=f64["ids"], relu_mask=f64["a_pre"] > 0, grad=True)
    want = torch.autograd.grad(loss(*leaves), leaves, allow_unused=True)
    for k, w in zip(C.grad_names(att)[1:len(names) + 1], want):
        w = torch.zeros_like(g[k]) if w is None else w
        assert float((g[k] - w).abs().max()) <= 1e-12, k
    assert float((g["d_hidden0"] - want[len(names)]).abs().max()) <= 1e-12
    assert float(g["d_b_pre"].abs().max()) <= 1e-12, "b_pre feeds BatchNorm: its gradient is zero"


def _differentiable_loss(inp, ids, pattern):
    """C.rollout's loss with the graph kept: the same recurrence called on tensors that require grad"""
    S1, H, att, p = inp["S1"], inp["H"], inp["att"], inp["p"]
    w, B = inp["w"], inp["B"]
    ke, kl0 = inp["keep_emb"].double(), inp["keep_l0"].double()
    h0, h1 = inp["h_init"][0], inp["h_init"][1]
    if att:
        ep = inp["enc"] @ w["w_attn"][:, H:].t()      # (enc_proj as the function of enc and W_attn it is)
    total = 0.0
    for t in range(S1):
        x = w["emb"][ids[t]] * ke[t] * 2.0
        if att:
            hp = h1 @ w["w_attn"][:, :H].t() + w["b_attn"]
            aw = torch.softmax((torch.tanh(hp.unsqueeze(0) + ep) * w["v_attn"]).sum(2).t(), dim=1)
            x = torch.cat([x, torch.einsum("bt,tbh->bh", aw, inp["enc"])], 1)
        u = x @ w["w_pre"].t() + w["b_pre"]
        a = O.batchnorm1d(u, w["bn_w"], w["bn_b"], torch.zeros(H, dtype=u.dtype), torch.ones(H, dtype=u.dtype), True)[0] * pattern[t]
        h0 = O.gru_cell(O.linear(a, w["w_ih0"], w["b_ih0"]), h0, w["w_hh0"], w["b_hh0"])
        h1 = O.gru_cell(O.linear(kl0[t] * h0 / (1 - p), w["w_ih1"], w["b_ih1"]), h1, w["w_hh1"], w["b_hh1"])
        total = total + ((h1 @ w["w_out"].t() + w["b_out"]) * inp["d_logits"][t].double()).sum()
    return total


def test_argmax_takes_the_lowest_index_among_equal_maxima():
    x = torch.tensor([[1.0, 3.0, 3.0, 2.0], [5.0, 5.0, 5.0, 5.0], [0.0, -1.0, 0.0, 0.0], [-2.0, -2.0, -1.0, -1.0]])
    assert C.argmax_lowest(x).tolist() == [1, 0, 0, 2]


def test_case_ids_are_unique():
    ids = [c["id"] for c in TS.CODE_F64_CASES]
    assert len(set(ids)) == len(ids)


@pytest.mark.parametrize("case", TS.CODE_F64_CASES, ids=lambda c: c["id"])
def test_case_meets_the_conditions_of_its_reference(case):
    kw = dict(S1=case["S1"], B=case["B"], H=case["H"], K=case["K"], Tw=case["Tw"], att=case["att"], persistent=case["level"], cus=256,
              facts=("ENTRY",))
    assert TS.route_name(backward=0, **kw) == case["route"]
    if case["training"]:
        assert TS.route_name(backward=1, **kw) == case["route_bwd"]
    if case["bptt"]:
        assert TS.route_name(backward=2, **kw) == "CLUSTER"
    ok, why = C.admissible(case)
    assert ok, why + ": take the next seed"
    ref = C.reference(case)
    assert ref["pattern32_differs"] == 0
    assert ref["ids32_differ"] == 0, "the float32 restatement left to itself feeds other codes than the float64 run"
    if case["tie"] is not None:
        k1, k2 = case["tie"][:2]
        fed = ref["f64"]["ids"][ref["f64"]["free"]]
        assert int((fed == k1).sum()) * 4 >= fed.numel() and int((fed == k2).sum()) == 0, "the planted pair is not preferred"
        lg = ref["f64"]["logits"]
        assert torch.equal(lg[..., k1], lg[..., k2])
    if case["training"] and case["B"] > 1:      # (a reference gradient that is exactly zero has no scale: only d_b_pre may be)
        assert float(ref["g64"]["d_b_pre"].abs().max()) == 0.0
        zero = {"d_b_pre"} | ({"d_w_attn", "d_b_attn", "d_v_attn"} if case["Tw"] == 1 else set())      # (one position: its weight is 1)
        assert {k for k in C.grad_names(case["att"]) if float(ref["g64"][k].abs().max()) == 0} == zero


def test_check_passes_the_float32_restatement_and_catches_planted_defects():
    """C.check, the assertion of the device test, on a stand-in for a kernel: the float32 restatement passes every array; without
    the 1 / (1 - p) of the inter-layer dropout, or feeding the higher of two tied codes, it does not"""
    case = next(c for c in TS.CODE_F64_CASES if c["id"] == "STEP-33x48x40-drop")
    ref = C.reference(case)
    f32 = C.rollout(ref["inp"], torch.float32, **ref["mode"])
    assert torch.equal(f32["ids"], ref["f64"]["ids"])
    for k in C.fwd_names(case):
        assert C.check("float32", k, f32[k], ref["f64"][k], ref["e32"][k], cap=C.cap_of(k), steps_of=C.steps_of(k))[0], k
    slip = f32["x1"] * (1.0 - case["p"])                                 # the rescaling left out
    assert not C.check("no rescaling", "x1", slip, ref["f64"]["x1"], ref["e32"]["x1"], cap=C.cap_of("x1"), steps_of="y")[0]
    tie = next(c for c in TS.CODE_F64_CASES if c["tie"] is not None)
    ref = C.reference(tie)
    k1, k2 = tie["tie"][:2]
    highest = torch.where(ref["f64"]["ids"] == k1, torch.full_like(ref["f64"]["ids"], k2), ref["f64"]["ids"])
    assert not torch.equal(highest, ref["f64"]["ids"])
