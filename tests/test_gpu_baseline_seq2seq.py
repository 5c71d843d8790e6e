"""GPU parity of the text -> pose baseline (Seq2SeqNet): the reference's golden vectors on both routes, the fused step kernels
(csrc/pose_attn.hip) against the float64 restatement (tests/_pose_attn_ref.py) and against the per-operator route, the feedback
gradient, the refusals of the C entries, and the surface (checkpoint, trainer script, refused options)."""
import argparse
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pose_attn_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRE_B = "decoder.decoder.pre_linear.0.bias"


def relerr(got, ref, scale=None):
    got = torch.as_tensor(got).detach().cpu().double().reshape(-1)
    ref = torch.as_tensor(ref).detach().cpu().double().reshape(-1)
    return float((got - ref).abs().max()) / max(float(ref.abs().max()) if scale is None else scale, 1e-300)


def _args(H, p, n_pre, S, w=(5.0, 0.1, 0.5)):
    return argparse.Namespace(hidden_size=H, n_layers=2, dropout_prob=p, n_pre_poses=n_pre, n_poses=S, loss_l1_weight=w[0],
                              loss_cont_weight=w[1], loss_var_weight=w[2])


def _route(monkeypatch, route):
    from gesture2vec_amd import rollout_t2e
    monkeypatch.setattr(rollout_t2e, "POSE_FUSED_MIN_ROWS", 1 if route == "fused" else 1 << 30)


# ---- 1. the reference's own numbers ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["per_operator", "fused"])
def test_baseline_matches_reference_golden(golden_dir, route, monkeypatch):
    """Two training iterations and the eval forward against the reference's recorded run (tests/golden/make_fixtures_baseline.py),
    at the bars of test_latent_text2embedding_matches_reference_golden: loss 1e-5 relative, gradients 5e-4, final weights as there,
    eval outputs 1e-4.  route="auto" with POSE_FUSED_MIN_ROWS forced to 1 / 1 << 30; the call counter shows which route ran."""
    from gesture2vec_amd import rollout_t2e
    from gesture2vec_amd.flat import FlatClipAdam
    from gesture2vec_amd.model.seq2seq_net import Seq2SeqNet
    from gesture2vec_amd.train_eval.train_seq2seq import train_iter_seq2seq
    _route(monkeypatch, route)
    calls0 = rollout_t2e.POSE_FUSED_CALLS
    with np.load(os.path.join(golden_dir, "baseline_seq2seq.npz")) as f:
        fx = {k: f[k] for k in f.files}
    B, Tw, S, NPRE, D, H, L, NW, EMB = [int(v) for v in fx["cfg"]]
    p, lr, w1, w2, w3 = [float(v) for v in fx["cfg_f"]]
    args = _args(H, p, NPRE, S, (w1, w2, w3))
    net = Seq2SeqNet(args, D, S, NW, EMB, np.zeros((NW, EMB), dtype=np.float32), None)
    net.load_state_dict({k[3:]: torch.from_numpy(fx[k].copy()) for k in fx if k.startswith("w0/")}, strict=True)
    net = net.to(DEV)
    net.train(True)
    assert net.route == "auto"
    optim = FlatClipAdam(net.parameters(), lr=lr, betas=(0.5, 0.999))
    ids = torch.from_numpy(fx["ids"].copy()).to(DEV)
    lengths = torch.from_numpy(fx["lengths"].copy())
    poses = torch.from_numpy(fx["poses"].copy()).to(DEV)
    for step in (1, 2):
        net.set_dropout_masks(torch.from_numpy(fx[f"s{step}/mask_dec_l0"].copy()).to(DEV),
                              torch.from_numpy(fx[f"s{step}/mask_enc_l0"].copy()).to(DEV).to(torch.uint8))
        loss = train_iter_seq2seq(args, 1, ids, lengths, poses, net, optim)
        ref = float(fx[f"s{step}/loss"])
        print(f"{route} step {step}: loss {loss['loss']:.8f} ref {ref:.8f} rel {abs(loss['loss'] - ref) / ref:.2e}")
        assert net.last_route == route
        assert abs(loss["loss"] - ref) <= 1e-5 * ref, (loss, ref)
        if step == 1:
            for n, prm in net.named_parameters():
                if n == PRE_B:
                    continue                       # feeds BatchNorm: mathematically zero
                err = relerr(prm.grad, fx["s1/grad/" + n]) if prm.grad is not None else float("inf")
                print(f"  grad {n}: {err:.2e}")
                assert err < 5e-4, (n, err)
    assert rollout_t2e.POSE_FUSED_CALLS - calls0 == (2 if route == "fused" else 0)
    for k in fx:
        if k.startswith("wN/"):
            n = k[3:]
            ref, got = torch.from_numpy(fx[k].copy()), net.state_dict()[n].cpu()
            if n in (PRE_B, "decoder.decoder.pre_linear.1.running_mean"):
                assert float((got - ref).abs().max()) <= 1.01 * 2 * lr, n
            elif ref.dtype.is_floating_point:
                err = float((got.double() - ref.double()).abs().max())
                assert err <= 1e-4 * float(ref.abs().max()) + 0.02 * 2 * lr, (n, err)
            else:
                assert torch.equal(got, ref), n
    net.train(False)
    with torch.no_grad():
        out = net(ids, lengths, poses, None)
    assert net.last_route == "per_operator" and out.shape == (B, S, D)
    print(f"{route} eval outputs: {relerr(out, fx['eval/outputs']):.2e}")
    assert relerr(out, fx["eval/outputs"]) < 1e-4
    assert torch.equal(out[:, 0], poses[:, 0])                 # outputs[:, 0] is the seed pose, bit for bit


# ---- 2. the fused kernels against the float64 restatement ------------------------------------------------------------------------
#         (B, H, D, Tw, S1, n_pre, p)
CASES = [(2, 16, 12, 1, 1, 1, 0.0),          # the smallest served shape: one row pair, one word, one step
         (16, 16, 135, 9, 5, 2, 0.2),        # one whole row tile at the pose width
         (17, 20, 135, 9, 5, 2, 0.2),        # row-tile edge, H padded to 32, D % 4 = 3
         (33, 64, 135, 64, 5, 6, 0.0),       # n_pre >= S1: nothing is fed back; Tw at its limit
         (33, 64, 133, 5, 5, 1, 0.2),        # D % 4 = 1, everything fed back
         (24, 200, 135, 12, 3, 1, 0.2)]      # the shipped width: the LDS budget
_CACHE = {}


def _kernel_inputs(case):
    """decoder weights (a fresh BahdanauAttnDecoderRNN with BatchNorm's affine moved off 1 / 0), inputs and the upstream gradient"""
    from gesture2vec_amd.model.seq2seq_net import BahdanauAttnDecoderRNN
    B, H, D, Tw, S1, n_pre, p = case
    torch.manual_seed(100 + B + H + D + Tw)
    dec = BahdanauAttnDecoderRNN(D, H, D, 2, p)
    g = torch.Generator().manual_seed(9)
    with torch.no_grad():
        dec.pre_linear[1].weight.copy_(1.0 + 0.3 * torch.randn(H, generator=g))
        dec.pre_linear[1].bias.copy_(0.2 * torch.randn(H, generator=g))
    h0 = torch.tanh(torch.randn(2, B, H, generator=g))
    enc = torch.tanh(torch.randn(Tw, B, H, generator=g))
    tgt = torch.tanh(torch.randn(S1 + 1, B, D, generator=g))
    gout = torch.randn(S1, B, D, generator=g)
    keep = (torch.rand(S1, B, H, generator=g) < 1 - p).to(torch.uint8) if p > 0 else None
    return dec, h0, enc, tgt, gout, keep


def _reference(case):
    """the float64 restatement and its float32 twin, computed once per case and shared"""
    if case not in _CACHE:
        dec, h0, enc, tgt, gout, keep = _kernel_inputs(case)
        sd = {"decoder.decoder." + k: v for k, v in dec.state_dict().items()}
        n_pre, p = case[5], case[6]
        _CACHE[case] = tuple(R.kernel_case(sd, h0, tgt, enc, gout, n_pre, p, keep, dtype=dt) for dt in (torch.float64, torch.float32))
    return _CACHE[case]


def _fused(case, dec, h0, enc, tgt, gout, keep, defer=True):
    """PoseAttnRollout on the device -> the quantities of R.kernel_case under the same names"""
    from gesture2vec_amd import rollout_t2e as RT
    B, H, D, Tw, S1, n_pre, p = case
    dec.zero_grad()
    h0d, encd = h0.to(DEV).requires_grad_(True), enc.to(DEV).requires_grad_(True)
    bn = dec.pre_linear[1]
    hold = [] if defer else None
    spec = RT.RolloutSpec(tgt.to(DEV), S1, n_pre, 2, True, p, None, None if keep is None else keep.to(DEV), bn.running_mean,
                          bn.running_var, defer_bn=hold)
    calls0 = RT.POSE_FUSED_CALLS
    full, aw = RT.PoseAttnRollout.apply(h0d, encd, dec.attn.project_encoder(encd), spec, *RT.pose_decoder_params(dec))
    assert RT.POSE_FUSED_CALLS == calls0 + 1
    assert torch.equal(full[0], tgt.to(DEV)[0])
    (full[1:] * gout.to(DEV)).sum().backward()
    out = dict(y=full[1:].detach(), attw=aw.detach(), d_hidden0=h0d.grad, d_enc=encd.grad)
    if defer:
        stats = hold[0][0]
        out.update(bn_mean=stats[:, 0].clone(), bn_invstd=stats[:, 1].clone())
    for k, v in dec.named_parameters():
        out["grad/" + k] = v.grad.detach().clone()
    return out


@pytest.mark.parametrize("case", CASES, ids=lambda c: "B%d-H%d-D%d-Tw%d-S%d-npre%d-p%g" % c)
def test_fused_kernels_match_float64_restatement(case):
    """g2v_pose_attn_rollout_fwd / _bwd against the restatement in float64: y, attw, the BatchNorm statistics, d_hidden0, d_enc (context
    and energy paths together: the caller's enc_proj product is part of the graph here) and every weight and bias gradient.
    Bar per quantity: 4 x the distance of the restatement's own float32 run from its float64 run, relative to the quantity's largest
    entry -- measured per case, not chosen in advance.  pre_linear.0.bias feeds BatchNorm: its gradient is zero but for rounding, so
    both its error and its bar are taken relative to the largest entry of pre_linear.0.weight's gradient (the same du summed over the
    same rows).  At one shape the call is repeated: the same input gives the same bits (no float atomics).  The running statistics
    the kernels update in place equal the per-operator route's to 1e-6.

    Measured on an MI355X (worst error / bar per case, in the order of CASES): 0.77, 0.39, 0.65, 0.43, 0.38, 0.39."""
    from gesture2vec_amd import ops
    B, H, D, Tw, S1, n_pre, p = case
    assert ops.pose_attn_rollout_ok(S1, B, H, D, Tw)
    dec, h0, enc, tgt, gout, keep = _kernel_inputs(case)
    ref, f32 = _reference(case)
    dec = dec.to(DEV)
    dec.train(True)
    got = _fused(case, dec, h0, enc, tgt, gout, keep)
    names = ["y", "attw", "bn_mean", "bn_invstd", "d_hidden0", "d_enc"] + sorted(k for k in ref if k.startswith("grad/"))
    assert len(names) == 6 + 17 and all(k in got for k in names)
    wmax = float(ref["grad/pre_linear.0.weight"].abs().max())
    worst, fails = 0.0, []
    for k in names:
        scale = wmax if k == "grad/pre_linear.0.bias" else None
        bar = 4 * relerr(f32[k], ref[k], scale)
        err = relerr(got[k], ref[k], scale)
        ratio = err / bar if bar > 0 else (0.0 if err == 0 else float("inf"))
        worst = max(worst, ratio)
        print(f"  {k:32s} err {err:.2e}  bar {bar:.2e}  ratio {ratio:.2f}")
        if not err <= bar:
            fails.append((k, err, bar))
    print("case", case, "worst error / bar:", f"{worst:.2f}")
    assert not fails, fails
    if case == CASES[2]:
        again = _fused(case, dec, h0, enc, tgt, gout, keep)
        for k in names:
            assert torch.equal(got[k], again[k]), ("not bit-reproducible", k)
    # running statistics: the kernels' in-place updates against the per-operator chain's
    bn = dec.pre_linear[1]
    bn.running_mean.zero_(); bn.running_var.fill_(1.0)
    with torch.no_grad():
        _fused_fwd_only(case, dec, h0, enc, tgt, keep)
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    bn.running_mean.zero_(); bn.running_var.fill_(1.0)
    with torch.no_grad():
        encd, hidden, x, tg = enc.to(DEV), h0.to(DEV), tgt.to(DEV)[0], tgt.to(DEV)
        ep = dec.attn.project_encoder(encd)
        for t in range(S1):
            y, hidden, _ = dec(x, hidden, encd, None, keep_l0=None if keep is None else keep[t].to(DEV).contiguous(), enc_proj=ep)
            x = tg[t + 1] if t + 1 < max(1, n_pre) else y
    print("  running stats:", relerr(rm, bn.running_mean), relerr(rv, bn.running_var))
    assert relerr(rm, bn.running_mean) < 1e-6 and relerr(rv, bn.running_var) < 1e-6
    rm64, rv64 = R.running_stats(ref["stats"], B)
    assert relerr(rm, rm64) < 1e-5 and relerr(rv, rv64) < 1e-5


def _fused_fwd_only(case, dec, h0, enc, tgt, keep):
    from gesture2vec_amd import rollout_t2e as RT
    B, H, D, Tw, S1, n_pre, p = case
    bn = dec.pre_linear[1]
    encd = enc.to(DEV)
    spec = RT.RolloutSpec(tgt.to(DEV), S1, n_pre, 2, True, p, None, None if keep is None else keep.to(DEV), bn.running_mean,
                          bn.running_var, defer_bn=None)
    return RT.PoseAttnRollout.apply(h0.to(DEV), encd, dec.attn.project_encoder(encd), spec, *RT.pose_decoder_params(dec))


# ---- 3. fused against per-operator on the whole model ---------------------------------------------------------------------------
def _model_case(B, H, D, Tw, S, n_pre, p, seed=5):
    from gesture2vec_amd.model.seq2seq_net import Seq2SeqNet
    NW, EMB = 50, 30
    args = _args(H, p, n_pre, S)
    g = torch.Generator().manual_seed(6)
    torch.manual_seed(seed)
    net = Seq2SeqNet(args, D, S, NW, EMB, np.random.RandomState(0).randn(NW, EMB).astype(np.float32), None).to(DEV)
    net.train(True)
    ids = torch.randint(1, NW, (B, Tw), generator=g).to(DEV)
    lengths = torch.sort(torch.randint(3, Tw + 1, (B,), generator=g), descending=True).values
    lengths[0] = Tw
    poses = torch.tanh(torch.randn(B, 1, D, generator=g) + (0.2 * torch.randn(B, S, D, generator=g)).cumsum(1)).to(DEV)
    masks = ((torch.rand(S - 1, B, H, generator=g) < 1 - p).to(torch.uint8).to(DEV) if p > 0 else None,
             (torch.rand(Tw, B, 2 * H, generator=g) < 1 - p).to(torch.uint8).to(DEV) if p > 0 else None)
    return args, net, ids, lengths, poses, masks


def test_fused_route_matches_per_operator_route():
    """one training step each on copies of the same net with the same masks at (B, H, D, Tw, S1, n_pre, p) = (17, 20, 135, 9, 5, 2,
    0.2): loss and every gradient to 1e-5 relative (pre_linear.0.bias relative to pre_linear.0.weight's gradient, as above)."""
    from gesture2vec_amd.flat import FlatClipAdam
    from gesture2vec_amd.train_eval.train_seq2seq import train_iter_seq2seq
    args, net, ids, lengths, poses, masks = _model_case(17, 20, 135, 9, 6, 2, 0.2)
    res = {}
    for route in ("fused", "per_operator"):
        n = copy.deepcopy(net)
        n.route = route
        n.set_dropout_masks(*masks)
        optim = FlatClipAdam(n.parameters(), lr=5e-4, betas=(0.5, 0.999))
        loss = train_iter_seq2seq(args, 1, ids, lengths, poses, n, optim)
        assert n.last_route == route
        bn = n.decoder.decoder.pre_linear[1]
        assert int(bn.num_batches_tracked) == 5
        res[route] = (loss["loss"], {k: v.grad.detach().clone() for k, v in n.named_parameters()}, bn.running_mean.clone(), bn.running_var.clone())
    lf, gf, rmf, rvf = res["fused"]
    lp, gp, rmp, rvp = res["per_operator"]
    print(f"loss fused {lf:.8f} per-operator {lp:.8f} rel {abs(lf - lp) / abs(lp):.2e}")
    fails = []
    if not abs(lf - lp) <= 1e-5 * abs(lp):
        fails.append(("loss", lf, lp))
    wmax = float(gp["decoder.decoder.pre_linear.0.weight"].abs().max())
    for k in gp:
        err = relerr(gf[k], gp[k], wmax if k == PRE_B else None)
        print(f"  grad {k}: {err:.2e}")
        if not err <= 1e-5:
            fails.append((k, err))
    assert not fails, fails
    assert relerr(rmf, rmp) < 1e-6 and relerr(rvf, rvp) < 1e-6


# ---- 4. the feedback gradient ----------------------------------------------------------------------------------------------------
def test_feedback_gradient_is_attached():
    """n_pre = 1: every step past the first reads the previous OUTPUT, so (a) perturbing the targets' slots 2.. leaves the gradient of
    the loss w.r.t. W_out unchanged, to the bit, and (b) the kernels' gradient is the restatement's with the feedback attached --
    detaching it there moves the gradient by far more than the test's bar, so a kernel that quietly detaches cannot pass."""
    case = CASES[4]
    dec, h0, enc, tgt, gout, keep = _kernel_inputs(case)
    ref, f32 = _reference(case)
    sd = {"decoder.decoder." + k: v for k, v in dec.state_dict().items()}
    det = R.kernel_case(sd, h0, tgt, enc, gout, case[5], case[6], keep, detach_feedback=True)
    dec = dec.to(DEV)
    dec.train(True)
    got = _fused(case, dec, h0, enc, tgt, gout, keep)
    tgt2 = tgt.clone()
    tgt2[2:] += 0.5
    got2 = _fused(case, dec, h0, enc, tgt2, gout, keep)
    k = "grad/out.weight"
    assert torch.equal(got[k], got2[k])
    bar = 4 * relerr(f32[k], ref[k])
    gap, err = relerr(det[k], ref[k]), relerr(got[k], ref[k])
    print(f"detached vs attached {gap:.3e}; fused vs attached {err:.2e}; bar {bar:.2e}")
    assert gap > 100 * bar and err <= bar and relerr(got[k], det[k]) > 50 * bar


# ---- 5. refusals before launch ---------------------------------------------------------------------------------------------------
def _raw_forward(B=4, H=16, D=12, Tw=3, S1=2, drop_w_attn=False, misalign_h_init=False, workspace_bytes=None):
    from gesture2vec_amd import ops
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=DEV)
    G = 3 * H
    wd = dict(w_pre=f32(H, D + H), b_pre=f32(H), bn_w=f32(H), bn_b=f32(H), w_ih0=f32(G, H), w_hh0=f32(G, H), b_ih0=f32(G), b_hh0=f32(G),
              w_ih1=f32(G, H), w_hh1=f32(G, H), b_ih1=f32(G), b_hh1=f32(G), w_out=f32(D, H), b_out=f32(D), w_attn=f32(H, 2 * H),
              b_attn=f32(H), v_attn=f32(H))
    if drop_w_attn:
        wd["w_attn"] = None
    y = torch.full((S1, B, D), -7.0, device=DEV)
    sv = dict(ec=f32(S1, B, ops.pose_attn_ldec(H, D)), u=f32(S1, B, H), a=f32(S1, B, H), bn_stats=f32(S1, 2, H), h0=f32(S1 + 1, B, H),
              h1=f32(S1 + 1, B, H), gates0=f32(S1, B, 4 * H), gates1=f32(S1, B, 4 * H), bn_partial=f32(2, (B + 15) // 16, 2, H),
              hp=f32(S1, B, H), attw=f32(S1, B, Tw), logits=y)
    h_init = f32(2 * B * H + 4)[1:1 + 2 * B * H].view(2, B, H) if misalign_h_init else f32(2, B, H)
    ops.pose_attn_rollout_fwd(f32(S1 + 1, B, D), h_init, f32(Tw, B, H), f32(Tw, B, H), wd, sv, None, 0.0, 1, S1, B, H, D, Tw,
                              workspace_bytes=workspace_bytes)
    torch.cuda.synchronize()
    return y


def test_entries_refuse_before_launch():
    from gesture2vec_amd import _lib, ops
    err = _lib.G2VLibraryError
    assert float(_raw_forward().max()) == 0.0                   # the served call writes y (all-zero weights: y = b_out = 0)
    for kw, text in ((dict(drop_w_attn=True), "attention: missing array"), (dict(misalign_h_init=True), "16-byte alignment"),
                     (dict(workspace_bytes=64), "workspace too small"), (dict(Tw=65), "shape not served"),
                     (dict(H=18), "shape not served"), (dict(B=1), "shape not served")):
        with pytest.raises(err, match=text):
            _raw_forward(**kw)
    lib = _lib.load()
    assert lib.g2v_pose_attn_rollout_ok(29, 128, 200, 135, 12) == 1 and lib.g2v_pose_attn_rollout_ok(1, 2, 16, 1, 1) == 1
    assert lib.g2v_pose_attn_rollout_ok(5, 33, 64, 256, 64) == 1
    for bad in ((0, 8, 16, 12, 3), (2, 1, 16, 12, 3), (2, 8, 18, 12, 3), (2, 8, 12, 12, 3), (2, 8, 260, 12, 3), (2, 8, 16, 0, 3),
                (2, 8, 16, 257, 3), (2, 8, 16, 12, 0), (2, 8, 16, 12, 65), (2, 8, 256, 135, 12)):
        assert lib.g2v_pose_attn_rollout_ok(*bad) == 0, bad
    assert lib.g2v_pose_attn_rollout_plan(29, 128, 200, 135, 12, 128) == 1
    assert lib.g2v_pose_attn_rollout_plan(29, 128, 200, 135, 12, 129) == 0
    assert lib.g2v_pose_attn_rollout_plan(29, 128, 18, 135, 12, 1) == 0
    assert ops.pose_attn_rollout_plan(29, 4096, 200, 135, 12, 1 << 40) == 0
    assert lib.g2v_latent_rollout_ok(5, 1024, 200, 400, 1) == 0 and lib.g2v_latent_rollout_ok(5, 1024, 200, 400, 0) == 1


# ---- 6. surface ------------------------------------------------------------------------------------------------------------------
def test_reference_checkpoint_loads_strictly(golden_dir):
    from gesture2vec_amd.model.seq2seq_net import Seq2SeqNet
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import utils.train_utils as tu
    path = os.path.join(golden_dir, "baseline_ckpt.bin")
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert set(ck) == {"args", "epoch", "lang_model", "pose_dim", "gen_dict"}
    a = ck["args"]
    net = Seq2SeqNet(a, ck["pose_dim"], a.n_poses, ck["lang_model"].n_words, ck["lang_model"].word_embedding_weights.shape[1],
                     ck["lang_model"].word_embedding_weights, None)
    net.load_state_dict(ck["gen_dict"], strict=True)
    assert set(net.state_dict()) == set(ck["gen_dict"])
    for k, v in ck["gen_dict"].items():
        assert net.state_dict()[k].shape == v.shape, k
    for k in ("encoder.embedding.weight", "decoder.decoder.pre_linear.0.weight", "decoder.decoder.pre_linear.1.running_var",
              "decoder.decoder.attn.attn.weight", "decoder.decoder.attn.attn.bias", "decoder.decoder.attn.v",
              "decoder.decoder.gru.weight_ih_l1", "decoder.decoder.out.weight", "decoder.decoder.out.bias"):
        assert k in ck["gen_dict"], k
    args2, net2, loss_fn, lang, dim = tu.load_checkpoint_and_model(path, DEV, "baseline")
    assert isinstance(net2, Seq2SeqNet) and not net2.training and dim == ck["pose_dim"] and callable(loss_fn)
    for k, v in ck["gen_dict"].items():
        assert torch.equal(net2.state_dict()[k].cpu(), v), k


def test_trainer_script_trains_on_synthetic_clips(tmp_path):
    out = str(tmp_path / "run")
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "train.py"), "--config=" + os.path.join(ROOT, "config", "baseline_synthetic.yml"),
           "--synthetic", "--synthetic_batches", "4", "--batch_size", "16", "--hidden_size", "32", "--n_poses", "8", "--n_pre_poses", "3",
           "--epochs", "2", "--save_every", "2", "--model_save_path", out, "--name", "b"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=170)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-3000:]
    ep = [ln for ln in log.splitlines() if "EP " in ln and "samples/s | loss:" in ln]
    val = [ln for ln in log.splitlines() if "[VAL] loss:" in ln]
    assert len(val) == 2 and len(ep) >= 2, log[-3000:]
    mean = lambda e: float(np.mean([float(ln.split("loss:")[1].split(",")[0]) for ln in ep if f"EP {e} " in ln]))
    first, last = mean(1), mean(2)               # (the same four batches every epoch)
    assert np.isfinite(first) and last < first, (first, last)
    ck = torch.load(os.path.join(out, "b_checkpoint_002.bin"), map_location="cpu", weights_only=False)
    assert set(ck) == {"args", "epoch", "lang_model", "pose_dim", "gen_dict"} and ck["epoch"] == 2 and ck["pose_dim"] == 135
    assert ck["gen_dict"]["decoder.decoder.pre_linear.0.weight"].shape == (32, 135 + 32)


def test_unbuilt_options_are_refused_by_name():
    from gesture2vec_amd.model.seq2seq_net import BahdanauAttnDecoderRNN, Generator, Seq2SeqNet
    args = _args(16, 0.0, 1, 4)
    spk = argparse.Namespace(n_words=3)
    with pytest.raises(NotImplementedError, match="speaker_model"):
        Seq2SeqNet(args, 12, 4, 20, 8, None, speaker_model=spk)
    with pytest.raises(NotImplementedError, match="speaker_model"):
        BahdanauAttnDecoderRNN(12, 16, 12, 2, 0.0, speaker_model=spk)
    with pytest.raises(NotImplementedError, match="discrete_representation"):
        Generator(args, 12, discrete_representation=True)
    gen = Generator(args, 12).to(DEV)
    with pytest.raises(NotImplementedError, match="z is not None"):
        gen(torch.zeros(2, 3, device=DEV), torch.zeros(2, 12, device=DEV), torch.zeros(2, 2, 16, device=DEV), torch.zeros(3, 2, 16, device=DEV))
