"""Gesture generation on the device (gesture2vec_amd/generate.py, csrc/dec_chain.hip) against the float64 restatements of
tests/_dec_chain_ref.py.

* The chain on both routes -- "chain" (g2v_dec_chain_fwd, one launch) and "rollout" (one eval-mode g2v_dec_rollout_fwd per chunk)
  -- and, on the first two shapes, the step API loop (net.decoder(...) with set_step_masks), each compared with float64 per chunk
  and step on `out` and on the last hidden state: e_kernel <= min(8 max(e32, 2u), cap), everything from the restatement alone (the
  rule of tests/test_gpu_dec_rollout_f64.py).  Cases (CASES of the restatement module): the smallest shapes at which the kernel
  can still go wrong -- one clip, a 135 x 64 net, two workgroups with a ragged second one at H = 200, D = 65 off every vector
  width, a teacher-forced prefix, an unconditioned decoder, ids that hit rows 0 and R - 1 and repeat a row, no ids, no start
  frame, and a call whose arrays all start 4 bytes (masks: 1 byte, ids: 8 bytes -- an int64's own alignment) past a 16-byte
  boundary.  H = 64, D = 135 runs the register-resident variant of the kernel (one ragged workgroup, and two), every
  other shape the streamed one.
* What holds because rows do not interact: the same call twice gives the same bits; clips 3..4 of the 17-clip case decoded alone
  give the bits they had in the batch.
* g2v_clip_finish against its float64 restatement under the same bar: blend, blend + un-normalise, blend + un-normalise + filter.
* The API: decode_codes, decode_latents(chunk_latents(...)), reconstruct_clips on a tiny VQ net and a plain net against the
  restatement fed the same rows; codebook_gestures' shape; text_to_codes against direct model calls.

Largest e_kernel / max(e32, 2u) on the MI355X per route over all cases (the quantity the margin of 8 multiplies):
  chain    out 2.22  h_last 1.50        rollout  out 3.71  h_last 2.09        step API  out 2.15  h_last 1.14
  clip_finish  1.00 (blend)  0.78 (blend + un-normalise)  2.15 (blend + un-normalise + filter)
  API level    2.31 (decode_codes, "rollout")  1.98 ("chain")  2.04 (decode_latents)  0.52 (reconstruct_clips)"""
import argparse

import numpy as np
import pytest
import torch

import _dec_chain_ref as CR
import _dec_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WEIGHTS = {
    "w_pre": "pre_linear.0.weight", "b_pre": "pre_linear.0.bias", "bn_w": "pre_linear.1.weight", "bn_b": "pre_linear.1.bias",
    "bn_running_mean": "pre_linear.1.running_mean", "bn_running_var": "pre_linear.1.running_var",
    "w_ih0": "gru.weight_ih_l0", "w_hh0": "gru.weight_hh_l0", "b_ih0": "gru.bias_ih_l0", "b_hh0": "gru.bias_hh_l0",
    "w_ih1": "gru.weight_ih_l1", "w_hh1": "gru.weight_hh_l1", "b_ih1": "gru.bias_ih_l1", "b_hh1": "gru.bias_hh_l1",
    "w_out": "out_layer.weight", "b_out": "out_layer.bias",
}


@pytest.fixture(scope="module")
def G():
    from gesture2vec_amd import _lib, generate
    assert _lib.load().g2v_device_ok() == 1, "no gfx950 device visible"
    return generate


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else t.dtype)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _put(src, unaligned):
    """a device copy, 16-byte aligned as torch hands it out, or one element past such a boundary (float32: 4 bytes, uint8: 1 byte,
    int64: 8 bytes)"""
    if src is None:
        return None
    off = 1 if unaligned else 0
    t = torch.zeros((src.numel() + off,), dtype=src.dtype, device=DEV)[off:].view(*src.shape)
    t.copy_(src)
    assert t.is_contiguous() and (t.data_ptr() % 16 != 0) == bool(off)
    return t


def _device_call(inp, clips=None):
    u = inp["unaligned"]
    sl = slice(0, inp["B"]) if clips is None else clips
    ids = inp["ids"]
    rows = inp["rows"]
    if ids is None and clips is not None:      # the slice's rows, renumbered
        C = inp["C"]
        rows = rows.view(inp["B"], C, -1)[sl].reshape(-1, rows.shape[1])
    return dict(rows=_put(rows, u), ids=_put(None if ids is None else ids[sl].contiguous(), u),
                start=_put(None if inp["start_t"] is None else inp["start_t"][sl].contiguous(), u),
                teacher=_put(None if inp["teacher_t"] is None else inp["teacher_t"][sl].contiguous(), u),
                keep95=_put(inp["keep95"][:, :, sl].contiguous(), u),
                weights={k: _put(inp["sd"][R.PRE + v], u) for k, v in WEIGHTS.items()})


def _run(G, route, inp, d, B=None):
    fn = G.dec_chain_fwd if route == "chain" else G._rollout_route
    B = inp["B"] if B is None else B
    out, h = fn(d["rows"], d["ids"], d["start"], d["teacher"], d["keep95"], d["weights"], inp["n_pre"] if inp["teacher"] else 1,
                inp["conditioned"], inp["C"], inp["T"], inp["W"], B, inp["D"], inp["H"], True)
    torch.cuda.synchronize()
    return out, h


@pytest.mark.parametrize("route", ["chain", "rollout"])
@pytest.mark.parametrize("case", CR.CASES, ids=lambda c: c["id"])
def test_chain_matches_float64(G, case, route):
    ref = CR.reference(case)
    inp, f64, e32 = ref["inp"], ref["f64"], ref["e32"]
    assert G.chain_ok(case["C"], case["T"], case["W"], case["B"], case["D"], case["H"])
    d = _device_call(inp)
    out, h = _run(G, route, inp, d)
    assert out.shape == (case["B"], case["C"] * case["T"], case["D"]) and h.shape == (2, case["B"], case["H"])
    assert not torch.isnan(out).any() and not torch.isnan(h).any()
    label = f"{route} {case['id']}"
    ok1, line1, _ = CR.check(label, "out", out.cpu(), f64["out"], e32["out"])
    ok2, line2, _ = CR.check(label, "h_last", h.cpu(), f64["h_last"], e32["h_last"])
    assert ok1 and ok2, line1 + "\n" + line2
    if inp["start_t"] is not None:
        assert _same(out[:, 0].cpu(), inp["start_t"]), "frame 0 is the start frame, bit for bit"
    out2, h2 = _run(G, route, inp, d)
    assert _same(out, out2) and _same(h, h2), "the same call twice gives other bits"


def test_clips_decoded_alone_keep_their_bits(G):
    case = CR.CASES[2]
    assert case["B"] == 17
    inp = CR.reference(case)["inp"]
    out, h = _run(G, "chain", inp, _device_call(inp))
    part, hp = _run(G, "chain", inp, _device_call(inp, clips=slice(3, 5)), B=2)
    assert _same(out[3:5], part) and _same(h[:, 3:5], hp)


def _net(D, H, T, sd, *, vq=True, n_pre=1, conditioned=True):
    from gesture2vec_amd.model.Autoencoder_VQVAE_model import Autoencoder_VQVAE
    args = argparse.Namespace(rep_learning_dim=D, hidden_size=H, n_layers=2, dropout_prob=0.0, autoencoder_vae="False",
                              autoencoder_vq="True" if vq else "False", autoencoder_vq_components=8, autoencoder_vq_commitment_cost=0.25,
                              n_pre_poses=n_pre, autoencoder_conditioned="True" if conditioned else "False", autoencoder_att="False",
                              autoencoder_fixed_weight="False", n_poses=T, loss_l1_weight=5.0, loss_cont_weight=0.1,
                              loss_var_weight=0.5, learning_rate=5e-4, epochs=10)
    net = Autoencoder_VQVAE(args, D, T)
    net.load_state_dict({k: v for k, v in sd.items() if vq or not k.startswith("vq_layer.")}, strict=True)
    return net.to(DEV).eval()


@pytest.mark.parametrize("case", CR.STEP_API_CASES, ids=lambda c: c["id"])
def test_step_api_loop_matches_float64(G, case):
    """what a user had to write before: net.decoder(...) one step at a time"""
    ref = CR.reference(case)
    inp, f64, e32 = ref["inp"], ref["f64"], ref["e32"]
    C, T, W, B, D, H = (case[k] for k in ("C", "T", "W", "B", "D", "H"))
    net = _net(D, H, T, inp["sd"])
    k95 = inp["keep95"].to(DEV)
    rows = inp["rows"].to(DEV)
    ids = inp["ids"] if inp["ids"] is not None else torch.arange(B * C).view(B, C)
    net.decoder.decoder.set_step_masks([k95[c, s].contiguous() for c in range(C) for s in range(W + T - 1)])
    frames, x = [], inp["start_t"].to(DEV)
    with torch.no_grad():
        for c in range(C):
            hidden = rows[ids[:, c].to(DEV)].view(B, 2, H).transpose(0, 1).contiguous()
            frames.append(x)
            for _ in range(W):
                _, hidden, _ = net.decoder(None, x, hidden, None, None)
            for t in range(1, T):
                x, hidden, _ = net.decoder(None, x, hidden, None, None)
                frames.append(x)
    out = torch.stack(frames, 1)
    label = f"step-api {case['id']}"
    ok1, line1, _ = CR.check(label, "out", out.cpu(), f64["out"], e32["out"])
    ok2, line2, _ = CR.check(label, "h_last", hidden.cpu(), f64["h_last"], e32["h_last"])
    assert ok1 and ok2, line1 + "\n" + line2


# ---------------------------------------------------------------------------------------------------------------- the clip's tail
@pytest.mark.parametrize("mode", CR.FINISH_MODES)
@pytest.mark.parametrize("shape", CR.FINISH_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_clip_finish_matches_float64(G, shape, mode):
    B, C, T, Dr = shape
    r, mean, std = CR.finish_inputs(B, C, T, Dr)
    unnorm, smooth = "unnorm" in mode, "savgol" in mode
    table = CR.savgol_table() if smooth else None
    m, s = (mean, std) if unnorm else (None, None)
    f64 = CR.clip_finish(r, m, s, T, 10, table, torch.float64)
    f32 = CR.clip_finish(r, m, s, T, 10, None if table is None else table.astype(np.float32), torch.float32)
    e32 = R.step_err(CR.by_step(f32), CR.by_step(f64), "y")
    got = G.clip_finish(r.to(DEV), m, s, n_poses=T, blend=10, smooth="savgol" if smooth else None)
    torch.cuda.synchronize()
    assert got.shape == r.shape and not torch.isnan(got).any()
    ok, line, _ = CR.check(f"clip_finish {mode} {shape}", "out", got.cpu(), f64, e32)
    assert ok, line
    with pytest.raises(ValueError):
        G.clip_finish(torch.zeros(1, 36, 4, device=DEV), n_poses=18, blend=10)
    with pytest.raises(ValueError):
        G.clip_finish(torch.zeros(1, 24, 4, device=DEV), n_poses=24, blend=0, smooth="savgol")


# ---------------------------------------------------------------------------------------------------------------------- the API
def _api_inp(net, rows, ids, start, teacher, keep95, C, B, W=5):
    """the restatement's inputs from what an API call was given (CPU copies)"""
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    cpu = lambda t: None if t is None else t.detach().cpu()
    return dict(C=C, T=net.n_frames, W=W, B=B, D=net.pose_dim, H=net.hidden_size, sd=sd, rows=cpu(rows), ids=cpu(ids),
                start_t=cpu(start), teacher_t=cpu(teacher), keep95=cpu(keep95), n_pre=net.n_pre_poses,
                conditioned=net.autoencoder_conditioned)


def _held(label, got, inp, post=lambda x, dt: x):
    f64, f32 = post(CR.chain(inp, torch.float64)["out"], torch.float64), post(CR.chain(inp, torch.float32)["out"], torch.float32)
    e32 = R.step_err(CR.by_step(f32), CR.by_step(f64), "y")
    ok, line, _ = CR.check(label, "out", got.cpu(), f64, e32)
    assert ok, line


@pytest.mark.parametrize("vq", [True, False], ids=["vq", "plain"])
def test_api_against_the_restatement(G, vq):
    from gesture2vec_amd.kmeans import KMeans
    from gesture2vec_amd.pipeline import chunk_latents
    D, H, T, B, C, W = 5, 8, 4, 3, 2, 5
    sd = R.inputs(2, 1, D, H, 0.0, 41, training=False)["sd"]
    net = _net(D, H, T, sd, vq=vq, n_pre=2)
    g = torch.Generator().manual_seed(77)
    keep95 = (torch.rand(C, W + T - 1, B, D, generator=g) < CR.KEEP_PROB).to(torch.uint8).to(DEV)
    start = torch.randn(B, D, generator=g).to(DEV)
    # ---- codes: the codebook's rows, or a k-means model's centres ----
    codes = torch.tensor([[0, 7], [3, 3], [7, 1]], dtype=torch.int64, device=DEV)
    if vq:
        rows, km = net.vq_layer._embedding.weight.detach(), None
    else:
        km = KMeans.from_centers(torch.randn(8, 2 * H, generator=g).numpy())
        rows = torch.from_numpy(np.asarray(km.cluster_centers_, dtype=np.float32)).to(DEV)
    for route in ("chain", "rollout", "auto"):
        got = G.decode_codes(net, codes, kmeans=km, start=start, keep95=keep95, route=route)
        assert got.shape == (B, C * T, D)
        _held(f"decode_codes {route}", got, _api_inp(net, rows, codes, start, None, keep95, C, B))
    with pytest.raises(IndexError):
        G.decode_codes(net, torch.tensor([[0, 8]], dtype=torch.int64, device=DEV), kmeans=km)
    assert not net.training
    net.train(True)
    G.decode_codes(net, codes, kmeans=km)              # masks drawn from net.rng_seed; the mode comes back
    assert net.training
    net.eval()
    # ---- latents: the rows chunk_latents returns ----
    x = torch.randn(B * C, T, D, generator=g).to(DEV)
    lat = chunk_latents(net, x)
    got = G.decode_latents(net, lat.view(B, C, -1), start=start, keep95=keep95, route="chain")
    _held("decode_latents", got, _api_inp(net, lat, None, start, None, keep95, C, B))
    # ---- a whole clip, identity DAE: (C + 1) T frames hold C chunks (the trailing full chunk is dropped, as in the reference) ----
    poses = torch.randn(B, (C + 1) * T, D, generator=g)
    mean, std = torch.randn(D, generator=g).numpy(), (torch.rand(D, generator=g) + 0.2).numpy()
    got = G.reconstruct_clips(None, net, poses.to(DEV), mean, std, blend=2, keep95=keep95, route="chain")
    assert got.shape == (B, C * T, D)
    enc = ((poses - torch.from_numpy(mean)) / torch.from_numpy(np.clip(std, 0.01, None))).float()
    chunks = enc[:, :C * T].reshape(B, C, T, D)
    lat = chunk_latents(net, chunks.reshape(B * C, T, D).to(DEV))
    if vq:
        rows, ids = net.vq_layer._embedding.weight.detach(), net.vq_layer.assign(lat).view(B, C)
    else:
        rows, ids = lat, None
    post = lambda fr, dt: CR.clip_finish(fr, torch.from_numpy(mean), torch.from_numpy(std), T, 2, None, dt)
    _held("reconstruct_clips", got, _api_inp(net, rows, ids, enc[:, 0], chunks, keep95, C, B), post)
    # ---- one gesture per code ----
    cb = G.codebook_gestures(net, None, mean, std, kmeans=km)
    assert cb.shape == (8, T, D) and not torch.isnan(cb).any()


def test_text_to_codes_is_the_reference_loop(G):
    from gesture2vec_amd import ops
    from gesture2vec_amd.model.text2embedding_model import text2embedding_model
    torch.manual_seed(0)
    B, Tw, S, H, L, K, NW, EMB = 4, 7, 3, 32, 2, 64, 50, 300
    args = argparse.Namespace(hidden_size=H, n_layers=L, dropout_prob=0.1, autoencoder_vq_components=K, autoencoder_att="False",
                              n_pre_poses=2, n_poses=20, sentence_frame_length=20 * S, text2_embedding_discrete="True")
    net = text2embedding_model(args, 135, 20, NW, EMB, np.random.RandomState(0).randn(NW, EMB).astype(np.float32), None).to(DEV)
    lengths = torch.tensor([Tw, 6, 4, 3])
    windows = []
    for _ in range(2):
        ids = torch.zeros(B, Tw, dtype=torch.int64)
        for b in range(B):
            ids[b, : lengths[b]] = torch.randint(4, NW, (int(lengths[b]),))
        windows.append((ids.to(DEV), lengths))
    net.train(True)
    got = G.text_to_codes(net, windows)
    assert net.training and got.shape == (B, 2 * S) and got.dtype == torch.int64
    net.eval()
    with torch.no_grad():
        pre = torch.zeros(B, S, dtype=torch.int64, device=DEV)
        lg, _ = net(windows[0][0], lengths, None, pre, None, None)
        best0 = lg.argmax(2)
        pre = pre.clone()
        pre[:, :2] = best0[:, S - 2:]
        lg, _ = net(windows[1][0], lengths, None, pre, None, best0[:, -1].contiguous())
        best1 = lg.argmax(2)
    assert torch.equal(got, torch.cat([best0, best1], 1))
