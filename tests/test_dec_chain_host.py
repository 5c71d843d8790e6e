"""No GPU: the restatements the generation tests are judged by (tests/_dec_chain_ref.py) against literal forms of the reference,
the host answers of g2v_dec_chain_ok / g2v_dec_chain_workspace, and the refusals of gesture2vec_amd.generate.

* the float64 chain against the reference's loop (inference_Autoencoder.py:207-231) written with torch.nn.GRU, BatchNorm1d in
  eval mode and Linear in float64, the Dropout(0.95) masks injected: within 1e-12;
* the blend against the reference's in-place loop at T = 19 and 20, and its refusal below 19;
* the Savitzky-Golay tables against scipy.signal.savgol_filter(x, 25, 5, axis=0), recorded in tests/golden/clip_finish.npz
  (and live where scipy imports)."""
import argparse
import os

import numpy as np
import pytest
import torch

import _dec_chain_ref as CR
import _dec_ref as R


def _module_loop(inp):
    """the reference's loop on modules, float64, batch of clips at once"""
    C, T, W, B, D, H = (inp[k] for k in ("C", "T", "W", "B", "D", "H"))
    sd = {k: inp["sd"][R.PRE + k].double() for k in R.PARAMS}
    lin, bn, gru, out_layer = torch.nn.Linear(D, H), torch.nn.BatchNorm1d(H), torch.nn.GRU(H, H, 2), torch.nn.Linear(H, D)
    for m in (lin, bn, gru, out_layer):
        m.double()
    with torch.no_grad():
        lin.weight.copy_(sd["pre_linear.0.weight"]); lin.bias.copy_(sd["pre_linear.0.bias"])
        bn.weight.copy_(sd["pre_linear.1.weight"]); bn.bias.copy_(sd["pre_linear.1.bias"])
        bn.running_mean.copy_(inp["sd"][R.PRE + "pre_linear.1.running_mean"]); bn.running_var.copy_(inp["sd"][R.PRE + "pre_linear.1.running_var"])
        for name in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0", "weight_ih_l1", "weight_hh_l1", "bias_ih_l1", "bias_hh_l1"):
            getattr(gru, name).copy_(sd["gru." + name])
        out_layer.weight.copy_(sd["out_layer.weight"]); out_layer.bias.copy_(sd["out_layer.bias"])
    for m in (lin, bn, gru, out_layer):
        m.eval()
    masks = inp["keep95"].double()

    def decoder(x, hidden, keep):                      # BahdanauAttnDecoderRNN.forward without attention
        if not inp["conditioned"]:
            x = torch.zeros_like(x)
        x = keep * x / 0.05                            # nn.Dropout(0.95), active in eval too, its mask injected
        x = torch.relu(bn(lin(x)))
        o, hidden = gru(x.unsqueeze(0), hidden)
        return out_layer(o.squeeze(0)), hidden

    ids = inp["ids"] if inp["ids"] is not None else torch.arange(B * C).view(B, C)
    teacher = None if inp["teacher_t"] is None else inp["teacher_t"].double()
    frames, decoder_input = [], None
    with torch.no_grad():
        for c in range(C):
            hidden = inp["rows"].double()[ids[:, c]].reshape(B, 2, H).transpose(0, 1).contiguous()      # reshape(n_layers, 1, H) per clip
            rec = torch.zeros(T, B, D, dtype=torch.float64)
            if decoder_input is None:
                decoder_input = inp["start_t"].double() if inp["start_t"] is not None else torch.zeros(B, D, dtype=torch.float64)
            rec[0] = decoder_input
            for rep in range(W):
                _, hidden = decoder(decoder_input, hidden, masks[c, rep])
            for t in range(1, T):
                if not inp["conditioned"]:
                    decoder_input = torch.zeros_like(decoder_input)
                y, hidden = decoder(decoder_input, hidden, masks[c, W + t - 1])
                rec[t] = y
                decoder_input = teacher[:, c, t] if (teacher is not None and t < inp["n_pre"]) else y
                if not inp["conditioned"]:
                    decoder_input = torch.zeros_like(decoder_input)
            frames.append(rec.transpose(0, 1))
    return torch.cat(frames, 1), hidden


@pytest.mark.parametrize("c", [CR.CASES[4], CR.case(2, 4, 1, 3, 5, 8, seed=15, ids="random", teacher=True, n_pre=2, conditioned=False,
                                                    tag="teacher-unconditioned")], ids=lambda c: c["id"])
def test_float64_chain_is_the_reference_loop(c):
    inp = CR.inputs(c)
    got = CR.chain(inp, torch.float64)
    want_out, want_h = _module_loop(inp)
    assert got["out"].shape == want_out.shape == (c["B"], c["C"] * c["T"], c["D"])
    scale = float(want_out.abs().max())
    assert float((got["out"] - want_out).abs().max()) <= 1e-12 * scale
    assert float((got["h_last"] - want_h).abs().max()) <= 1e-12 * float(want_h.abs().max())


def test_every_case_meets_the_mask_condition_and_a_slice_is_the_batch():
    for c in CR.CASES:
        inp = CR.inputs(c)                             # (asserts the condition on the masks)
        assert inp["keep95"].shape == (c["C"], c["W"] + c["T"] - 1, c["B"], c["D"])
    inp = CR.inputs(CR.CASES[2])
    whole, part = CR.chain(inp, torch.float64), CR.chain(inp, torch.float64, clips=slice(3, 5))
    # (to rounding only: a host matrix product may block a 2-row batch differently from a 17-row one; the kernel's bits are
    #  held equal on the device, tests/test_gpu_dec_chain.py)
    assert float((whole["out"][3:5] - part["out"]).abs().max()) <= 1e-13 * float(whole["out"].abs().max())
    assert float((whole["h_last"][:, 3:5] - part["h_last"]).abs().max()) <= 1e-13


@pytest.mark.parametrize("T", [19, 20])
def test_blend_is_the_reference_in_place_loop(T):
    g = torch.Generator().manual_seed(T)
    r = torch.randn(2, 3 * T, 6, generator=g, dtype=torch.float64)
    got = CR.clip_finish(r, None, None, T, 10, None, torch.float64)
    for b in range(2):
        assert float((got[b] - CR.blend_inplace(r[b], T, 10)).abs().max()) <= 1e-15
    # ... and below 2 n - 1 the two differ: the in-place loop reads frames the previous boundary already blended
    r18 = torch.randn(1, 3 * 18, 6, generator=g, dtype=torch.float64)
    assert float((CR.clip_finish(r18, None, None, 18, 10, None, torch.float64)[0] - CR.blend_inplace(r18[0], 18, 10)).abs().max()) > 1e-3


def test_blend_and_filter_refusals():
    from gesture2vec_amd import generate as G

    class _Cuda:                                       # shapes and flags only: the refusals come before any launch
        is_cuda = True

        def __init__(self, *shape):
            self.shape = shape

        def dim(self):
            return len(self.shape)

    with pytest.raises(ValueError, match="19"):
        G.clip_finish(_Cuda(1, 36, 4), n_poses=18, blend=10)
    with pytest.raises(ValueError, match="25"):
        G.clip_finish(_Cuda(1, 24, 4), n_poses=24, blend=0, smooth="savgol")
    with pytest.raises(ValueError, match="smooth"):
        G.clip_finish(_Cuda(1, 40, 4), n_poses=20, smooth="gauss")


def test_savgol_tables_match_scipy(golden_dir):
    from gesture2vec_amd import generate as G
    fx = np.load(os.path.join(golden_dir, "clip_finish.npz"))
    x, y = fx["x"], fx["y"]
    table = G.savgol_table()
    assert table.shape == (25 + 2 * 12 * 25,) and table.dtype == np.float64
    assert np.array_equal(table, CR.savgol_table())
    got = CR.clip_finish(torch.from_numpy(x)[None], None, None, x.shape[0], 0, table, torch.float64)[0].numpy()
    assert np.abs(got - y).max() <= 1e-12 * np.abs(y).max()
    try:
        from scipy.signal import savgol_filter
    except ImportError:
        return
    x2 = np.random.RandomState(5).standard_normal((25, 3))                 # the shortest clip: both edges meet
    got2 = CR.clip_finish(torch.from_numpy(x2)[None], None, None, 25, 0, table, torch.float64)[0].numpy()
    assert np.abs(got2 - savgol_filter(x2, 25, 5, axis=0)).max() <= 1e-12 * np.abs(x2).max()
    assert np.abs(got - savgol_filter(x, 25, 5, axis=0)).max() <= 1e-12 * np.abs(y).max()


def test_chain_ok_and_workspace_answers():
    from gesture2vec_amd import _lib
    lib = _lib.load()
    ok = lib.g2v_dec_chain_ok
    for c in CR.CASES:
        assert ok(c["C"], c["T"], c["W"], c["B"], c["D"], c["H"]) == 1
    assert ok(60, 34, 5, 1, 135, 64) == 1 and ok(6, 20, 5, 4096, 40, 200) == 1 and ok(1, 2, 0, 1, 1, 1) == 1
    assert ok(2, 20, 5, 8, 256, 256) == 1
    for bad in ((0, 20, 5, 8, 40, 200), (2, 1, 5, 8, 40, 200), (2, 20, -1, 8, 40, 200), (2, 20, 5, 0, 40, 200), (2, 20, 5, 8, 0, 200),
                (2, 20, 5, 8, 257, 200), (2, 20, 5, 8, 40, 0), (2, 20, 5, 8, 40, 257), (2, 20, 5, 8, 40, 400)):
        assert ok(*bad) == 0, bad
    ws = lib.g2v_dec_chain_workspace
    assert ws(40, 257) == 0 and ws(0, 64) == 0

    def floats(D, H):                                  # fragment-major packs (256 floats per 16 x 16 block) + the bias vectors;
        r64 = lambda n: (n + 63) // 64 * 64            # out_layer and its bias padded to a multiple of 12 tiles
        th, td = (H + 15) // 16, (D + 15) // 16
        to = (td + 11) // 12 * 12
        return th * td * 256 + to * th * 256 + 4 * 3 * th * th * 256 + r64(H) + 4 * r64(3 * H) + r64(16 * to)

    for D, H in ((135, 64), (40, 200), (5, 8), (65, 200)):
        assert ws(D, H) == 4 * floats(D, H), (D, H)


def _args(att="False", vq="True", layers=2):
    return argparse.Namespace(rep_learning_dim=5, hidden_size=8, n_layers=layers, dropout_prob=0.0, autoencoder_vae="False",
                              autoencoder_vq=vq, autoencoder_vq_components=6, autoencoder_vq_commitment_cost=0.25, n_pre_poses=1,
                              autoencoder_conditioned="True", autoencoder_att=att, autoencoder_fixed_weight="False", n_poses=4,
                              loss_l1_weight=5.0, loss_cont_weight=0.1, loss_var_weight=0.5, learning_rate=5e-4, epochs=10)


def test_python_refusals():
    from gesture2vec_amd import generate as G
    from gesture2vec_amd.model.Autoencoder_VQVAE_model import Autoencoder_VQVAE
    rows, codes = torch.zeros(6, 16), torch.zeros(2, 3, dtype=torch.int64)
    with pytest.raises(NotImplementedError, match="attention"):
        G.decode_chunks(Autoencoder_VQVAE(_args(att="True"), 5, 4), rows, chunks=3)
    with pytest.raises(NotImplementedError, match="n_layers"):
        G.decode_chunks(Autoencoder_VQVAE(_args(layers=1), 5, 4), torch.zeros(6, 8), chunks=3)
    net = Autoencoder_VQVAE(_args(), 5, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        G.decode_chunks(net, rows, chunks=3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        G.decode_codes(net, codes)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        G.decode_latents(net, torch.zeros(2, 3, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        G.finish_clips(None, torch.zeros(1, 8, 5), None, None, n_poses=4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        G.reconstruct_clips(None, net, torch.zeros(1, 12, 5), None, None)
    with pytest.raises(ValueError, match="route"):
        G.decode_chunks(net, rows, chunks=3, route="fast")
    for bad in ([[0, 6]], [[-1, 0]]):
        with pytest.raises(IndexError):
            G.check_ids(torch.tensor(bad), 6)
    G.check_ids(torch.tensor([[0, 5]]), 6)
    plain = Autoencoder_VQVAE(_args(vq="False"), 5, 4)
    with pytest.raises(ValueError, match="no quantiser"):
        G.decode_codes(plain, codes)
    with pytest.raises(ValueError, match="no quantiser"):
        G.codebook_gestures(plain)
    assert set(G.AUTO_CHAIN_MIN_CLIPS) == {"resident", "streamed"} and all(v >= 1 for v in G.AUTO_CHAIN_MIN_CLIPS.values())
