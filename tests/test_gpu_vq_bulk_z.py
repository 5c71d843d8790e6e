"""Bulk code assignment from raw latents at the checkpoints' width (E = 400): g2v_vq_assign_bulk_z must return, bit for bit, what
the current route returns (linear_fwd + vq_assign at the same N) -- ties, near-ties and non-finite rows included."""
import argparse
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E = 400


def _operands(K, N, kind, seed):
    g = torch.Generator().manual_seed(seed)
    bound = 1.0 / E ** 0.5                                   # nn.Linear's init
    Wp = (torch.rand(E, E, generator=g, dtype=torch.float64) * 2 - 1) * bound
    b = (torch.rand(E, generator=g, dtype=torch.float64) * 2 - 1) * bound
    W = torch.randn(K, E, generator=g, dtype=torch.float64)
    if kind == "small":
        W *= 0.05
    elif kind == "trained":                                  # EMA-trained: live codes near the data, a block of dead codes far out
        W *= 0.05
        W[K // 4:K // 4 + 40] *= 300.0
    elif kind == "dup":                                      # an exact tie: code 300 repeats code 7
        W *= 0.05
        W[300] = W[7]
    z = torch.randn(N, E, generator=g, dtype=torch.float64) * 0.5
    # planted rows, built in float64 and rounded: projections ON a code, at the MIDPOINT of two codes, NaN and Inf rows
    Wp_f, b_f, W_f = Wp.float().double(), b.float().double(), W.float().double()
    pos = torch.randperm(N, generator=g)[:72]
    on, mid = pos[:24], pos[24:64]
    codes = torch.randint(0, K // 4 - 1, (64,), generator=g)       # live codes (and their neighbours) in every kind
    codes[:4] = 7                                            # (the duplicated code of "dup")
    tgt_on = W_f[codes[:24]]
    tgt_mid = 0.5 * (W_f[codes[24:64]] + W_f[codes[24:64] + 1])
    z[on] = torch.linalg.solve(Wp_f, (tgt_on - b_f).T).T
    z[mid] = torch.linalg.solve(Wp_f, (tgt_mid - b_f).T).T
    z[pos[64]] = float("nan")
    z[pos[65], 3] = float("nan")
    z[pos[66]] = float("inf")
    z[pos[67], 10] = -float("inf")
    n_must = 40 + 4                                          # midpoints and non-finite rows cannot be decided by the screen
    return (z.float().to(DEV), Wp.float().to(DEV), b.float().to(DEV), W.float().to(DEV), n_must)


def _current_route(ops, z, Wp, b, W):
    flat = ops.linear_fwd(z, Wp, b)
    return ops.vq_assign(flat, None, W, ops.vq_code_sqnorm(W), want_quantized=False)[0]


CASES = [(K, N, kind) for K in (512, 400) for N in (2048 + 5, 20000 + 37, 2 ** 17 + 37)
         for kind in ("normal", "small", "trained", "dup")] + [(512, 2 ** 20, "normal"), (400, 2 ** 20, "trained")]


@pytest.mark.parametrize("K,N,kind", CASES)
def test_bitwise_equal_to_the_current_route(K, N, kind):
    from gesture2vec_amd import ops
    z, Wp, b, W, n_must = _operands(K, N, kind, seed=K + N)
    assert ops.vq_assign_bulk_z_ok(N, E, K)
    assert ops.vq_route("RAW", "IDX_BULK", N, E, K, facts=("ENTRY",)) == "BULK_Z"
    assert ops.vq_route("RAW", "IDX", N, E, K) == f"PROJECT>PACKED*{4 if N >= 32768 else 2 if N >= 8192 else 1}"      # (the current route)
    idx, und = ops.vq_assign_bulk_z(z, Wp, b, W, ops.vq_code_sqnorm(W), want_undecided=True)
    ref = _current_route(ops, z, Wp, b, W)
    torch.cuda.synchronize()
    und = int(und.item())
    print(f"K={K} N={N} {kind}: undecided {und} ({und / N:.4f})")
    assert idx.dtype == torch.int64 and idx.shape == (N,)
    mism = int((idx != ref).sum())
    assert mism == 0, f"{mism} rows differ from linear_fwd + vq_assign"
    assert und >= n_must, "planted midpoint / non-finite rows were decided by the screen"
    # the screen's radius is a worst-case fp32 bound (~400 u of the operands' magnitudes): codes drawn far from the data (N(0,1))
    # leave few rows to the exact path, codebooks 20x smaller than the data (all others here) more
    assert und <= (N // 8 if kind == "normal" else N // 2) + n_must


def test_nonfinite_codebook_and_projection_send_every_row_to_the_exact_path():
    from gesture2vec_amd import ops
    z, Wp, b, W, _ = _operands(512, 4096, "small", seed=9)
    for what in ("code", "w_pre", "bias"):
        W2, Wp2, b2 = W.clone(), Wp.clone(), b.clone()
        if what == "code":
            W2[100, 5] = float("nan")
        elif what == "w_pre":
            Wp2[3, 3] = float("inf")
        else:
            b2[0] = float("nan")
        idx, und = ops.vq_assign_bulk_z(z, Wp2, b2, W2, ops.vq_code_sqnorm(W2), want_undecided=True)
        assert int(und.item()) == 4096, what
        assert torch.equal(idx, _current_route(ops, z, Wp2, b2, W2)), what


def _raw_call(lib, z, Wp, b, W, wsq, idx, ws, nb, N, K):
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    return lib.g2v_vq_assign_bulk_z(p(z), p(Wp), p(b), p(W), p(wsq), p(idx), N, E, K, p(ws), nb, None,
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_workspace_poisoned_short_and_unsupported_shapes():
    from gesture2vec_amd import _lib, ops
    lib = _lib.load()
    K, N = 512, 20000 + 37
    z, Wp, b, W, _ = _operands(K, N, "trained", seed=21)
    wsq = ops.vq_code_sqnorm(W)
    nb = int(lib.g2v_vq_assign_bulk_z_workspace(N, E, K))
    ws = torch.full((nb // 4 + 64,), float("nan"), device=DEV)            # dirty: every byte a NaN pattern
    idx = torch.empty(N, dtype=torch.int64, device=DEV)
    assert _raw_call(lib, z, Wp, b, W, wsq, idx, ws, nb, N, K) == 0
    assert torch.equal(idx, _current_route(ops, z, Wp, b, W))
    ws.fill_(-1.0e30)
    idx2 = torch.empty_like(idx)
    assert _raw_call(lib, z, Wp, b, W, wsq, idx2, ws, nb, N, K) == 0
    assert torch.equal(idx2, idx)
    # short workspace
    sentinel = torch.full((N,), -7, dtype=torch.int64, device=DEV)
    assert _raw_call(lib, z, Wp, b, W, wsq, sentinel, ws, nb - 256, N, K) == -3
    assert b"workspace" in lib.g2v_last_error()
    # unsupported: another width, too few rows, a K outside the range -- nothing launched
    for (n, e, k) in ((N, 128, 512), (2047, 400, 512), (N, 400, 520), (N, 400, 1024)):
        assert not ops.vq_assign_bulk_z_ok(n, e, k)
        zz = torch.zeros(n, e, device=DEV)
        ww = torch.zeros(k, e, device=DEV)
        wp = torch.zeros(e, e, device=DEV)
        bb = torch.zeros(e, device=DEV)
        rc = lib.g2v_vq_assign_bulk_z(ctypes.c_void_p(zz.data_ptr()), ctypes.c_void_p(wp.data_ptr()), ctypes.c_void_p(bb.data_ptr()),
                                      ctypes.c_void_p(ww.data_ptr()), ctypes.c_void_p(wsq.data_ptr()),
                                      ctypes.c_void_p(sentinel.data_ptr()), n, e, k, ctypes.c_void_p(ws.data_ptr()), ws.numel() * 4,
                                      None, None)
        assert rc == -4 and b"g2v_vq_assign_bulk_z" in lib.g2v_last_error()
    torch.cuda.synchronize()
    assert bool((sentinel == -7).all()), "a refused call wrote to idx"


def test_smallm_rows_bound_follows_the_context():
    from gesture2vec_amd import _lib, ops
    assert ops.vq_assign_bulk_z_ok(4096, E, 512)
    with _lib.Context.current().scoped(smallm_rows=4096):
        assert not ops.vq_assign_bulk_z_ok(4096, E, 512)     # g2v_linear_fwd would take gemm_smallm_kernel there
        assert ops.vq_assign_bulk_z_ok(4097, E, 512)


def test_matches_the_oracle_outside_the_rounding_band():
    from gesture2vec_amd import ops
    from oracle import g2v_oracle as O
    K, N = 512, 2 ** 17 + 37
    z, Wp, b, W, _ = _operands(K, N, "normal", seed=5)
    idx = ops.vq_assign_bulk_z(z, Wp, b, W, ops.vq_code_sqnorm(W))
    rows = torch.cat([torch.arange(0, N, N // 8000)[:8000], torch.arange(N - 192, N)])
    zr = z[rows].cpu()
    fin = torch.isfinite(zr).all(1)
    flat_o = O.linear(zr[fin], Wp.cpu(), b.cpu())
    d = O.vq_distances(flat_o, W.cpu())
    top2 = torch.topk(d, 2, dim=1, largest=False).values
    safe = (top2[:, 1] - top2[:, 0]) > 1e-4 * torch.clamp(top2[:, 0].abs(), min=1.0)
    got = idx[rows.to(DEV)].cpu()[fin]
    assert torch.equal(got[safe], d.argmin(1)[safe]), "differs from the oracle outside the rounding band"
    assert int((~safe).sum()) <= len(rows) // 100


@pytest.mark.parametrize("K", [512, 400])
def test_quantiser_module_takes_the_new_route(K, monkeypatch):
    from gesture2vec_amd import _lib, ops
    from gesture2vec_amd.model import Autoencoder_VQVAE_model as M
    torch.manual_seed(K)
    q = M.VQ_Payam_EMA(K, E, 0.25, 0.85).to(DEV)
    min_rows = _lib.CONSTANTS["G2V_VQ_BULK_Z_MIN_ROWS"]
    N = max(min_rows, 2048) + 37
    assert ops.vq_route("RAW", "IDX_BULK", N, E, K) == "BULK_Z" and ops.vq_route("RAW", "IDX_BULK", min_rows - 1, E, K) == "PROJECT>PACKED*2"
    z = torch.randn(N, E, device=DEV) * 0.3
    calls = []
    real = ops.vq_assign_bulk_z
    monkeypatch.setattr(ops, "vq_assign_bulk_z", lambda *a, **k: calls.append(1) or real(*a, **k))
    idx = q.assign(z)
    assert calls, "VQ_Payam_EMA.assign did not take vq_assign_bulk_z"
    assert torch.equal(idx, _current_route(ops, z, q.pre_linear.weight.data, q.pre_linear.bias.data, q._embedding.weight.data))
    calls.clear()
    small = q.assign(z[:min_rows - 1])                       # below the threshold: the route of before
    assert not calls and small.shape == (min_rows - 1,)


def test_chunks_to_codes_at_the_shipped_width():
    from gesture2vec_amd import _lib, ops
    from gesture2vec_amd.model import Autoencoder_VQVAE_model as M
    from gesture2vec_amd.pipeline import chunk_latents, chunks_to_codes
    torch.manual_seed(17)
    D, H, L, K, T = 45, 200, 2, 512, 34
    N = max(_lib.CONSTANTS["G2V_VQ_BULK_Z_MIN_ROWS"], 2048) + 11
    assert ops.vq_route("RAW", "IDX_BULK", N, L * H, K) == "BULK_Z"
    args = argparse.Namespace(rep_learning_dim=D, hidden_size=H, n_layers=L, dropout_prob=0.0, autoencoder_vq="True",
                              autoencoder_vae="False", autoencoder_vq_components=K, autoencoder_vq_commitment_cost=0.25,
                              autoencoder_conditioned="True", autoencoder_att="False", autoencoder_fixed_weight="False",
                              n_pre_poses=1, n_poses=T)
    net = M.Autoencoder_VQVAE(args, D, T).to(DEV)
    net.train(False)
    chunks = torch.randn(N, T, D, device=DEV)
    lat, codes = chunks_to_codes(net, chunks)
    assert lat.shape == (N, L * H) and torch.equal(lat, chunk_latents(net, chunks))
    vq = net.vq_layer
    ref = _current_route(ops, lat, vq.pre_linear.weight.data, vq.pre_linear.bias.data, vq._embedding.weight.data)
    assert torch.equal(codes, ref)
