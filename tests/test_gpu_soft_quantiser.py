"""The soft quantiser's kernels (VQ_Payam_GSSoft: csrc/vq.hip's separate launches, csrc/vq_soft.hip's fused pair) against a float64
restatement of the oracle (tests/_soft_inputs.py: staged) at the shipped width E = 400, K = 512 and at the shapes where the kernels'
tiling has edges: N = 1, N % 4 != 0, N % 16 != 0, K < 64, K % 64 != 0, E % 64 != 0, K > 1024, more elements than one grid-stride pass.

The bound of every output is built from the reference alone: e_kernel <= max(8 e32, floor) with e32 the fp32 oracle's own distance from
float64 on the same input and floor the largest e32 of that output over all cases, never looser than the fused-versus-separate test's
tolerance (tests/_soft_inputs.py: bound, CAP).  Every test prints e_kernel, e32 and their ratio per output.

Largest e_kernel / e32 per output on the MI355X, over the separate, fused, perplexity and module tests (case, e_kernel, e32):
  flat 3.18 (sep-1x400x512, 7.3e-7, 2.3e-7)            logvar 2.09 (sep-4096x400x512, 7.3e-7, 3.5e-7)
  dist 1.51 (sep-517x400x512-peaked, 2.5e-7, 1.7e-7)   probs 2.50 (sep-517x400x512-peaked, 1.7e-6, 6.7e-7)
  q 3.35 (sep-130x128x1100, 1.5e-6, 4.5e-7)            quant 2.23 (sep-517x400x512-peaked, 1.5e-6, 6.6e-7)
  mse 3.79 (sep-517x400x512, 6.5e-8, 1.7e-8)           loss_vq 2.83 (sep-517x400x512, 4.8e-8, 1.7e-8)
  dq 1.97 (sep-517x400x512-peaked, 3.7e-7, 1.9e-7)     perplexity 123 (fused-1030x128x512, 4.8e-7, 3.9e-9): see below
  dd 2.29 (sep-1x400x512, 8.2e-7, 3.6e-7)              dlogvar 2.56 (sep-1x400x512, 6.9e-7, 2.7e-7)
  rowsum 2.25 (sep-517x400x512-peaked, 2.5e-6, 1.1e-6) dflat 3.10 (sep-130x128x1100, 1.3e-6, 4.2e-7)
  gz 1.00 (sep-4096x400x512, 8.5e-8, 8.5e-8)           g_embedding 1.47 (module-1024x400x512, 4.1e-7, 2.8e-7)
  g_mean_w 2.49 (fused-17x128x1024, 8.1e-7, 3.3e-7)    g_mean_b 1.96 (fused-17x128x1024, 6.5e-7, 3.3e-7)
  g_logvar_w 2.69 (sep-1x400x512, 1.2e-6, 4.5e-7)      g_logvar_b 2.80 (sep-517x400x512-peaked, 3.4e-7, 1.2e-7)
Every output but perplexity stays under half the margin of 8.  perplexity = exp(H) with the entropy H near ln 512 = 6.2: an fp32 H in [4, 8)
has spacing 2^-21 = 4.77e-7, and the relative error of exp(H) is the absolute error of H, so one ulp of H is 4.8e-7 of the result.
The three cases whose ratio is above 8 (fused-1030x128x512: 123, sep-1x400x512: 20.5, sep-4096x400x512: 12.3) have
e_kernel = 3.9e-7 to 4.8e-7, that one ulp, against an e32 of 3.9e-9 to 3.2e-8, below fp32's unit roundoff of 6e-8: there the
oracle's fp32 H happened to round onto the float nearest the exact value.  What holds them is the floor, 8.8e-7 (the largest e32 of
perplexity over all cases, under two ulp of H), as the rule provides; no bound was moved.  rowsum against the sum of the kernel's
own dd: 6.3e-9 to 7.2e-8 of the summed magnitudes, bound 4.2e-7 to 1.4e-6."""
import pytest
import torch

import _soft_inputs as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from gesture2vec_amd import ops as o
    return o


def _dev(inp):
    d = {k: v.to(DEV).contiguous() for k, v in inp.items()}
    d["gl"] = torch.full((1,), S.G_LOSS, device=DEV)
    return d


def _param_grads(ops, d, o):
    """the five parameter gradients from (dd, dlogvar, dflat, dq, probs, flat) by the products of _SoftAssignFn / _ProbsCodebookFn /
    LinearFn (gesture2vec_amd/model/Autoencoder_VQVAE_model.py)"""
    K, E = d["codebook"].shape
    tw, colsum = ops.linear_bwd_weight(o["dd"], o["flat"], K, E, want_bias=True)
    gW = ops.rowscale_combine(d["codebook"], colsum, tw)                       # 2 W sum_n dd - 2 dd^T flat
    tp, _ = ops.linear_bwd_weight(o["probs"], o["dq"], K, E, want_bias=False)  # probs^T dq
    o["g_embedding"] = gW + tp
    o["g_logvar_w"], o["g_logvar_b"] = ops.linear_bwd_weight(o["dlogvar"], o["flat"], K, E, want_bias=True)
    o["g_mean_w"], o["g_mean_b"] = ops.linear_bwd_weight(o["dflat"], d["x"], E, E, want_bias=True)
    return o


def run_separate(ops, d):
    """the call sequence of _SoftAssignFn / _ProbsCodebookFn / VQVAEEngine._backward_gssoft_chain"""
    x, Wm, bm, Wl, bl, W = (d[k] for k in ("x", "w_mean", "b_mean", "w_logvar", "b_logvar", "codebook"))
    o = {}
    o["flat"] = ops.linear_fwd(x, Wm, bm)
    o["logvar"] = ops.linear_fwd(o["flat"], Wl, bl)
    dots = ops.linear_fwd(o["flat"], W, None)
    o["probs"], o["dist"], o["perplexity"] = ops.vq_soft_fwd(o["flat"], dots, o["logvar"], ops.vq_code_sqnorm(W))
    o["q"] = ops.linear_bwd_data(o["probs"], W)
    o["mse"], o["dq"] = ops.mse_fwd_bwd(o["q"], x, True, S.G_SCALE)
    o["loss_vq"] = ops.scale(o["mse"], torch.full((1,), 1.0 + S.BETA, device=DEV))
    o["quant"] = ops.ste(x, o["q"])
    gz = ops.vq_bwd(d["dh"], d["gl"], x, o["q"], None, S.BETA)
    dprobs = ops.linear_fwd(o["dq"], W, None)
    o["dd"], o["dlogvar"], o["rowsum"] = ops.vq_soft_bwd(o["probs"], dprobs, o["dist"], o["logvar"])
    o["dflat"] = ops.rowscale_combine(o["flat"], o["rowsum"], ops.linear_bwd_data(o["dd"], W))
    ops.linear_bwd_data(o["dlogvar"], Wl, out=o["dflat"], accumulate=True)
    o["gz"] = ops.linear_bwd_data(o["dflat"], Wm, out=gz, accumulate=True)
    return _param_grads(ops, d, o)


def run_fused(ops, d):
    x, Wm, bm, Wl, bl, W = (d[k] for k in ("x", "w_mean", "b_mean", "w_logvar", "b_logvar", "codebook"))
    assert ops.vq_soft_fused_ok(x.shape[0], x.shape[1], W.shape[0])
    o = dict(ops.vq_soft_fused_fwd(x, Wm, bm, Wl, bl, W, S.BETA, S.G_SCALE))
    o["gz"], o["dd"], o["dlogvar"], o["dflat"] = ops.vq_soft_fused_bwd(d["dh"], d["gl"], x, o, Wm, Wl, W, S.BETA)
    return _param_grads(ops, d, o)


def _bitwise_equal(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _parity(ops, name, run, label):
    inp, _ = S.reference(name)
    d = _dev(inp)
    o, o2 = run(ops, d), run(ops, d)
    torch.cuda.synchronize()
    for k in o:
        assert _bitwise_equal(o[k], o2[k]), f"{k}: two runs differ"
    o = {k: v.cpu() for k, v in o.items()}
    return S.check_outputs(name, o, label), o


@pytest.mark.parametrize("case", list(S.SEPARATE_CASES))
def test_separate_kernels_match_float64(ops, case):
    """every forward and backward array and scalar of the separate launches, and that two runs are bitwise equal"""
    N, E, K = S.SEPARATE_CASES[case][:3]
    if E == 400 or K % 128 or K > 1024:
        assert not ops.vq_soft_fused_ok(N, E, K)
    rows, o = _parity(ops, "sep-" + case, run_separate, "separate")
    assert set(rows) == set(S.OUTPUTS)
    # rowsum is the sum of the dd the same launch wrote: one wave per row, a serial chain of ceil(K / 64) terms per lane and the six
    # levels of the wave reduction, so at most depth * 2^-24 of the summed magnitudes away from the exact sum of those fp32 values
    dd = o["dd"].double()
    depth = -(-K // 64) + 6
    e = float((o["rowsum"].double() - dd.sum(1)).abs().max()) / float(dd.abs().sum(1).max())
    print(f"separate sep-{case} rowsum against its own dd: {e:.3e} bound {depth * 2.0 ** -24:.3e}")
    assert e <= depth * 2.0 ** -24


@pytest.mark.parametrize("case", list(S.FUSED_CASES))
def test_fused_kernels_match_float64(ops, case):
    """the same for csrc/vq_soft.hip; at N = 1, 15, 17 the padded rows of the ragged 16-row tile would show in mse / loss_vq /
    perplexity (and in the parameter gradients' inputs) if they leaked into mse_partial / colsum"""
    rows, _ = _parity(ops, "fused-" + case, run_fused, "fused")
    assert set(rows) == set(S.OUTPUTS) - {"rowsum"}          # the fused backward keeps the row sums in LDS


@pytest.mark.parametrize("name", ["sep-130x128x1100", "sep-517x400x512", "sep-517x400x512-peaked", "sep-1x400x512", "sep-33x64x48"])
def test_perplexity_three_ways(ops, name):
    """the one-workgroup kernel inside g2v_vq_soft_fwd (perplexity != NULL), g2v_vq_soft_perplexity's two launches, float64"""
    from gesture2vec_amd import _lib
    lib = _lib.load()
    inp, ref = S.reference(name)
    d = _dev(inp)
    N, E = d["x"].shape
    K = d["codebook"].shape[0]
    flat = ops.linear_fwd(d["x"], d["w_mean"], d["b_mean"])
    logvar = ops.linear_fwd(flat, d["w_logvar"], d["b_logvar"])
    wsq = ops.vq_code_sqnorm(d["codebook"])
    st = torch.cuda.current_stream().cuda_stream
    got = []
    for _ in range(2):
        dots = ops.linear_fwd(flat, d["codebook"], None)
        probs = torch.empty((N, K), device=DEV)
        perp = torch.full((1,), -1.0, device=DEV)
        _lib.check(lib.g2v_vq_soft_fwd(flat.data_ptr(), dots.data_ptr(), logvar.data_ptr(), wsq.data_ptr(), probs.data_ptr(),
                                       perp.data_ptr(), N, E, K, st), "vq_soft_fwd")
        got.append(perp)
    probs2, _, perp2 = ops.vq_soft_fwd(flat, ops.linear_fwd(flat, d["codebook"], None), logvar, wsq)
    torch.cuda.synchronize()
    assert _bitwise_equal(got[0], got[1]) and _bitwise_equal(probs, probs2)
    S.check_outputs(name, {"perplexity": got[0].cpu()}, "one-workgroup perplexity")
    S.check_outputs(name, {"perplexity": perp2.cpu()}, "two-launch perplexity")
    b = S.bound(name, "perplexity")
    assert abs(float(got[0]) - float(perp2)) <= 2 * b * float(ref["perplexity"])


ROW_CASES = {"separate": ("sep", S.Case(37, 400, 512, 0.3, *S.FLAT)), "fused": ("fused", S.Case(37, 128, 512, 0.3, *S.FLAT))}


@pytest.mark.parametrize("row", [7, 36])
@pytest.mark.parametrize("route", ["separate", "fused"])
def test_a_nan_row_stays_in_its_row(ops, route, row):
    """NaN in one row of x (row 7: inside the full tile 0..15; row 36: the last real row of the ragged tile 32..36, the row the padded
    lanes of the fused kernels read in its place): every other row of every per-row array is bitwise what the run with that row
    zeroed gives."""
    inp = S.make_inputs(ROW_CASES[route][1])
    run = run_separate if route == "separate" else run_fused
    outs = []
    for fill in (0.0, float("nan")):
        d = _dev(inp)
        d["x"][row] = fill
        outs.append(run(ops, d))
    torch.cuda.synchronize()
    others = [r for r in range(inp["x"].shape[0]) if r != row]
    for k in ("flat", "logvar", "dist", "probs", "q", "quant", "gz", "dflat", "dq", "dd", "dlogvar"):
        a, b = outs[0][k], outs[1][k]
        assert bool(torch.isnan(b[row]).all()), f"{k}: the NaN row came out finite"
        assert bool(torch.isfinite(a).all()), k
        assert _bitwise_equal(a[others], b[others]), f"{k}: a NaN in row {row} reached another row"


SENT = -12345.678


@pytest.mark.parametrize("N", [17, 517])
def test_kernels_write_nothing_behind_their_rows(ops, N):
    """C ABI calls with every (N, .) output carved from a sentinel-filled buffer 16 rows longer, mse_partial / colsum 16 blocks longer
    than g2v_vq_soft_fused_blocks(N): the guard rows are untouched by the fused forward / backward and by g2v_vq_soft_fwd / _bwd"""
    from gesture2vec_amd import _lib
    lib = _lib.load()
    E, K, G = 128, 512, 16
    d = _dev(S.make_inputs(S.Case(N, E, K, 0.3, *S.FLAT)))
    st = torch.cuda.current_stream().cuda_stream
    buf = lambda rows, cols: torch.full((rows + G, cols), SENT, device=DEV)
    p = lambda t: t.data_ptr()
    wsq = ops.vq_code_sqnorm(d["codebook"])
    nblk = lib.g2v_vq_soft_fused_blocks(N)
    assert nblk == (N + 15) // 16
    f = {k: buf(N, E) for k in ("flat", "q", "dq", "quant", "dflat", "gz")}
    f.update({k: buf(N, K) for k in ("logvar", "dist", "probs", "dd", "dlogvar")})
    f["mse_partial"], f["colsum"] = buf(nblk, 1), buf(nblk, K)
    _lib.check(lib.g2v_vq_soft_fused_fwd(p(d["x"]), p(d["w_mean"]), p(d["b_mean"]), p(d["w_logvar"]), p(d["b_logvar"]), p(d["codebook"]),
                                         p(wsq), p(f["flat"]), p(f["logvar"]), p(f["dist"]), p(f["probs"]), p(f["q"]), p(f["dq"]),
                                         p(f["quant"]), p(f["mse_partial"]), p(f["colsum"]), S.G_SCALE, N, E, K, st), "fused_fwd")
    _lib.check(lib.g2v_vq_soft_fused_bwd(p(d["dh"]), p(d["gl"]), p(d["x"]), p(f["q"]), p(f["dq"]), p(f["flat"]), p(f["probs"]),
                                         p(f["dist"]), p(f["logvar"]), p(d["w_mean"]), p(d["w_logvar"]), p(d["codebook"]), p(f["dd"]),
                                         p(f["dlogvar"]), p(f["dflat"]), p(f["gz"]), S.BETA, N, E, K, st), "fused_bwd")
    # the separate pair on the fused forward's flat / logvar
    s = {"dots": buf(N, K), "probs": buf(N, K), "perp": buf(1, 1), "dd": buf(N, K), "dlogvar": buf(N, K), "rowsum": buf(N, 1)}
    s["dots"][:N] = ops.linear_fwd(f["flat"][:N], d["codebook"], None)
    dprobs = ops.linear_fwd(f["dq"][:N], d["codebook"], None)
    _lib.check(lib.g2v_vq_soft_fwd(p(f["flat"]), p(s["dots"]), p(f["logvar"]), p(wsq), p(s["probs"]), p(s["perp"]), N, E, K, st), "soft_fwd")
    _lib.check(lib.g2v_vq_soft_bwd(p(s["probs"]), p(dprobs), p(s["dots"]), p(f["logvar"]), p(s["dd"]), p(s["dlogvar"]), p(s["rowsum"]),
                                   N, K, st), "soft_bwd")
    torch.cuda.synchronize()
    for tag, group in (("fused", f), ("separate", s)):
        for k, t in group.items():
            rows = t.shape[0] - G
            assert bool((t[rows:] == SENT).all()), f"{tag} {k}: wrote behind its {rows} rows"
            assert bool((t[:rows] != SENT).all()) and bool(torch.isfinite(t[:rows]).all()), f"{tag} {k}: a row was left unwritten"
    # and the guarded calls computed what the wrappers compute
    o = run_fused(ops, d)
    for k in ("flat", "logvar", "dist", "probs", "q", "dq", "quant", "dd", "dlogvar", "dflat", "gz"):
        assert _bitwise_equal(f[k][:N], o[k]), k
    assert S.relerr(s["probs"][:N], o["probs"]) < 5e-5 and S.relerr(s["dd"][:N], o["dd"]) < 3e-4


@pytest.mark.parametrize("case", list(S.MODULE_CASES))
def test_module_matches_float64(case):
    """VQ_Payam_GSSoft.forward in training mode on inputs (2, 1024, E / 2) + the backward of (quantized gq).sum() + c loss, and
    assign(), against float64.  E = 400: the shipped shape (every real checkpoint).  The module calls the separate launches at both
    widths; the fused pair is reached through the engine only (tests/test_gpu_shipped_gssoft.py)."""
    from gesture2vec_amd.model.Autoencoder_VQVAE_model import VQ_Payam_GSSoft
    name = "module-" + case
    N, E, K = S.MODULE_CASES[case][:3]
    inp, ref = S.reference(name)
    q = VQ_Payam_GSSoft(K, E, S.BETA)
    q.load_state_dict(S.state_dict(inp), strict=True)
    q = q.to(DEV)
    q.train(True)
    z = inp["x"].view(2, N, E // 2).to(DEV).requires_grad_(True)
    loss, quant, perp, probs = q(z)
    assert quant.shape == z.shape and probs.shape == (N, K)
    ((quant * inp["dh"].view(2, N, E // 2).to(DEV)).sum() + S.G_LOSS * loss).backward()
    torch.cuda.synchronize()
    assert q.pre_linear.weight.grad is None and q.pre_linear.bias.grad is None
    got = {"loss_vq": loss, "quant": quant.reshape(N, E), "perplexity": perp, "probs": probs, "gz": z.grad.reshape(N, E),
           "g_mean_w": q.mean_layer.weight.grad, "g_mean_b": q.mean_layer.bias.grad, "g_logvar_w": q.logvar_layer.weight.grad,
           "g_logvar_b": q.logvar_layer.bias.grad, "g_embedding": q._embedding.weight.grad}
    S.check_outputs(name, {k: v.detach().cpu() for k, v in got.items()}, "module")
    # assign(): the float64 mode wherever the decision is not a near-tie, a code within 1e-4 of the row maximum elsewhere
    idx = q.assign(z.detach()).cpu()
    p64 = ref["probs"]
    assert idx.dtype == torch.int64 and idx.shape == (N,)
    near = S.near_tie_rows(p64)
    assert int(near.sum()) <= N // 100
    assert torch.equal(idx[~near], p64.argmax(1)[~near])
    assert bool((p64[torch.arange(N), idx] >= (1 - 1e-4) * p64.max(1).values).all())
