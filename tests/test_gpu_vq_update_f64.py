"""The codebook update kernels against float64 at their tiling edges: code statistics (both kernels behind g2v_vq_stats), the EMA
update (both entry points), g2v_vq_bwd in all its forms, the codebook gradient, the code norms, the straight-through value, and
one engine step at a batch the tile-owner kernel's row split once left rows out of.

Reference and bars: tests/_vq_update_ref.py (float64 numpy; every bar derived there from the operation, none from a kernel's
output).  Cases and inputs: tests/_vq_update_cases.py.  tests/test_vq_update_ref_host.py shows, without a device, that a
strictly sequential float32 restatement is inside every bar and each planted defect outside.  Counts and copies are compared for
equality.

What this module found: vq_stats_owner_kernel gave each of its four waves ((N / 4) + 3) & ~3 rows, which is short of N when
N % 16 is 1, 2 or 3, so the last one to three rows were in no count and no sum (N = 1025, 1026, 1027, 4099 below, and the engine
step at B = 1025).  The split is now ceil(N / 4) rounded up to a multiple of 4.

Largest observed error as a fraction of its bar, over all cases (MI355X; each test prints its own as `FRACTION name value`):
    statistics sums   tile owner 0.38   slabs 0.22   two shards summed 0.18
    EMA update        plain: cs 0.45  ema_w 0.98  codebook 0.52  |W|^2 0.10  loss 0.04  perplexity 0.05
                      exact: cs 0.40  ema_w 0.97  codebook 0.47  |W|^2 0.09  loss 0.04  perplexity 0.05
                      ema_w from zero at decay 0.99 (one product): plain 0.50, exact 0.49; the other entry point's weight would sit at 7.8
    vq_bwd            with g_quantized 0.998   loss term alone 0.42   (without g_loss: equality)
    codebook_grad 0.40   code_sqnorm 0.07   engine perplexity at B = 1025: 5e-5
The three figures near one are expected and the bars stay as derived.  ema_w' = ema_w d + w dw is two products and one sum, vq_bwd
with g_quantized ends in one sum whose other term is 1e-6 of it: the bars are gamma(2) (|ema_w d| + |w dw|) and, in effect, one
rounding of the result.  A single rounding reaches its whole bound u |x| when x sits just above a power of two, so the largest of
5e4 .. 5e5 elements comes close to a bound that no element can pass; the codebook, a quotient of ema_w', inherits half of it.
The sums, whose bars are worst cases over n roundings of either sign, stay far below."""
import numpy as np
import pytest
import torch

import _vq_update_cases as C
import _vq_update_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -12345.0


@pytest.fixture(scope="module")
def ops():
    from gesture2vec_amd import _lib, ops as _ops
    assert _lib.load().g2v_device_ok() == 1, "no gfx950 device visible"
    return _ops


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def inside(name, got, ref, bar):
    """print the figure, then assert"""
    frac, bad = R.fraction(host(got) if isinstance(got, torch.Tensor) else got, ref, bar)
    print(f"FRACTION {name} {frac:.4f}")
    assert bad == 0, f"{name}: {bad} elements outside the bar, worst at {frac:.3g} of it"


def run_stats(idx_d, flat_d, K, fill=SENTINEL):
    """g2v_vq_stats with a workspace of this test's own, filled with a sentinel: (stats, workspace as float32)"""
    from gesture2vec_amd import _lib
    lib = _lib.load()
    N, E = flat_d.shape
    nbytes = int(lib.g2v_vq_stats_workspace(N, E, K))
    assert nbytes % 4 == 0 and nbytes >= 4 * (K * E + K)
    ws = torch.full((nbytes // 4,), fill, dtype=torch.float32, device=DEV)
    out = torch.full((K + K * E,), float("nan"), dtype=torch.float32, device=DEV)
    _lib.check(lib.g2v_vq_stats(idx_d.data_ptr(), flat_d.data_ptr(), out.data_ptr(), N, E, K, ws.data_ptr(), nbytes,
                                torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return out, ws


# ---- statistics ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", C.ID_KINDS)
@pytest.mark.parametrize("N,E,K", list(C.STATS_CASES))
def test_statistics_against_float64(ops, N, E, K, kind):
    idx, flat = C.stats_inputs(N, E, K, kind)
    cnt, dw, mag = R.stats(idx, flat, K)
    owner = C.STATS_CASES[(N, E, K)]["owner"]
    idx_d, flat_d = dev(idx), dev(flat)
    stats, ws = run_stats(idx_d, flat_d, K)
    # the route: the tile-owner kernel never touches the workspace, the slab kernel fills every slab of every split
    untouched = ws == SENTINEL
    if owner:
        assert bool(untouched.all()), "expected the tile-owner kernel: it leaves the workspace alone"
    else:
        used = C.slab_splits(N, E, K) * (K * E + K)
        assert used * 4 == ws.numel() * 4 and not bool(untouched.any()), "expected the slab kernel: it writes every slab"
    got_cnt = host(stats[:K])
    assert np.array_equal(got_cnt, cnt.astype(np.float32)), \
        f"counts differ at codes {np.flatnonzero(got_cnt != cnt)[:8]}: got sum {got_cnt.sum():.0f} of {N} rows"
    c = R.C_BLOCK if owner else R.c_slab(C.slab_splits(N, E, K))
    inside("stats_owner_dw" if owner else "stats_slab_dw", stats[K:].reshape(K, E), dw, R.stats_bar(cnt, mag, c))
    # a second call on a dirty workspace: the same bits
    again, _ = run_stats(idx_d, flat_d, K, fill=3.0e38)
    assert torch.equal(bits(again), bits(stats)), "the result depends on what the workspace held"


@pytest.mark.parametrize("shape", list(C.ADDITIVITY))
def test_statistics_of_two_shards_add_up_to_the_batch(ops, shape):
    N, E, K = shape
    a, _ = C.ADDITIVITY[shape]
    idx, flat = C.stats_inputs(N, E, K, "random")
    cnt, dw, mag = R.stats(idx, flat, K)
    whole, _ = run_stats(dev(idx), dev(flat), K)
    parts = [run_stats(dev(idx[s]), dev(flat[s]), K)[0] for s in (slice(0, a), slice(a, N))]
    total = parts[0] + parts[1]                     # what the SUM all-reduce of the data-parallel step forms
    assert torch.equal(total[:K], whole[:K]) and np.array_equal(host(total[:K]), cnt.astype(np.float32))
    c = 1 + max(R.c_slab(C.slab_splits(n, E, K)) for n in (a, N - a))
    inside("stats_shards_dw", total[K:].reshape(K, E), dw, R.stats_bar(cnt, mag, c))


# ---- EMA update ------------------------------------------------------------------------------------------------------------------
def _ema_device(i, K, E):
    stats = dev(np.concatenate([i["cnt"], i["dw"].reshape(-1)]))
    return stats, dev(i["sse"]), dev(i["cs"]), dev(i["ema_w"]), torch.full((K, E), 7.0, device=DEV), torch.full((K,), 7.0, device=DEV)


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("decay", C.EMA_DECAYS)
@pytest.mark.parametrize("n_sse", C.EMA_N_SSE)
@pytest.mark.parametrize("E,K", C.EMA_CASES)
def test_ema_update_against_float64(ops, E, K, n_sse, decay, exact):
    i = C.ema_inputs(E, K, n_sse)
    ref = R.ema_step(i["cnt"], i["dw"], i["sse"], i["cs"], i["ema_w"], i["N_loss"], i["N_cnt"], C.BETA, decay, C.EPS, exact)
    tag = "exact" if exact else "plain"
    call = lambda st, sse, *state, update: ops.vq_ema_update(st, sse, *state, i["N_loss"], i["N_cnt"], E, K, C.BETA, decay, C.EPS,
                                                             update, exact_decay=exact)
    # update = 0 with state given: the state stays bitwise as it was, both scalars are written
    stats, sse, cs, ew, W, wsq = _ema_device(i, K, E)
    before = [t.clone() for t in (cs, ew, W, wsq)]
    sc = call(stats, sse, cs, ew, W, wsq, update=False)
    for t, b in zip((cs, ew, W, wsq), before):
        assert torch.equal(bits(t), bits(b)), "update = 0 wrote EMA state"
    inside(f"ema_{tag}_loss", sc[0], *ref["loss"])
    inside(f"ema_{tag}_perplexity", sc[1], *ref["perplexity"])
    # update = 0 with null state pointers (the form VQ_Payam calls)
    sc0 = call(stats, sse, None, None, None, None, update=False)
    assert torch.equal(bits(sc0), bits(sc))
    # the step
    sc1 = call(stats, sse, cs, ew, W, wsq, update=True)
    assert torch.equal(bits(sc1), bits(sc)), "the scalars do not depend on `update`"
    for name, got in (("cs", cs), ("ema_w", ew), ("codebook", W), ("wsq", wsq)):
        inside(f"ema_{tag}_{name}", got, *ref[name])
    assert torch.equal(stats, dev(np.concatenate([i["cnt"], i["dw"].reshape(-1)]))), "the statistics are read-only"


@pytest.mark.parametrize("E,K", C.EMA_CASES)
def test_ema_entry_points_use_their_own_weight_at_decay_099(ops, E, K):
    """from ema_w = 0 the new ema_w is w dw: the two entry points' weights differ by 9.3e-7 of their value, 7.8 times the bar"""
    i = C.ema_inputs(E, K, 7, True)
    for exact in (False, True):
        ref = R.ema_step(i["cnt"], i["dw"], i["sse"], i["cs"], i["ema_w"], i["N_loss"], i["N_cnt"], C.BETA, 0.99, C.EPS, exact)
        stats, sse, cs, ew, W, wsq = _ema_device(i, K, E)
        ops.vq_ema_update(stats, sse, cs, ew, W, wsq, i["N_loss"], i["N_cnt"], E, K, C.BETA, 0.99, C.EPS, True, exact_decay=exact)
        inside(f"ema_{'exact' if exact else 'plain'}_ema_w_from_zero", ew, *ref["ema_w"])


# ---- vq_bwd ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gathered", [True, False])
@pytest.mark.parametrize("has_gq,has_gl", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("N,E,K", list(C.BWD_CASES))
def test_vq_bwd_against_float64(ops, N, E, K, has_gq, has_gl, gathered):
    i = C.bwd_inputs(N, E, K)
    gq, gl = (i["gq"] if has_gq else None), (i["gl"] if has_gl else None)
    val, bar = R.vq_bwd(gq, gl, i["z"], i["dense"], N, E, C.BETA)
    out = torch.full((N, E), float("nan"), device=DEV)
    gz = ops.vq_bwd(dev(gq), dev(gl), dev(i["z"]), dev(i["W"] if gathered else i["dense"]), dev(i["idx"]) if gathered else None,
                    C.BETA, out=out)
    torch.cuda.synchronize()
    if has_gl:
        inside("vq_bwd_with_gq" if has_gq else "vq_bwd_loss_only", gz, val, bar)
    else:
        assert np.array_equal(host(gz), val.astype(np.float32)), "without g_loss the result is g_quantized, or zero, exactly"


# ---- codebook gradient, code norms, straight-through value -----------------------------------------------------------------------
@pytest.mark.parametrize("E,K", list(C.CBGRAD_CASES))
def test_codebook_grad_against_float64(ops, E, K):
    idx, flat = C.cbgrad_inputs(E, K)
    stats, _ = run_stats(dev(idx), dev(flat), K)
    cnt32, dw32 = host(stats[:K]), host(stats[K:]).reshape(K, E)        # the float32 statistics the kernel reads
    assert np.array_equal(cnt32, np.bincount(idx, minlength=K).astype(np.float32)) and (cnt32 == 0).any()
    W, gl = C.codebook(K, E), np.array([C.G_LOSS], np.float32)
    val, bar = R.codebook_grad(cnt32, dw32, W, gl, C.CBGRAD_ROWS)
    inside("codebook_grad", ops.vq_codebook_grad(stats, dev(W), dev(gl), C.CBGRAD_ROWS), val, bar)


@pytest.mark.parametrize("K,E", C.SQNORM_CASES)
def test_code_sqnorm_against_float64(ops, K, E):
    W = C.codebook(K, E)
    out = torch.full((K + 3,), SENTINEL, device=DEV)
    ops.vq_code_sqnorm(dev(W), out=out)
    inside("code_sqnorm", out[:K], *R.code_sqnorm(W))
    assert bool((out[K:] == SENTINEL).all()), "the partly idle last workgroup wrote past K"


@pytest.mark.parametrize("n", C.STE_COUNTS)
def test_straight_through_value_is_the_reference_float32_expression(ops, n):
    z, q = C.ste_inputs(n)
    got = ops.ste(dev(z), dev(q))
    assert np.array_equal(host(got).view(np.int32), R.ste(z, q).view(np.int32))


# ---- where a user would meet it --------------------------------------------------------------------------------------------------
def test_engine_step_counts_every_row_of_a_batch_of_1025(ops):
    """one train_step at B = 1025 (N = B rows of E = 128 at K = 512: the tile-owner kernel, N % 16 = 1)"""
    from oracle import g2v_oracle as O
    from test_gpu_dp_engine import _engine
    B, T, D, H, K = 1025, 4, 135, 64, 512
    assert C.owner_route(B, 2 * H, K) and B % 16 == 1
    sd = O.init_vqvae_state(D, H, 2, K, seed=11)
    eng = _engine(sd, D, H, K, T, 0.0)
    x = torch.randn(B, T, D, generator=torch.Generator().manual_seed(5)).to(DEV)
    eng.train_step(x, x, lr=5e-4, w_l1=5.0, w_cont=0.1, w_var=0.5, draw_masks=True)
    torch.cuda.synchronize()
    idx = host(eng.buffers(B)["idx"]).reshape(-1)
    assert idx.shape == (B,)
    cnt = np.bincount(idx, minlength=K).astype(np.float32)
    got = host(eng.vq_stats[:K])
    assert float(got.astype(np.float64).sum()) == float(B), f"the engine counted {got.sum():.0f} of {B} rows"
    assert np.array_equal(got, cnt)
    val, bar = R.perplexity(cnt, B)
    perp = float(eng.vq_scalars[1].item())
    print(f"FRACTION engine_perplexity {abs(perp - val) / bar:.4f}")
    assert abs(perp - val) <= bar, f"perplexity {perp!r} vs {val!r} from the engine's own code ids: off by {abs(perp - val) / bar:.3g} bars"
