"""Host conditions of the codebook-update bars (tests/_vq_update_ref.py), for every case of tests/_vq_update_cases.py, before the
GPU test (tests/test_gpu_vq_update_f64.py) may rely on them:

  * not too tight: a float32 restatement that takes every sum strictly sequentially -- the worst order the bars admit -- is inside;
  * not too loose: each planted defect lands outside a bar or breaks an equality (the last row dropped, one row credited to the
    neighbouring code, decay and 1 - decay swapped, the `_exact` weight replaced by the plain one at decay 0.99);
  * the tables say what they claim: every stated fact follows from the launchers' constants by plain arithmetic.

No device, no library: numpy only."""
import numpy as np
import pytest

import _vq_update_cases as C
import _vq_update_ref as R

STATS_PARAMS = [(*shape, kind) for shape in C.STATS_CASES for kind in C.ID_KINDS]
EMA_PARAMS = [(E, K, n_sse, decay, exact) for (E, K) in C.EMA_CASES for n_sse in C.EMA_N_SSE for decay in C.EMA_DECAYS
              for exact in (False, True)]


def inside(got, ref, bar, what):
    frac, bad = R.fraction(got, ref, bar)
    assert bad == 0, f"{what}: {bad} elements outside the bar, worst at {frac:.3g} of it"
    return frac


def outside(got, ref, bar, what):
    frac, bad = R.fraction(got, ref, bar)
    assert bad > 0, f"{what}: the planted defect stays inside the bar (worst {frac:.3g} of it)"


# ---- the tables ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,E,K", list(C.STATS_CASES))
def test_statistics_tables_state_facts(N, E, K):
    facts = C.STATS_CASES[(N, E, K)]
    owner = E % 16 == 0 and K % 16 == 0 and N >= 1024 and (K // 16) * (E // 16) >= 128
    assert facts["owner"] == owner == C.owner_route(N, E, K)
    assert ((N, E, K) in C.STATS_OWNER) == owner
    if "rem16" in facts:
        assert N % 16 == facts["rem16"]
    if "tiles16" in facts:
        assert (K // 16) * (E // 16) == facts["tiles16"] and K % 16 == 0 and E % 16 == 0
    if "e_rem16" in facts:
        assert E % 16 == facts["e_rem16"] != 0 and K % 16 == 0 and N >= 1024
    if "k_rem16" in facts:
        assert K % 16 == facts["k_rem16"] != 0 and E % 16 == 0 and N >= 1024
    if "column_tiles" in facts:
        assert E // 16 == facts["column_tiles"]
    if owner:
        per = C.owner_rows_per_wave(N)
        assert per % 4 == 0 and 4 * per >= N > 3 * per, "the four waves' shares cover every row and each wave has one"
        if facts.get("ragged_batch"):
            assert 4 * per == N + 4 and per % C.OWNER_BATCH not in (0, C.OWNER_BATCH // 2), "a wave's last batch is partly idle"
        # what the split was before: short exactly at the remainders 1, 2, 3
        assert (4 * (((N // 4) + 3) & ~3) < N) == (N % 16 in (1, 2, 3))
    else:
        tiles = -(-K // 64) * -(-E // 64)
        splits = max(1, min(-(-512 // tiles), -(-N // 64)))
        rows = -(-(-(-N // splits)) // 32) * 32
        assert (splits, rows) == (C.slab_splits(N, E, K), C.slab_rows_per_split(N, E, K))
        if "splits" in facts:
            assert splits == facts["splits"] and N - (splits - 1) * rows == facts["last"] == C.slab_last_split_rows(N, E, K)
        assert splits * rows >= N


def test_a_slab_split_without_rows_exists_and_the_table_holds_one():
    """the issue asks for such a case if host arithmetic finds one: search small shapes that take the slab kernel"""
    found = [(N, E, K) for K in (64, 512) for E in (64, 128, 1024, 1088) for N in range(1, 1100)
             if not C.owner_route(N, E, K) and C.slab_last_split_rows(N, E, K) <= 0]
    assert (257, 1024, 512) in found
    assert any(C.slab_last_split_rows(*s) <= 0 for s in C.STATS_SLAB)


def test_remaining_tables_state_facts():
    for (N, E, K), facts in C.BWD_CASES.items():
        assert -(-N * E // C.GRID_CAP) == facts["passes"] and (N * E) % 256 == facts["rem256"]
        assert bool(facts.get("exactly_cap")) == (N * E == C.GRID_CAP)
    for (E, K), facts in C.CBGRAD_CASES.items():
        assert -(-K * E // C.GRID_CAP) == facts["passes"]
    assert (400, 1320) in C.CBGRAD_CASES and 400 * 1320 == 528000 > C.GRID_CAP == 524288
    assert any(K % 4 for K, _ in C.SQNORM_CASES) and {63, 64, 65} <= {E for _, E in C.SQNORM_CASES}
    assert max(C.STE_COUNTS) == C.GRID_CAP + 1 and {1, 255, 257} <= set(C.STE_COUNTS)
    assert any(n > C.EMA_THREADS for n in C.EMA_N_SSE) and 1 in C.EMA_N_SSE
    for shape, (a, b) in C.ADDITIVITY.items():
        assert a + b == shape[0] and shape in C.STATS_CASES
    assert C.owner_route(1026, 128, 256) and not C.owner_route(513, 128, 256)
    for (E, K) in C.EMA_CASES:
        inp = C.ema_inputs(E, K, 7)
        assert inp["N_loss"] != inp["N_cnt"] == int(inp["cnt"].sum()) and inp["N_loss"] > 0
        if K >= 2:
            assert inp["dead"].any() and not inp["cnt"][inp["dead"]].any() and not inp["cs"][inp["dead"]].any()


# ---- statistics ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,E,K,kind", STATS_PARAMS)
def test_statistics_bar_admits_sequential_float32_and_rejects_planted_defects(N, E, K, kind):
    idx, flat = C.stats_inputs(N, E, K, kind)
    cnt, dw, mag = R.stats(idx, flat, K)
    assert int(cnt.sum()) == N
    if K >= 2:
        assert (cnt == 0).any(), "at least one code receives no row"
    if N > 2 * C.BIG_ROWS:
        assert np.abs(flat[-C.BIG_ROWS:]).mean() > 16 * np.abs(flat[:-C.BIG_ROWS]).mean()
    c = R.C_BLOCK if C.owner_route(N, E, K) else R.c_slab(C.slab_splits(N, E, K))
    bar = R.stats_bar(cnt, mag, c)
    cnt32, dw32 = R.stats_f32(idx, flat, K)
    assert np.array_equal(cnt32.astype(np.int64), cnt)
    inside(dw32, dw, bar, "sequential float32 sums")
    # the last row dropped
    cnt_d, dw_d = R.stats_f32(idx[:-1], flat[:-1], K)
    assert not np.array_equal(cnt_d.astype(np.int64), cnt)
    outside(dw_d, dw, bar, "last row dropped")
    # one row credited to the neighbouring code
    if K >= 2:
        moved = idx.copy()
        moved[N // 2] = (moved[N // 2] + 1) % K
        cnt_m, dw_m = R.stats_f32(moved, flat, K)
        assert not np.array_equal(cnt_m.astype(np.int64), cnt)
        outside(dw_m, dw, bar, "one row credited to the neighbouring code")


@pytest.mark.parametrize("shape", list(C.ADDITIVITY))
def test_shard_sums_stay_inside_the_bar_with_one_more_merge(shape):
    N, E, K = shape
    a, _ = C.ADDITIVITY[shape]
    idx, flat = C.stats_inputs(N, E, K, "random")
    cnt, dw, mag = R.stats(idx, flat, K)
    ca, da = R.stats_f32(idx[:a], flat[:a], K)
    cb, db = R.stats_f32(idx[a:], flat[a:], K)
    assert np.array_equal((ca + cb).astype(np.int64), cnt)
    c = 1 + max(R.c_slab(C.slab_splits(n, E, K)) for n in (a, N - a))
    inside(da + db, dw, R.stats_bar(cnt, mag, c), "two float32 shards summed")


# ---- EMA step --------------------------------------------------------------------------------------------------------------------
def _ema_args(E, K, n_sse, zero_ema_w=False):
    i = C.ema_inputs(E, K, n_sse, zero_ema_w)
    return (i["cnt"], i["dw"], i["sse"], i["cs"], i["ema_w"], i["N_loss"], i["N_cnt"], C.BETA)


@pytest.mark.parametrize("E,K,n_sse,decay,exact", EMA_PARAMS)
def test_ema_bars_admit_sequential_float32_and_reject_planted_defects(E, K, n_sse, decay, exact):
    args = _ema_args(E, K, n_sse)
    ref = R.ema_step(*args, decay, C.EPS, exact)
    got = R.ema_step_f32(*args, decay, C.EPS, exact)
    for name, (val, bar) in ref.items():
        assert np.all(np.isfinite(val)) and np.all(np.asarray(bar) >= 0)
        inside(got[name], val, bar, name)
    # decay and 1 - decay swapped
    swapped = R.ema_step(*args, decay, C.EPS, exact, swap_weights=True)
    for name in ("cs", "ema_w", "codebook", "wsq"):
        if name == "codebook" and K == 1 and E == 1:
            continue      # one code: ema_w and the cluster size are scaled alike and their quotient does not move far
        outside(swapped[name][0], *ref[name], f"{name} with decay and 1 - decay swapped")


@pytest.mark.parametrize("E,K", C.EMA_CASES)
def test_exact_and_plain_weight_are_told_apart_at_decay_099(E, K):
    """from ema_w = 0 the new ema_w is w dw alone: the two weights differ by 9.3e-7 of their value, the bar is gamma(2)"""
    d, plain = R.ema_weights(0.99, False)
    _, exact = R.ema_weights(0.99, True)
    assert abs(float(plain) / float(exact) - 1.0) == pytest.approx(9.3e-7, rel=0.02)
    args = _ema_args(E, K, 7, zero_ema_w=True)
    for is_exact, wrong in ((True, plain), (False, exact)):
        ref = R.ema_step(*args, 0.99, C.EPS, is_exact)
        got = R.ema_step_f32(*args, 0.99, C.EPS, is_exact)
        inside(got["ema_w"], *ref["ema_w"], "ema_w from zero")
        planted = R.ema_step(*args, 0.99, C.EPS, is_exact, weights=(d, wrong))
        outside(planted["ema_w"][0], *ref["ema_w"], "ema_w with the other entry point's weight")


@pytest.mark.parametrize("N,E,K,kind", [(s + (k,)) for s in list(C.STATS_CASES)[:3] + [(33, 100, 7)] for k in C.ID_KINDS])
def test_perplexity_bar_from_statistics_counts(N, E, K, kind):
    """the bar the end-to-end check uses: sequential float32 inside, one row dropped or moved outside"""
    idx, _ = C.stats_inputs(N, E, K, kind)
    cnt = np.bincount(idx, minlength=K).astype(np.float32)
    val, bar = R.perplexity(cnt, N)
    p = cnt / np.float32(N)
    got = np.exp(-R._seq_sum(p * np.log(p + np.float32(1e-10))))
    assert abs(float(got) - val) <= bar
    dropped = cnt.copy()
    dropped[idx[-1]] -= 1
    assert abs(R.perplexity(dropped, N)[0] - val) > bar or kind == "collapsed"      # collapsed: p log p is 0 at p = 1 and near it
    moved = cnt.copy()
    moved[idx[-1]] -= 1
    moved[(idx[-1] + 1) % K] += 1
    assert abs(R.perplexity(moved, N)[0] - val) > bar


# ---- element-wise kernels ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,E,K", list(C.BWD_CASES))
@pytest.mark.parametrize("has_gq,has_gl", [(True, True), (True, False), (False, True), (False, False)])
def test_vq_bwd_bar(N, E, K, has_gq, has_gl):
    i = C.bwd_inputs(N, E, K)
    gq, gl = (i["gq"] if has_gq else None), (i["gl"] if has_gl else None)
    val, bar = R.vq_bwd(gq, gl, i["z"], i["dense"], N, E, C.BETA)
    inside(R.vq_bwd_f32(gq, gl, i["z"], i["dense"], N, E, C.BETA), val, bar, "sequential float32")
    if has_gl:      # the rows of the neighbouring code gathered instead (beside g_quantized the loss term is small: some elements show it)
        wrong = i["W"][(i["idx"] + 1) % K]
        outside(R.vq_bwd(gq, gl, i["z"], wrong, N, E, C.BETA)[0], val, bar, "neighbouring code's rows gathered")
    else:
        assert not bar.any(), "without g_loss the result is g_quantized, or zero, exactly"


@pytest.mark.parametrize("E,K", list(C.CBGRAD_CASES))
def test_codebook_grad_bar(E, K):
    idx, flat = C.cbgrad_inputs(E, K)
    cnt, dw, _ = R.stats(idx, flat, K)
    assert (cnt == 0).any()
    cnt32, dw32 = cnt.astype(np.float32), dw.astype(np.float32)
    W, gl = C.codebook(K, E), np.array([C.G_LOSS], np.float32)
    val, bar = R.codebook_grad(cnt32, dw32, W, gl, C.CBGRAD_ROWS)
    inside(R.codebook_grad_f32(cnt32, dw32, W, gl, C.CBGRAD_ROWS), val, bar, "sequential float32")
    outside(val * (1 + 1e-6), val, bar, "off by 1e-6")


@pytest.mark.parametrize("K,E", C.SQNORM_CASES)
def test_code_sqnorm_bar(K, E):
    W = C.codebook(K, E)
    val, bar = R.code_sqnorm(W)
    inside(R.code_sqnorm_f32(W), val, bar, "sequential float32")
    outside(val * (1 + 4 * float(R.gamma(E + 7))), val, bar, "four bars off")


def test_straight_through_value_is_float32_and_not_q():
    z, q = C.ste_inputs(257)
    out = R.ste(z, q)
    assert out.dtype == np.float32 and not np.array_equal(out, q), "z + (q - z) rounds twice: it is not q everywhere"
    assert np.abs(out.astype(np.float64) - q) .max() <= 2 * R.U * np.abs(np.stack([z, q])).max() * 2
