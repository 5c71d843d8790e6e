"""The kernels every training step ends in -- custom_loss (its two register kernels, the generic one and the finalize), the MSE
pair, sumsq + clip_adam (csrc/misc.hip) and the cross-entropy pair (csrc/seq2seq.hip) -- against float64 restatements of the
operations (tests/_loss_inputs.py), at the sizes where their tiling has edges: one column, a partial / an exactly full / a barely
started workgroup, both sides of the compile-time T, D = 1, more than 256 partials for the finalize, the capped grids (n > 2^20),
sizes under one wave, K = 1 / 63 / 64 / 65, a strided logits array and an offset gradient view.

Array outputs (dy, the cross-entropy gradient, Adam's p / m / v): e_kernel <= min(max(8 e32, floor), cap), built from the reference
alone.  Scalars (loss terms, MSE loss, gnorm, cross-entropy loss): an a-priori bound counted from the kernels' summation trees.
The MSE gradient: per element.  All of it in tests/_loss_inputs.py.  Every test prints e_kernel, e32, their ratio and the bound.

Largest figures on the MI355X (case, e_kernel, e32 where the bound is built from it):
  arrays, e_kernel / e32, margin 8:
    custom_loss dy 2.44 (5x20x135-s1000, 1.1e-7, 4.3e-8); on the planted zero columns at most 1.2e-7 (300x34x1-g3, bound 1.4e-6)
    Adam p 1.47 (1025-gs0.125-zero-init, 1.7e-7, 1.2e-7)   m 1.07 (100003-gs0.125-zero-first, 9.2e-8, 8.6e-8)
    Adam v 1.37 (100003-gs0.125-clipped, 2.3e-7, 1.7e-7)   cross-entropy gradient 1.00 (3x512, 6.4e-8, 6.4e-8)
  scalars, e_kernel / a-priori bound:
    custom_loss l1 0.052 (7x9x40-g3, 9.4e-8)   cont 0.047 (4096x6x135-g3, 9.5e-8)   var 0.044 (7x9x40-g3, 7.0e-8)
    custom_loss mse 0.055 (4096x6x135-g3, 1.2e-7)   total 0.062 (7x9x40-g3, 1.2e-7 of |l1| + |cont| + |var|)
    MSE loss 0.062 (3145733-g0.25, 1.4e-7)   gnorm 0.071 (100003-gs0.125-clipped, 6.3e-8)
    cross-entropy loss 0.132 (4x64, 2.5e-4 absolute on a mean of 2503.5)
  MSE dy: worst element 2.67 u of the 4 u counted (63-g0.25).
Every scalar sits under a seventh of its a-priori bound: the bounds count the worst case of every rounding, the sums behave like
random walks.  One check failed on the code as it stood and was fixed in the kernel; the test that caught it says how
(test_cross_entropy_matches_float64).
"""
import math

import pytest
import torch

import _loss_inputs as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    from gesture2vec_amd import ops as o
    return o


def _bitwise_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _poison(*sizes):
    """NaN into blocks of the sizes the wrappers are about to take from the caching allocator with torch.empty (terms, partials,
    dy): a kernel that leaves part of them unwritten, or reads them before writing, shows as NaN instead of passing on zero pages"""
    blocks = [torch.full((max(int(s), 1),), NAN, device=DEV) for s in sizes for _ in range(2)]
    del blocks


# ================================================================================================ custom_loss
def _custom_loss(ops, name, weights=None, want_grad=True):
    c = L.CL_CASES[name]
    out, tgt = L.cl_inputs(name)
    y = out.transpose(0, 1).contiguous().to(DEV)                 # the kernels take y as (T,B,D), the target as (B,T,D)
    _poison(5, 4 * L.cl_blocks(c.B, c.D), out.numel())
    terms, dy = ops.custom_loss_fwd_bwd(y, tgt.to(DEV), *(weights or c.weights), g_scale=c.g_scale, want_grad=want_grad)
    return terms, dy


@pytest.mark.parametrize("name", list(L.CL_CASES))
def test_custom_loss_matches_float64(ops, name):
    """terms[0..4] and every element of dy (no sign pinned, nothing excluded: the sign of a difference of two fp32 numbers is exact),
    the planted zero column on its own, want_grad=False, a second run, and weights (0, 0, 0): the evaluation script's call"""
    c = L.CL_CASES[name]
    ref, e32, sb = L.cl_reference(name), L.cl_noise(name), L.cl_scalar_bounds(c)
    terms, dy = _custom_loss(ops, name)
    terms2, dy2 = _custom_loss(ops, name)
    terms_ng, none = _custom_loss(ops, name, want_grad=False)
    terms_w0, dy_w0 = _custom_loss(ops, name, weights=(0.0, 0.0, 0.0))
    torch.cuda.synchronize()
    assert none is None and _bitwise_equal(terms, terms2) and _bitwise_equal(dy, dy2), "two runs differ"
    assert _bitwise_equal(terms, terms_ng), "want_grad=False changes the terms"
    t = terms.cpu()
    for j, k in enumerate(("l1", "cont", "var", "mse"), start=1):
        L.check_scalar("custom_loss", name, k, t[j], ref[k], sb[k], e32[k])
    L.check_scalar("custom_loss", name, "total", t[0], ref["total"], sb["total"], e32["total"], scale=L.cl_total_scale(ref))
    got = dy.transpose(0, 1).cpu()                               # (B,T,D)
    L.check_array("custom_loss", name, "dy", got, ref["dy"])
    pl = L.cl_planted(c)
    if pl:
        # the zero column: g_scale * loss_grad_const of its signs, no norm term; against float64 on the column's own magnitude
        b, d = pl["zero_col"]
        col, rcol = got[b, :, d], ref["dy"][b, :, d]
        assert bool(torch.isfinite(col).all()) and float(col.abs().min()) > 0
        ez = L.relerr(col, rcol)
        print(f"custom_loss {name} dy on the zero column: e_kernel {ez:.3e} bound {L.bound(name, 'dy'):.3e}")
        assert ez <= L.bound(name, "dy")
    # weights (0, 0, 0): terms[0..3] vanish, terms[4] is still the MSE, the gradient is zero
    t0 = terms_w0.cpu()
    assert bool((t0[:4] == 0).all()) and bool((dy_w0 == 0).all())
    assert _bitwise_equal(terms_w0[4:], terms[4:])


# ================================================================================================ MSE
@pytest.mark.parametrize("name", list(L.MSE_CASES))
def test_mse_matches_float64(ops, name):
    n, gs = L.MSE_CASES[name]
    y, t = L.mse_inputs(name)
    ref = L.mse_reference(name)
    yd, td = y.to(DEV), t.to(DEV)
    runs = []
    for want_grad in (True, True, False):
        _poison(1, L.mse_blocks(n), n)
        runs.append(ops.mse_fwd_bwd(yd, td, want_grad, gs))
    torch.cuda.synchronize()
    (loss, dy), (loss2, dy2), (loss_ng, none) = runs
    assert none is None and _bitwise_equal(loss, loss2) and _bitwise_equal(dy, dy2) and _bitwise_equal(loss, loss_ng)
    e32 = abs(float(L.mse(y, t, gs, torch.float32)["loss"]) - float(ref["loss"])) / float(ref["loss"])
    L.check_scalar("mse", name, "loss", loss.cpu()[0], ref["loss"], L.mse_loss_bound(n), e32)
    # dy[e] = (2 g_scale / n) (y[e] - t[e]): a fixed chain of MSE_DY_ROUNDINGS roundings, so the bound holds for every element
    got, r = dy.cpu().double(), ref["dy"]
    assert bool(torch.isfinite(got).all())
    excess = (got - r).abs() - L.gamma(L.MSE_DY_ROUNDINGS) * r.abs()
    worst = float(((got - r).abs() / r.abs().clamp_min(1e-300)).max())
    print(f"mse {name} dy: worst element {worst / L.U:.2f} u, bound {L.MSE_DY_ROUNDINGS} u")
    assert float(excess.max()) <= 0.0, (name, worst)


# ================================================================================================ clip + Adam
@pytest.mark.parametrize("name", list(L.ADAM_CASES))
def test_clip_adam_matches_float64(ops, name):
    """ADAM_STEPS steps: m, v, p, every step's gnorm and the step counter; partial and gnorm_out start as NaN.
    The reference runs at the betas the ABI carries (tests/_loss_inputs.py: BETAS_ABI)."""
    c = L.ADAM_CASES[name]
    p0, grads = L.adam_inputs(name)
    ref, e32 = L.adam_reference(name), L.adam_noise(name)
    assert ops.adam_blocks(c.n) == L.adam_blocks(c.n)
    p, m, v = p0.to(DEV), torch.zeros(c.n, device=DEV), torch.zeros(c.n, device=DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    partial = torch.full((ops.adam_blocks(c.n),), NAN, device=DEV)
    gn = torch.full((1,), NAN, device=DEV)
    gd = grads.to(DEV)
    gnorms, after_first = [], None
    for k in range(L.ADAM_STEPS):
        ops.clip_adam_step(p, gd[k], m, v, step, partial, gn, L.MAX_NORM, c.grad_scale, L.LR, *L.BETAS, L.EPS)
        gnorms.append(gn.clone())
        if k == 0:
            after_first = (p.clone(), m.clone(), v.clone())
    torch.cuda.synchronize()
    assert int(step.item()) == ref["step"] == L.ADAM_STEPS
    for k in range(L.ADAM_STEPS):
        r = float(ref["gnorm"][k])
        if r == 0.0:
            assert float(gnorms[k]) == 0.0
        else:
            L.check_scalar("clip_adam", name, f"gnorm[{k}]", gnorms[k].cpu()[0], r, L.gnorm_bound(c.n), e32["gnorm"])
    if c.regime == "zero-first":      # an all-zero gradient: m = v = 0, denom = eps, and the parameters do not move by a bit
        assert _bitwise_equal(after_first[0], p0.to(DEV)) and bool((after_first[1] == 0).all()) and bool((after_first[2] == 0).all())
    for k, got in (("m", m), ("v", v), ("p", p)):
        L.check_array("clip_adam", name, k, got.cpu(), ref[k])


# ================================================================================================ cross entropy
@pytest.mark.parametrize("name", list(L.CE_CASES))
def test_cross_entropy_matches_float64(ops, name):
    """the contiguous call, and the same through a strided logits array (ld = K + 5, the gap NaN) whose first rows are not part of
    the call, writing into a row-offset view of a larger gradient array: functional.cross_entropy's skip_rows route.
    Regression: the gradient was exp(z - lse) with lse = mx + log s rounded at its own magnitude; the row around +5000 (half an
    ulp of lse: 2.4e-4) put the gradient 8.5e-5 off at (4, 64), 5.9e-5 at (5, 63), 2.1e-5 at (257, 400), 1.5e-5 at (4099, 512),
    and the +-80 row 8.8e-7 at (6, 65), against bounds of 4.2e-7 to 3.4e-6.  It is exp(z - mx) / s now (csrc/seq2seq.hip: ce_kernel)."""
    M, K = L.CE_CASES[name]
    z, t = L.ce_inputs(name)
    ref, e32 = L.ce_reference(name), L.ce_noise(name)
    zd, td = z.to(DEV), t.to(DEV)
    _poison(1, M, M * K)
    loss, dl = ops.cross_entropy_fwd_bwd(zd, td)
    loss_ng, none = ops.cross_entropy_fwd_bwd(zd, td, want_grad=False)
    skip, ld = 2, K + 5
    wide = torch.full((skip + M, ld), NAN, device=DEV)
    wide[skip:, :K] = zd
    big = torch.full((skip + M + 3, K), NAN, device=DEV)
    _poison(1, M)
    loss_s, dl_s = ops.cross_entropy_fwd_bwd(wide[skip:, :K], td, ld=ld, dl_out=big[skip:skip + M])
    torch.cuda.synchronize()
    assert none is None and _bitwise_equal(loss, loss_ng)
    assert _bitwise_equal(loss, loss_s) and _bitwise_equal(dl, dl_s), "the strided / offset call differs from the contiguous one"
    assert dl_s.data_ptr() == big[skip:].data_ptr()
    assert bool(torch.isnan(big[:skip]).all()) and bool(torch.isnan(big[skip + M:]).all()), "wrote outside its rows"
    L.check_scalar("cross_entropy", name, "loss", loss.cpu()[0], ref["loss"], L.ce_loss_bound(name), e32["loss"], scale=1.0)
    L.check_array("cross_entropy", name, "ce_grad", dl.cpu(), ref["grad"])
    pl = L.ce_planted(M, K)
    if pl:
        r = pl["far_target"]
        g = dl.cpu()[r, int(t[r])]
        assert abs(float(g) + 1.0 / M) <= 2 * L.U / M              # -gcoef: gcoef = 1.0f / float(M), one rounding
        assert math.isfinite(float(loss)) and float(loss) > 1e4 / M
