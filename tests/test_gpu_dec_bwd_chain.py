"""The persistent backward rollout (csrc/dec_persist.hip, dec_persist_bwd_kernel) keeps the hidden-side products dgh1 W_hh1 and
dgh0 W_hh0 of a step off the chain from one publish to the next: they run inside the NEXT iteration's exchange, from the gate
tiles the step left in LDS, and after the last step they become dh_init.  Each chain keeps its order, so the kernel with and
without the fused W_hh1 weight gradient (<true> / <false>) must agree bit for bit, run to run, and with the per-step kernels up
to the summation order of the BatchNorm sums.  Shapes: D = 135, H = 64 (the kernel is specialised); B = 32 is two workgroups and
a one-hop exchange, B = 272 is 17 workgroups and two hops with a short last row; T = 2 has exactly one full iteration (the
pending products run in the final exchange only), T = 3 one iteration with pending products in front of it."""
import pytest
import torch

from test_gpu_ops import DEV, _alloc_saved, _dec_state, _dec_weight_tensors, ops, relclose  # noqa: F401  (ops: fixture)

pytestmark = pytest.mark.gpu

D, H, G = 135, 64, 192
CASES = [(B, T, p, 1, True) for B in (32, 272) for T in (2, 3, 5) for p in (0.0, 0.2)]
CASES.append((272, 5, 0.2, 2, False))      # teacher-forced prefix, unconditioned: no feedback product anywhere


@pytest.mark.parametrize("B,T,p,n_pre,conditioned", CASES)
def test_dec_bwd_hidden_products_off_the_chain(ops, B, T, p, n_pre, conditioned):
    from gesture2vec_amd import _lib
    lib = _lib.load()
    sd = _dec_state(D, H, seed=31)
    g = torch.Generator().manual_seed(11 + B + T)
    target = torch.randn(B, T, D, generator=g).to(DEV)
    h_init = (torch.randn(2, B, H, generator=g) * 0.5).to(DEV)
    k95 = (torch.rand(T - 1, B, D, generator=g) < 0.05).to(torch.uint8).to(DEV)
    kl0 = (torch.rand(T - 1, B, H, generator=g) < (1 - p)).to(torch.uint8).to(DEV) if p > 0 else None
    gy = (torch.randn(T, B, D, generator=g) / (T * B * D) * 100).to(DEV)
    nblk = ops.dec_rollout_blocks(B)
    z = lambda *s: torch.zeros(*s, device=DEV)
    assert lib.g2v_dec_rollout_bwd_fuses_wgrad(B, D, H) == 8

    wt, _ = _dec_weight_tensors(sd, DEV)
    ws = ops.dec_weights_struct(wt)
    saved = _alloc_saved(T, B, D, H, nblk, DEV, p)
    ops.dec_rollout_fwd(target, h_init, ws, saved, k95, kl0, p, n_pre, conditioned, True, T, B, D, H)
    torch.cuda.synchronize()

    def bwd(persistent, fused):
        grads = {"dy": gy.clone(), "du": z(T - 1, B, H), "dbn": z(T - 1, B, H), "dgi0": z(T - 1, B, G), "dgh0": z(T - 1, B, G),
                 "dgi1": z(T - 1, B, G), "dgh1": z(T - 1, B, G), "dh_init": z(2, B, H), "d_bn_w": z(H), "d_bn_b": z(H),
                 "bn_bwd_partial": z(2, nblk, 2, H)}
        dw, db = z(G, H), z(G)
        if fused:
            grads["dw_gru"], grads["db_gru"] = [None, None, None, dw], [None, None, None, db]
        with _lib.Context.current().scoped(persistent=int(persistent)):
            ops.dec_rollout_bwd(ws, saved, grads, k95, kl0, p, n_pre, conditioned, T, B, D, H)
        torch.cuda.synchronize()
        assert lib.g2v_dec_rollout_persist_fault(0) == 0
        # dbn is scratch of the per-step kernels only; the fused kernel never writes dgh1
        out = {k: v for k, v in grads.items() if torch.is_tensor(v) and k not in ("bn_bwd_partial", "dbn") and not (fused and k == "dgh1")}
        return out, dw, db

    (fw, dw, db), (nf, _, _), (ps, _, _), (fw2, dw2, db2) = bwd(True, True), bwd(True, False), bwd(False, False), bwd(True, True)
    assert set(nf) == {"dy", "du", "dgi0", "dgh0", "dgi1", "dgh1", "dh_init", "d_bn_w", "d_bn_b"}
    for k in fw:
        assert torch.isfinite(fw[k]).all(), k
        assert torch.equal(fw[k], nf[k]), f"with / without the fused weight gradient: {k} differs"
        assert torch.equal(fw[k], fw2[k]), f"persistent backward not reproducible: {k}"
    assert torch.equal(dw, dw2) and torch.equal(db, db2), "fused weight gradient not reproducible"
    for k in nf:
        relclose(nf[k], ps[k], 2e-4, f"persistent vs per-step backward: {k}")
    M = (T - 1) * B
    dw_ref, db_ref = ops.linear_bwd_weight(ps["dgh1"].view(M, G), saved["h1"][:-1].reshape(M, H).contiguous(), G, H)
    relclose(dw, dw_ref, 2e-5, "fused dW_hh1")
    relclose(db, db_ref, 2e-5, "fused db_hh1")
