"""Child process of tests/test_gpu_launch_order.py: a fresh process, so that no earlier call has raised any kernel's LDS mark in the
launch ledger (csrc/launch_ledger.hpp).  For every kernel family whose dynamic LDS depends on the call's shape and can pass the
no-reservation limit it calls ONE kernel instance three times -- a shape below the limit, one above it, the small
one again -- and holds every call to the family's own test: the test functions and helpers of the existing GPU tests are imported
and called, not restated.  Then the same order on a kernel that used to reserve a compile-time maximum once (silhouette_samples).

Prints "ok <family> <step>" per call and stops at the first failure (exit status 1, traceback on stderr)."""
import math
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import pytest  # noqa: E402
import torch  # noqa: E402

import _dec_chain_ref as CR  # noqa: E402
import _vq_route_shapes as VS  # noqa: E402
import test_gpu_dec_chain as DC  # noqa: E402
import test_gpu_dec_rollout_f64 as DF  # noqa: E402
import test_gpu_ops as T  # noqa: E402
import test_gpu_silhouette as SIL  # noqa: E402
import test_gpu_soft_quantiser as SQ  # noqa: E402
import test_gpu_t2e_latent as TL  # noqa: E402
import test_gpu_text2embedding as TE  # noqa: E402
import test_gpu_vae_latent as V  # noqa: E402
from _dec_route_shapes import route_name as dec_route_name  # noqa: E402
from _f64 import as64, default64  # noqa: E402
from gesture2vec_amd import _lib, generate, ops  # noqa: E402
from oracle import g2v_oracle as O  # noqa: E402

DEV = T.DEV
LIMIT = 48 * 1024      # g2v::LDS_NO_RESERVE_LIMIT


# ---- GRU BPTT, the scalar streaming body (gru_seq_bwd_kernel<0>): H % 4 != 0 keeps both shapes off the split, cluster, resident and
# vector routes.  LDS = 16 ((ceil16(3 H) + 4) + (ceil16(H) + 4)) floats: 8.7 KB at H = 30, 52.7 KB at H = 202.  test_gru_seq's recipe
# and bars (tests/test_gpu_ops.py), the oracle run in float64.
def gru_bptt(H, Tn=2, B=16, I=24):
    c16 = lambda n: (n + 15) & ~15
    lds = 16 * ((c16(3 * H) + 4) + (c16(H) + 4)) * 4
    assert ops.gru_route(Tn, B, H) == "STREAM" and ops.gru_route(Tn, B, H, backward=True) == "STREAM", "not the scalar streaming bodies"
    x = T.rnd(Tn, B, I, seed=31)
    w_ih, w_hh = T.rnd(3 * H, I, seed=32, scale=0.2), T.rnd(3 * H, H, seed=33, scale=1 / math.sqrt(H))
    b_ih, b_hh = T.rnd(3 * H, seed=34, scale=0.1), T.rnd(3 * H, seed=35, scale=0.1)
    g_out, g_hn = T.rnd(Tn, B, H, seed=37), T.rnd(B, H, seed=38)
    with default64():
        leaves = [t.double().requires_grad_(True) for t in (x, w_ih, w_hh, b_ih, b_hh)]
        out_ref, hn_ref = O.gru_direction(*leaves, False, None)
        grads_ref = torch.autograd.grad((out_ref * as64(g_out)).sum() + (hn_ref * as64(g_hn)).sum(), leaves)
    gi = ops.linear_fwd(x.to(DEV), w_ih.to(DEV), b_ih.to(DEV))
    hs, h_n, gates = ops.gru_seq_fwd(gi, w_hh.to(DEV), b_hh.to(DEV), Tn, B, H)
    T.relclose(hs, out_ref, 2e-5, "gru hs")
    T.relclose(h_n, hn_ref, 2e-5, "gru h_n")
    dgi, dgh, _ = ops.gru_seq_bwd(g_out.to(DEV), H, g_hn.to(DEV), hs, H, None, gates, w_hh.to(DEV), Tn, B, H)
    dx = ops.linear_bwd_data(dgi, w_ih.to(DEV))
    dw_ih, db_ih = ops.linear_bwd_weight(dgi, x.to(DEV), 3 * H, I)
    hprev = torch.zeros(Tn, B, H, device=DEV)
    hprev[1:] = hs[:-1]
    dw_hh, db_hh = ops.linear_bwd_weight(dgh, hprev, 3 * H, H)
    for name, got, ref in (("dx", dx.reshape(Tn, B, I), grads_ref[0]), ("dW_ih", dw_ih, grads_ref[1]), ("dW_hh", dw_hh, grads_ref[2]),
                           ("db_ih", db_ih, grads_ref[3]), ("db_hh", db_hh, grads_ref[4])):
        T.relclose(got, ref, 5e-5, "gru " + name)
    return lds


# ---- the generic decoder step kernels dec_step_fwd_kernel<0, 0> / dec_step_bwd_kernel<0, 0> at persistent level 0, B = 16, T = 3:
# (D, H) = (16, 30) is 13 KB + scratch forward, (135, 200) is 80 KB + scratch.  (H % 4 != 0: the small shape is no split shape.)
# tests/test_gpu_dec_rollout_f64.py's test on a case of ours: it asserts the route both ways, then every array against float64.
def dec_step(D, H):
    case = dict(id=f"STEP-3x16x{D}x{H}-order", variant="plain", T=3, B=16, D=D, H=H, p=0.0, n_pre=1, conditioned=1, training=1, level=0,
                unaligned=False, route="STEP", route_bwd="STEP", seed=0)
    DF.test_dec_rollout_matches_float64_on_its_route(ops, case)


# ---- the latent step kernels (t2e_latent.hip): E = 2 H; H = 32 stays below the limit, H = 200 is above it both ways.  The test
# asserts that the fused kernels served the call and holds them to the float64 restatement.
def latent_step(H):
    mp = pytest.MonkeyPatch()
    try:
        TL.test_fused_latent_kernels_match_per_operator_path_and_restatement(16, H, 2, 1, 0.0, mp)
    finally:
        mp.undo()


# ---- the code step kernels (t2e_rollout.hip: code_step_fwd_kernel, code_bptt_kernel; with attention code_step_bwd_att_kernel).
# Their rollout feeds greedy codes back, and the family's own test holds it to the per-operator path on the same weights, not to
# float64: that test is what runs here (it asserts the plan, STEP / STEP*1).
def code_step(att, H, K):
    mp = pytest.MonkeyPatch()
    try:
        TE.test_fused_step_kernels_match_per_operator_path(att, 0.0, 16, 1, H, K, mp)
    finally:
        mp.undo()


# ---- code assignment.  vq_assign_kernel / vq_assign_split_kernel: 16 (ceil16(E) + 4) + 164 floats, above the limit from E = 753.
# vq_assign_p_kernel<NR, NT>: 16 NR (E + 4) + ... floats; two row tiles pass the limit from E = 368, four from E = 176, one never
# does (its plan stops at E = 608: 40 KB).
def vq_rows(route, N, E, K):
    assert ops.vq_route("ROWS", "FULL", N, E, K) == route
    T.test_vq_assign_vs_oracle(ops, N, E, K)


def vq_packed(nr, N, E, K):
    assert VS.route("ROWS", "FULL", N, E, K, facts=("ENTRY",)) == f"PACKED*{nr}"
    T.test_vq_assign_packed_kernel_equals_the_generic_kernel_bitwise(ops, N, E, K)


# ---- vq_soft_fused_fwd_kernel / _bwd_kernel through K: 25 KB / 34 KB at K = 128, 50 KB / 82 KB at K = 512
def vq_soft(case):
    SQ.test_fused_kernels_match_float64(ops, case)


# ---- vae_latent_fwd_kernel<16> / _bwd_kernel<16>: 2 x 16 (E + 4) / 3 x 16 (E + 4) floats: 8.7 / 13 KB at E = 64, 52 / 78 KB at E = 400
VAE_REFS = V.block_refs.__wrapped__()


def vae_latent(E):
    V.test_kernels_against_float64(VAE_REFS, 16, E, 0.37)


# ---- dec_chain_kernel<4, false>: 5 x 16 (ceil16(H) + 4) + 3 x 16 (ceil16(D) + 4) floats: 13 KB at (D, H) = (24, 8), 53 KB at (160, 64)
CHAIN_CASES = {D: CR.case(2, 3, 1, 16, D, H, seed=31, ids="random", tag="order") for D, H in ((24, 8), (160, 64))}
CR.CASES.extend(CHAIN_CASES.values())      # (tests/_dec_chain_ref.py looks a case up by its id; this process only)


def dec_chain(D):
    DC.test_chain_matches_float64(generate, CHAIN_CASES[D], "chain")


# ---- a kernel that used to reserve its compile-time maximum once and now reserves what it launches: sil_tile_kernel,
# 64 (ceil16(E) + 4) + 4608 floats: 23 KB at E = 16, 150 KB at its largest admitted E = 512
def silhouette(E):
    SIL.test_shapes_against_float64(E, 2, 17)


FAMILIES = [      # name, the call, its argument tuples: below the limit, above it
    ("gru_seq_bwd_scalar_stream", gru_bptt, (30,), (202,)),
    ("dec_step_generic", dec_step, (16, 30), (135, 200)),
    ("latent_step", latent_step, (32,), (200,)),
    ("code_step", code_step, ("False", 48, 40), ("False", 200, 512)),
    ("code_step_attention", code_step, ("True", 48, 40), ("True", 200, 512)),
    ("vq_assign_generic", vq_rows, ("GENERIC", 100, 16, 16), ("GENERIC", 100, 768, 16)),
    ("vq_assign_split", vq_rows, ("SPLIT*2", 40, 16, 128), ("SPLIT*2", 40, 768, 128)),
    ("vq_assign_packed_2_tiles", vq_packed, (2, 8192, 16, 16), (2, 8192, 400, 16)),
    ("vq_assign_packed_4_tiles", vq_packed, (4, 32768, 16, 16), (4, 32768, 176, 16)),
    ("vq_soft_fused", vq_soft, ("1x128x128",), ("16x128x512",)),
    ("vae_latent", vae_latent, (64,), (400,)),
    ("dec_chain", dec_chain, (24,), (160,)),
    ("silhouette_samples", silhouette, (16,), (512,)),
]


def main():
    assert _lib.load().g2v_device_ok() == 1, "no gfx950 device visible"
    assert dec_route_name(3, 16, 16, 30, persistent=0, cus=0) == dec_route_name(3, 16, 135, 200, persistent=0, cus=0) == "STEP"
    for name, call, small, large in FAMILIES:
        for step, args in (("small", small), ("large", large), ("small again", small)):
            try:
                r = call(*args)
                torch.cuda.synchronize()
            except BaseException:      # (pytest.skip / pytest.fail raise BaseException subclasses: neither is a pass here)
                traceback.print_exc()
                print(f"FAILED {name} {step} {args}", flush=True)
                return 1
            if call is gru_bptt:      # (the one formula restated here: the pair does straddle the limit)
                assert (r > LIMIT) == (step == "large"), (r, step)
            print(f"ok {name} {step}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
