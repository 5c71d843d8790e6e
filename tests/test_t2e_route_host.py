"""CPU-only: the code decoder's dispatch plan (csrc/t2e_rollout.hip code_route_plan) through g2v_attn_code_rollout_route, the two
older *_ok queries against it, and the three size queries pinned to what the library returned before the dispatch moved into the
plan (tests/golden/t2e_route_sizes.npz).  T2E_ROUTE_SHAPES (tests/_t2e_route_shapes.py) names, for every route, variant and
direction, a shape that selects it and the nearest shapes that miss it.  No kernel is launched."""
import os

import numpy as np
import pytest

import _t2e_route_shapes as TS
from gesture2vec_amd import _lib, ops


def test_size_queries_are_pinned(golden_dir):
    fx = np.load(os.path.join(golden_dir, "t2e_route_sizes.npz"))
    lib = _lib.load()
    for key, query, sweep in (("fwd", lib.g2v_attn_code_rollout_fwd_workspace, TS.FWD_HKA), ("bwd", lib.g2v_attn_code_rollout_bwd_workspace, TS.BWD_ARGS),
                              ("bptt", lib.g2v_code_cluster_bptt_workspace, TS.BPTT_BH)):
        assert tuple(map(tuple, fx[key + "_args"])) == sweep, "the sweep moved: record again"
        assert fx[key].shape == (len(sweep),)
        for args, want in zip(sweep, fx[key]):
            assert query(*args) == int(want), (key, args)
    # the shipped dims by hand: the forward's cluster records at 256 / 13 + 1 = 20 row groups of H = 200 (Hp = 208, nt = 13) outweigh
    # its fragment images; the BPTT's partial products at B = 128
    assert int(fx["fwd"][TS.FWD_HKA.index((200, 512, 0))]) == 2 * 20 * ((3 * 16 + 2) * 208 + 13 * 32) * 8 + 20 * 13 * 4 + 16
    assert int(fx["bptt"][TS.BPTT_BH.index((128, 200))]) == 8 * 4 * 13 * 16 * 208 * 8 + 8 * 13 * 4 + 16
    assert all(int(v) == 0 for a, v in zip(TS.BWD_ARGS, fx["bwd"]) if a[0] == 0) and all(int(v) > 0 for a, v in zip(TS.BWD_ARGS, fx["bwd"]) if a[0] > 0)


@pytest.mark.parametrize("case", TS.T2E_ROUTE_SHAPES, ids=lambda c: c["name"])
def test_shape_selects_its_named_route(case):
    assert TS.routes(case) == case["route"]


def test_route_table_names_every_constant_of_the_header_in_both_directions():
    calls = [c for c in TS.T2E_ROUTE_SHAPES if not c["bptt"]]
    for d in (0, 1):
        assert {c["route"][d].split("*")[0] for c in calls if c["route"][d]} == set(TS.ROUTES)
        assert any(c["route"][d] == "" for c in calls)
    assert {c["route"] for c in calls} >= {("CLUSTER", "CLUSTER"), ("CLUSTER", "CHAIN"), ("CLUSTER", "STEP"), ("STEP", "STEP"), ("STEP", "STEP*1"),
                                           ("CHAIN", "CHAIN"), ("", "")}
    assert {c["route"] for c in TS.T2E_ROUTE_SHAPES if c["bptt"]} == {("CLUSTER",), ("",)}
    assert TS.ROUTES == {"CLUSTER": 1, "STEP": 2, "CHAIN": 3}
    assert TS.FACTS == {"ENTRY": 1, "NO_CLUSTER_FWD": 2, "NO_CLUSTER_BPTT": 4, "WS_SMALL": 8}
    assert {f for c in TS.T2E_ROUTE_SHAPES for f in c["facts"]} == set(TS.FACTS)
    assert len({c["name"] for c in TS.T2E_ROUTE_SHAPES}) == len(TS.T2E_ROUTE_SHAPES)


def test_the_two_directions_of_one_call_are_consistent():
    """STEP goes with STEP, CHAIN with CHAIN, a refusal with a refusal; a forward CLUSTER with STEP exactly where the fused pair's row
    count is reached (or the entry itself is called), else with CLUSTER or, the cluster BPTT not accepted, with CHAIN."""
    for c in TS.T2E_ROUTE_SHAPES:
        if c["bptt"]:
            continue
        fwd, bwd = c["route"]
        if fwd in ("STEP", "CHAIN", ""):
            assert bwd.split("*")[0] == fwd and (bwd == "STEP*1") == (fwd == "STEP" and c["att"]), c["name"]
        else:
            pair = "ENTRY" in c["facts"] or c["B"] >= c["fused_min_rows"]
            assert fwd == "CLUSTER" and bwd == ("STEP" if pair else "CHAIN" if "NO_CLUSTER_BPTT" in c["facts"] else "CLUSTER"), c["name"]


def test_route_is_a_function_of_its_arguments_alone():
    """persistent = -1 reads the bound context's level; any other value and every cus > 0 make the answer independent of the context
    and of the device -- which is what lets this file run without one."""
    kw = dict(fused_min_rows=1024, cus=256)
    with _lib.Context.current().scoped(persistent=0):
        assert ops.code_route(3, 16, 48, 40, **kw) == "CHAIN" and ops.code_route(3, 16, 48, 40, persistent=1, **kw) == "CLUSTER"
        assert ops.code_route(3, 16, 48, 40, backward=True, persistent=1, **kw) == "CLUSTER"
    with _lib.Context.current().scoped(persistent=1):
        assert ops.code_route(3, 16, 48, 40, **kw) == "CLUSTER" and ops.code_route(3, 16, 48, 40, persistent=0, **kw) == "CHAIN"
    for c in TS.T2E_ROUTE_SHAPES[::7]:
        assert TS.routes(c) == TS.routes(c) == c["route"]
    lib = _lib.load()
    assert lib.g2v_attn_code_rollout_route(3, 3, 16, 48, 40, 0, 0, 2, 0, 1, 256, 0) == 0 and lib.g2v_attn_code_rollout_route(-1, 3, 16, 48, 40, 0, 0, 2, 0, 1, 256, 0) == 0


# ---- the conditions of the two older queries, written out as they stood before the plan -----------------------------------------
def _fwd_lds_floats(H, Hin, Tw, scratch):
    Hp = (H + 15) & ~15
    ldh, ldx = Hp + 4, ((Hin + 15) & ~15) + 4
    return 5 * 16 * ldh + 16 * ldx + 2 * Hp + 2 * Hp + scratch + 8 * 16 + 8 * 16 + 16 + 16 * (Tw if Tw > 0 else 1)


def _bwd_lds_floats(H, K):
    Hp = (H + 15) & ~15
    ldh, ldg, ldk = Hp + 4, ((3 * H + 15) & ~15) + 4, ((K + 15) & ~15) + 4
    return 16 * max(ldk, 2 * ldh) + 2 * 16 * ldg + 3 * 16 * ldh


def rollout_ok_as_it_stood(S1, B, H, K, Tw, att):
    if S1 < 1 or B < 1 or H < 16 or (H & 3) or H > 256 or K < 4 or (K & 3) or K > 1024:
        return False
    if att and (Tw < 1 or Tw > 64):
        return False
    Hin, Hp = (2 * H if att else H), (H + 15) & ~15
    if att and (2 * Hp + 1024 > 16 * (((3 * H + 15) & ~15) + 4) or 2 * 16 * Tw > 16 * (Hp + 4)):
        return False
    return _fwd_lds_floats(H, Hin, Tw if att else 0, 1024) * 4 <= 160 * 1024 and _bwd_lds_floats(H, K) * 4 <= 160 * 1024


def cluster_ok_as_it_stood(S1, B, H, K, att, level, cus):
    if att or S1 < 1 or B < 1 or H < 16 or (H & 3) or H > 16 * 13 or K < 4 or (K & 3):
        return False
    nt, nblk = (H + 15) >> 4, (B + 15) >> 4
    if ((K + 15) >> 4) > 3 * nt or nt * nblk > cus:
        return False
    return level != 0


SWEEP_S1, SWEEP_B = (0, 1, 3), (0, 1, 16, 24, 304, 305, 320, 1024, 1376, 4096)
SWEEP_H, SWEEP_K = (12, 16, 20, 48, 50, 64, 200, 208, 212, 224, 228, 256, 260), (0, 4, 40, 42, 144, 148, 512, 624, 628, 688, 692, 1024, 1028)
SWEEP_TW_ATT = ((0, 0), (0, 1), (1, 1), (5, 1), (26, 1), (27, 1), (64, 1), (65, 1))


def older_queries_are_fields_of_the_route(cus, levels):
    """For every level: the bound context's answers of g2v_attn_code_rollout_ok / _cluster_ok equal the conditions as they stood and
    the route query of the call each describes.  cus: what the library's own CU query says here (0 without a device)."""
    lib = _lib.load()
    n = 0
    for level in levels:
        with _lib.Context.current().scoped(persistent=level):
            for S1 in SWEEP_S1:
                for B in SWEEP_B:
                    for H in SWEEP_H:
                        for K in SWEEP_K:
                            for Tw, att in SWEEP_TW_ATT:
                                ok, cl = rollout_ok_as_it_stood(S1, B, H, K, Tw, att), cluster_ok_as_it_stood(S1, B, H, K, att, level, cus)
                                assert lib.g2v_attn_code_rollout_ok(S1, B, H, K, Tw, att) == int(ok), (S1, B, H, K, Tw, att)
                                assert lib.g2v_attn_code_rollout_cluster_ok(S1, B, H, K, att) == int(cl), (level, S1, B, H, K, att)
                                # no input serves the cluster kernel that the step kernels do not: the forward entry asks both
                                assert ok or not cl
                                r = ops.code_route(S1, B, H, K, Tw, att, facts=("ENTRY",))
                                assert (r != "") == ok and (r == "CLUSTER") == cl, (level, S1, B, H, K, Tw, att, r)
                                n += 1
    return n


def test_older_queries_are_fields_of_the_route():
    """Without a device the library's CU count is 0 and no grid fits; tests/test_gpu_text2embedding.py repeats this on one, over the
    route table's shapes."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 0
    assert older_queries_are_fields_of_the_route(cus, (0, 1)) == 2 * 3 * 10 * 13 * 13 * 8
    # ... and with the CU count passed in, the same conditions describe the route at any count
    for cus in (64, 256):
        for B in SWEEP_B:
            for H in SWEEP_H:
                for K in SWEEP_K:
                    want = rollout_ok_as_it_stood(3, B, H, K, 0, 0) and cluster_ok_as_it_stood(3, B, H, K, 0, 1, cus)
                    assert (ops.code_route(3, B, H, K, persistent=1, cus=cus, facts=("ENTRY",)) == "CLUSTER") == want, (cus, B, H, K)
