"""Shapes of the GRU sequence dispatch tests (no device): the sweep of the workspace pin (tests/golden/gru_seq_workspace.npz) and
GRU_ROUTE_SHAPES -- for every route of g2v_gru_seq_route, every variant and both directions of travel a shape that selects it and
the nearest shapes that miss it.  Every row passes explicit options and cus = 256, so the answer depends on neither the bound
context nor the device.  tests/test_gru_route_host.py holds the table to the query on the CPU; tests/test_gpu_ops.py checks the
older queries against it at the device's own CU count.  GRU_F64_CASES (at the end) are the calls a device runs against float64."""
from gesture2vec_amd import _lib, ops

WORKSPACE_H = (4, 8, 50, 52, 64, 192, 196, 200, 208, 256, 260)
WSLAB_BH = ((16, 64), (37, 64), (4096, 64), (128, 200), (1, 4), (0, 64))

ROUTES = {k[len("G2V_GRU_ROUTE_"):]: v for k, v in _lib.CONSTANTS.items() if k.startswith("G2V_GRU_ROUTE_")}
FACTS = {k[len("G2V_GRU_PLAN_"):]: v for k, v in _lib.CONSTANTS.items() if k.startswith("G2V_GRU_PLAN_")}


def route_name(T, B, H, ndir=2, *, backward=False, cluster=1, resident_rows=1025, resident_bwd=1, cus=256, facts=(), **_):
    """ops.gru_route with the defaults of the table: "CLUSTER", "FAST*1", "STREAM*2", "STREAM" (variant 0: the scalar body), ...;
    "" where the call is refused"""
    return ops.gru_route(T, B, H, ndir, backward=backward, cluster=cluster, resident_rows=resident_rows, resident_bwd=resident_bwd,
                         cus=cus, facts=facts)


def _fwd(name, route, T, B, H, **kw):
    return [dict(name=name, route=route, T=T, B=B, H=H, **kw)]


def _bwd(name, route, T, B, H, **kw):
    return [dict(name=name + ", backward", route=route, T=T, B=B, H=H, backward=True, **kw)]


def _both(name, route, T, B, H, **kw):      # the same route forward and backward
    return _fwd(name, route, T, B, H, **kw) + _bwd(name, route, T, B, H, **kw)


# H = 200, two directions, 256 CUs, cluster on, resident from 1025 rows, backward too: unless the row says otherwise
GRU_ROUTE_SHAPES = tuple(
    # ---- FAST and its variants
    _both("fast", "FAST", 4, 16, 64)
    + _both("fast, one direction, large batch", "FAST", 4, 4096, 64, ndir=1)
    + _both("fast, prepared", "FAST", 4, 16, 64, facts=("PREPARED",))
    + _both("fast, projection / dx fused", "FAST*1", 4, 16, 64, facts=("FUSED",))
    + _bwd("fast, W_hh gradient fused", "FAST*2", 4, 16, 64, facts=("FUSED", "WGRAD_HH"))
    + _bwd("fast, both weight gradients fused", "FAST*3", 4, 16, 64, facts=("FUSED", "WGRAD_HH", "WGRAD_IH"))
    + _bwd("fast, both weight gradients fused, no dgi / dgh", "FAST*3", 4, 16, 64, facts=("FUSED", "WGRAD_HH", "WGRAD_IH", "NO_DGI"))
    # (FAST moves every array as float4s: it asks for STEP's list, the vector body's -- backward RESIDENT's -- and its own fused operands)
    + _both("H = 64, every list unaligned: off fast, the scalar body", "STREAM", 4, 16, 64,
            facts=("SPLIT_UNALIGNED", "VEC_UNALIGNED", "D_HN_UNALIGNED", "FAST_UNALIGNED"))
    + _both("H = 64, a split array unaligned: off fast, streaming, vector body", "STREAM*1", 4, 16, 64, facts=("SPLIT_UNALIGNED",))
    + _both("H = 64, a vector array unaligned: off fast, a cluster", "CLUSTER", 4, 16, 64, facts=("VEC_UNALIGNED",))
    + _both("H = 64, a vector array unaligned, T = 1: off fast, per step", "STEP", 1, 16, 64, facts=("VEC_UNALIGNED",))
    + _both("H = 64, a vector array unaligned, large batch: off fast, the scalar body", "STREAM", 4, 1025, 64, facts=("VEC_UNALIGNED",))
    + _fwd("H = 64, d_hn is not the forward's", "FAST", 4, 16, 64, facts=("D_HN_UNALIGNED",))
    + _bwd("H = 64, d_hn unaligned: off fast, a cluster", "CLUSTER", 4, 16, 64, facts=("D_HN_UNALIGNED",))
    + _both("H = 64, x / b_ih / dx / wslab unaligned: off fast, a cluster", "CLUSTER", 4, 16, 64, facts=("FAST_UNALIGNED",))
    + _both("H = 64, prepared, a split array unaligned: off fast", "STREAM*1", 4, 16, 64, facts=("PREPARED", "SPLIT_UNALIGNED"))
    + _both("refused: fused at H = 64, a split array unaligned", "", 4, 16, 64, facts=("FUSED", "SPLIT_UNALIGNED"))
    + _both("refused: fused at H = 64, a vector array unaligned", "", 4, 16, 64, facts=("FUSED", "VEC_UNALIGNED"))
    + _fwd("fused at H = 64: d_hn is not the forward's", "FAST*1", 4, 16, 64, facts=("FUSED", "D_HN_UNALIGNED"))
    + _bwd("refused: fused at H = 64, d_hn unaligned", "", 4, 16, 64, facts=("FUSED", "D_HN_UNALIGNED"))
    + _both("refused: fused at H = 64, x / b_ih / dx / wslab unaligned", "", 4, 16, 64, facts=("FUSED", "FAST_UNALIGNED"))
    + _bwd("refused: weight gradients at H = 64, wslab unaligned", "", 4, 16, 64, facts=("FUSED", "WGRAD_HH", "WGRAD_IH", "FAST_UNALIGNED"))
    + _bwd("refused: weight gradients at H = 64, a vector array unaligned", "", 4, 16, 64, facts=("FUSED", "WGRAD_HH", "VEC_UNALIGNED"))
    + _bwd("H = 64, quantiser backward, a vector array unaligned: the cluster serves it", "CLUSTER", 4, 16, 64, facts=("HN", "VEC_UNALIGNED"))
    + _bwd("refused: H = 64, quantiser backward, a split array unaligned", "", 4, 16, 64, facts=("HN", "SPLIT_UNALIGNED"))
    + _bwd("fast, quantiser backward", "FAST", 4, 16, 64, facts=("HN",))
    + _both("H = 64, hs_ld % 4 != 0: off fast, a cluster", "CLUSTER", 4, 16, 64, facts=("HS_LD",))
    + _bwd("H = 64, d_hs_ld % 4 != 0: off fast, a cluster", "CLUSTER", 4, 16, 64, facts=("D_HS_LD",))
    + _fwd("H = 64, d_hs_ld is not the forward's", "FAST", 4, 16, 64, facts=("D_HS_LD",))
    + _both("H = 64, hs_ld % 4 != 0, large batch: the scalar body", "STREAM", 4, 1025, 64, facts=("HS_LD",))
    # ---- CLUSTER / STEP
    + _both("cluster: 9 x 13 x 2 = 234 workgroups", "CLUSTER", 4, 144, 200)
    + _both("per-step: 10 x 13 x 2 = 260 workgroups", "STEP", 4, 160, 200)
    + _both("cluster, one direction: 19 x 13 = 247", "CLUSTER", 4, 304, 200, ndir=1)
    + _both("per-step, one direction: 20 x 13 = 260", "STEP", 4, 320, 200, ndir=1)
    + _both("cluster: T = 2", "CLUSTER", 2, 144, 200)
    + _both("per-step: T = 1", "STEP", 1, 144, 200)
    + _both("per-step: the cluster switch is off", "STEP", 4, 144, 200, cluster=0)
    + _both("per-step: eight CUs", "STEP", 4, 144, 200, cus=8)
    + _both("per-step: the cluster kernel is not resident", "STEP", 4, 144, 200, facts=("NOT_RESIDENT",))
    + _both("per-step: B = 1024", "STEP", 4, 1024, 200)
    + _both("cluster: H = 256", "CLUSTER", 4, 16, 256)
    + _both("cluster, smallest", "CLUSTER", 2, 16, 8, ndir=1)
    + _both("cluster: vector arrays unaligned changes nothing", "CLUSTER", 4, 144, 200, facts=("VEC_UNALIGNED", "D_HN_UNALIGNED"))
    + _both("split arrays unaligned: streaming, vector body", "STREAM*1", 4, 144, 200, facts=("SPLIT_UNALIGNED",))
    + _both("split arrays unaligned, resident from 512 rows", "RESIDENT", 4, 1024, 200, resident_rows=512, facts=("SPLIT_UNALIGNED",))
    + _both("resident from 512 rows, aligned: still per-step", "STEP", 4, 1024, 200, resident_rows=512)
    # ---- RESIDENT
    + _both("resident: B = 1025", "RESIDENT", 4, 1025, 200)
    + _fwd("resident forward: H = 196", "RESIDENT", 4, 1025, 196)
    + _bwd("streaming backward: H = 196", "STREAM*1", 4, 1025, 196)
    + _fwd("resident forward: H = 208", "RESIDENT", 4, 1025, 208)
    + _bwd("streaming backward: H = 208", "STREAM*1", 4, 1025, 208)
    + _both("streaming: H = 192", "STREAM*1", 4, 1025, 192)
    + _both("streaming: H = 212", "STREAM*1", 4, 1025, 212)
    + _both("streaming: resident_rows = 0", "STREAM*1", 4, 1025, 200, resident_rows=0)
    + _both("streaming: resident from 1026 rows", "STREAM*1", 4, 1025, 200, resident_rows=1026)
    + _fwd("resident forward whatever resident_bwd says", "RESIDENT", 4, 1025, 200, resident_bwd=0)
    + _bwd("streaming: resident_bwd = 0", "STREAM*1", 4, 1025, 200, resident_bwd=0)
    + _both("vector arrays unaligned: the scalar body", "STREAM", 4, 1025, 200, facts=("VEC_UNALIGNED",))
    + _fwd("d_hn is not the forward's", "RESIDENT", 4, 1025, 200, facts=("D_HN_UNALIGNED",))
    + _bwd("d_hn unaligned: streaming, vector body", "STREAM*1", 4, 1025, 200, facts=("D_HN_UNALIGNED",))
    + _both("hs_ld % 4 != 0: the scalar body", "STREAM", 4, 1025, 200, facts=("HS_LD",))
    + _bwd("d_hs_ld % 4 != 0: the scalar body", "STREAM", 4, 1025, 200, facts=("D_HS_LD",))
    + _both("resident, packed rows", "RESIDENT", 64, 1025, 200, facts=("PACKED",))
    + _fwd("resident, gathered", "RESIDENT", 4, 1025, 200, facts=("GATHERED",))
    + _fwd("resident, gathered and packed", "RESIDENT", 4, 1025, 200, facts=("GATHERED", "PACKED"))
    # ---- STREAM and its bodies
    + _fwd("streaming, two row tiles: 96 x 2 = 192 workgroups", "STREAM*2", 4, 3041, 200, resident_rows=0)
    + _fwd("streaming, one row tile: 95 x 2 = 190", "STREAM*1", 4, 3040, 200, resident_rows=0)
    + _bwd("streaming backward has one body for 3041 rows", "STREAM*1", 4, 3041, 200, resident_rows=0)
    + _fwd("streaming, two row tiles, one direction", "STREAM*2", 4, 6113, 192, ndir=1)
    + _fwd("streaming, one row tile, one direction", "STREAM*1", 4, 6112, 192, ndir=1)
    + _both("scalar body: H = 50", "STREAM", 4, 16, 50)
    + _both("scalar body: H = 50, large batch", "STREAM", 4, 6200, 50)
    + _both("scalar body: H = 260", "STREAM", 4, 16, 260)
    + _both("streaming, packed rows", "STREAM*1", 4, 1025, 200, resident_rows=0, facts=("PACKED",))
    + _fwd("scalar body: the most LDS, H = 1264", "STREAM", 2, 16, 1264)
    + _bwd("scalar body: the most LDS, H = 632", "STREAM", 2, 16, 632)
    # ---- refused
    + _fwd("refused: H = 1280 needs more than 160 KB of LDS", "", 2, 16, 1280)
    + _bwd("refused: H = 636 needs more than 160 KB of LDS", "", 2, 16, 636)
    + _fwd("refused: gathered on a cluster shape", "", 4, 144, 200, facts=("GATHERED",))
    + _fwd("refused: gathered, resident_rows = 0", "", 4, 1025, 200, resident_rows=0, facts=("GATHERED",))
    + _fwd("refused: gathered at H = 64", "", 4, 1025, 64, facts=("GATHERED",))
    + _fwd("refused: gathered at H = 192", "", 4, 1025, 192, facts=("GATHERED",))
    + _fwd("refused: gathered, vector arrays unaligned", "", 4, 1025, 200, facts=("GATHERED", "VEC_UNALIGNED"))
    + _fwd("refused: gathered, a split shape off its route by alignment", "", 4, 1024, 200, resident_rows=512,
           facts=("GATHERED", "SPLIT_UNALIGNED"))
    + _both("refused: packed at H = 64", "", 4, 16, 64, facts=("PACKED",))
    + _both("refused: packed at T = 65", "", 65, 144, 200, facts=("PACKED",))
    + _both("packed at T = 64", "CLUSTER", 64, 144, 200, facts=("PACKED",))
    + _both("refused: packed at H = 50", "", 4, 16, 50, facts=("PACKED",))
    + _both("refused: packed at H = 260", "", 4, 16, 260, facts=("PACKED",))
    + _both("refused: packed without lengths", "", 4, 144, 200, facts=("PACKED", "NO_LENGTHS"))
    + _both("no lengths, not packed", "CLUSTER", 4, 144, 200, facts=("NO_LENGTHS",))
    + _both("refused: packed on the scalar body", "", 4, 1025, 200, resident_rows=0, facts=("PACKED", "VEC_UNALIGNED"))
    + _both("refused: packed on the scalar body, hs_ld", "", 4, 1025, 200, facts=("PACKED", "HS_LD"))
    + _both("refused: fused projection / dx at H = 200", "", 4, 144, 200, facts=("FUSED",))
    + _both("refused: fused with in_dim != H", "", 4, 16, 64, facts=("FUSED", "IN_DIM"))
    + _both("refused: fused at H = 64 off fast", "", 4, 16, 64, facts=("FUSED", "HS_LD"))
    + _both("refused: workspace too small", "", 4, 144, 200, facts=("SMALL_WORKSPACE",))
    + _bwd("quantiser backward on a cluster", "CLUSTER", 2, 16, 8, ndir=1, facts=("HN",))
    + _bwd("refused: quantiser backward, a split array unaligned", "", 2, 16, 8, ndir=1, facts=("HN", "SPLIT_UNALIGNED"))
    + _bwd("refused: quantiser backward, the cluster switch is off", "", 2, 16, 8, ndir=1, cluster=0, facts=("HN",))
    + _bwd("refused: quantiser backward, T = 1", "", 1, 16, 8, ndir=1, facts=("HN",))
    + _bwd("refused: quantiser backward, the cluster kernel is not resident", "", 2, 16, 8, ndir=1, facts=("HN", "NOT_RESIDENT"))
    + _bwd("refused: quantiser backward on the resident kernel", "", 4, 1025, 200, facts=("HN",))
    + _bwd("refused: quantiser backward on the streaming kernel", "", 4, 16, 50, facts=("HN",))
    + _bwd("refused: quantiser backward without d_hn or unaligned slices", "", 4, 16, 64, facts=("HN", "HN_UNUSABLE"))
    + _bwd("refused: weight gradients on a cluster", "", 2, 16, 8, ndir=1, facts=("WGRAD_HH",))
    + _bwd("refused: weight gradients on a cluster, no dgi", "", 2, 16, 8, ndir=1, facts=("WGRAD_HH", "NO_DGI"))
    + _bwd("refused: weight gradients per step", "", 1, 16, 8, ndir=1, facts=("WGRAD_HH", "WGRAD_IH"))
    + _bwd("refused: weight gradients on the resident kernel", "", 4, 1025, 200, facts=("WGRAD_HH", "WGRAD_IH", "NO_DGI"))
    + _bwd("refused: weight gradients on the streaming kernel", "", 4, 16, 50, facts=("WGRAD_HH",))
    + _bwd("refused: weight gradients at H = 64 off fast", "", 4, 16, 64, facts=("FUSED", "WGRAD_HH", "D_HS_LD"))
    + _bwd("refused: weight gradients without dx", "", 4, 16, 64, facts=("WGRAD_HH",))
    + _bwd("refused: weight gradients, a group incomplete", "", 4, 16, 64, facts=("FUSED", "WGRAD_HH", "WGRAD_PARTIAL"))
    + _bwd("refused: dW_ih without dW_hh", "", 4, 16, 64, facts=("FUSED", "WGRAD_IH"))
    + _bwd("refused: no dgi, nothing fused", "", 4, 16, 64, facts=("NO_DGI",))
    + _bwd("refused: no dgi on a cluster", "", 2, 16, 8, ndir=1, facts=("NO_DGI",))
    + _both("rejected: T = 0", "", 0, 16, 200)
    + _both("rejected: B = 0", "", 4, 0, 200)
    + _both("rejected: H = 0", "", 4, 16, 0)
    + _both("rejected: three directions", "", 4, 16, 200, ndir=3))


# ---- GRU_F64_CASES: one case per route and variant at the smallest shape the plan admits on 256 CUs, and the nearest shapes that
# exercise an edge of its kernel.  tests/test_gpu_gru_f64.py runs every one against the float64 restatement of tests/_gru_ref.py;
# tests/test_gru_ref_host.py holds the list to the route query and to the reference's own conditions.  Two directions = forward,
# then reverse; weights scaled 1 / sqrt(H); in_dim = H.  Options of a case (all default off):
#   h0, lengths, packed, gathered; hs_ld / d_hs_ld (default H; `shared`: both directions write one (T,B,2H) buffer, ld = 2H);
#   fused (projection and dx), wgrad 1 / 2 (dW_hh / and dW_ih), no_dgi (dgi = dgh = NULL), hn, prepared; bwd = False: forward only;
#   cluster / resident_rows / resident_bwd: the scoped options;
#   unaligned: "all" = every array 4 bytes past a 16-byte boundary; "split" = only arrays of STEP's list beyond the vector body's
#   in either direction of travel (forward w_hh, h_n; backward d_hn: h0 is on the backward's vector list and stays aligned);
#   "d_hn" = d_hn alone.  The workspace stays aligned: the entry points require it.
def case_facts(case, backward):
    """the G2V_GRU_PLAN_* names of the call this case makes in one direction of travel"""
    ua, f = case.get("unaligned"), []
    hs_ld = case.get("hs_ld") or (2 * case["H"] if case.get("shared") else case["H"])
    d_hs_ld = case.get("d_hs_ld") or (2 * case["H"] if case.get("shared") else case["H"])
    f += ["PACKED"] if case.get("packed") else []
    f += ["NO_LENGTHS"] if not case.get("lengths") else []
    f += ["FUSED"] if case.get("fused") else []
    f += ["HS_LD"] if hs_ld % 4 else []
    f += ["PREPARED"] if case.get("prepared") else []
    if ua == "all":
        f += ["SPLIT_UNALIGNED", "VEC_UNALIGNED"] + (["FAST_UNALIGNED"] if case.get("fused") else [])
    if not backward:
        f += ["GATHERED"] if case.get("gathered") else []
        f += ["SPLIT_UNALIGNED"] if ua == "split" else []
        return tuple(f)
    f += ["D_HS_LD"] if d_hs_ld % 4 else []
    f += ["WGRAD_HH"] if case.get("wgrad", 0) >= 1 else []
    f += ["WGRAD_IH"] if case.get("wgrad", 0) >= 2 else []
    f += ["NO_DGI"] if case.get("no_dgi") else []
    f += ["HN"] if case.get("hn") else []
    f += ["SPLIT_UNALIGNED", "D_HN_UNALIGNED"] if ua in ("split", "d_hn") else (["D_HN_UNALIGNED"] if ua == "all" else [])
    return tuple(f)


def case_route(case, backward, cus=256):
    """route_name of the call this case makes, under the case's options (cus = 0: the device's own count)"""
    return route_name(case["T"], case["B"], case["H"], case["ndir"], backward=backward, cluster=case.get("cluster", 1),
                      resident_rows=case.get("resident_rows", 1025), resident_bwd=case.get("resident_bwd", 1), cus=cus,
                      facts=case_facts(case, backward))


def _f64(route, route_bwd, T, B, H, tag, ndir=2, **kw):
    bwd = kw.pop("bwd", route_bwd != "")
    return dict(id=f"{route}-{T}x{B}x{H}-{tag}", route=route, route_bwd=route_bwd, T=T, B=B, H=H, ndir=ndir, bwd=bwd, **kw)


GRU_F64_CASES = (
    # ---- FAST (H = 64)
    _f64("FAST", "FAST", 2, 1, 64, "smallest", ndir=1),
    _f64("FAST", "FAST", 5, 20, 64, "shared-h0-lengths", shared=True, h0=True, lengths=True, seed=0),
    _f64("FAST", "FAST", 34, 32, 64, "plain"),
    _f64("FAST*1", "FAST*1", 4, 20, 64, "fused", fused=True, h0=True, lengths=True),
    _f64("FAST*1", "FAST*2", 5, 37, 64, "wgrad-hh", fused=True, wgrad=1, lengths=True),
    _f64("FAST*1", "FAST*3", 5, 37, 64, "wgrad-hh-ih", fused=True, wgrad=2, h0=True, lengths=True),
    _f64("FAST*1", "FAST*3", 3, 16, 64, "wgrad-no-dgi", fused=True, wgrad=2, no_dgi=True),
    _f64("FAST", "FAST", 4, 16, 64, "hn", hn=True, h0=True),
    _f64("FAST", "FAST", 4, 20, 64, "prepared", prepared=True, lengths=True),
    # ---- CLUSTER
    _f64("CLUSTER", "CLUSTER", 2, 16, 8, "smallest", ndir=1),
    _f64("CLUSTER", "CLUSTER", 2, 16, 8, "reverse", ndir=1, reverse=(True,), h0=True, lengths=True),
    _f64("CLUSTER", "CLUSTER", 7, 19, 200, "h0-lengths", h0=True, lengths=True),
    _f64("CLUSTER", "CLUSTER", 34, 40, 52, "partial-tile"),
    _f64("CLUSTER", "CLUSTER", 4, 16, 256, "widest"),
    _f64("CLUSTER", "CLUSTER", 4, 16, 64, "hs_ld65", hs_ld=65, lengths=True),
    _f64("CLUSTER", "CLUSTER", 6, 40, 200, "packed", packed=True, lengths=True, h0=True),
    _f64("CLUSTER", "CLUSTER", 2, 16, 8, "hn", ndir=1, hn=True),
    # ---- STEP
    _f64("STEP", "STEP", 1, 16, 8, "one-step", ndir=1, h0=True),
    _f64("STEP", "STEP", 1, 144, 200, "one-step", h0=True, lengths=True),
    _f64("STEP", "STEP", 4, 19, 52, "cluster-off", cluster=0, h0=True, lengths=True),
    _f64("STEP", "STEP", 4, 160, 200, "260-workgroups"),
    _f64("STEP", "STEP", 4, 160, 200, "packed", packed=True, lengths=True),
    # ---- RESIDENT
    _f64("RESIDENT", "RESIDENT", 3, 1025, 200, "h0-lengths", h0=True, lengths=True),
    _f64("RESIDENT", "STREAM*1", 2, 1025, 196, "H196"),
    _f64("RESIDENT", "STREAM*1", 2, 1025, 208, "H208", lengths=True),
    _f64("RESIDENT", "RESIDENT", 3, 1025, 200, "packed", packed=True, lengths=True),
    _f64("RESIDENT", "", 3, 1025, 200, "gathered", gathered=True, lengths=True),
    _f64("RESIDENT", "", 3, 1025, 200, "gathered-packed", gathered=True, packed=True, lengths=True, h0=True),
    _f64("RESIDENT", "STREAM*1", 3, 1025, 200, "resident_bwd0", resident_bwd=0, lengths=True),
    # ---- STREAM: the scalar body
    _f64("STREAM", "STREAM", 3, 16, 50, "H50", h0=True, lengths=True),
    _f64("STREAM", "STREAM", 3, 17, 50, "H50-ragged", lengths=True),
    _f64("STREAM", "STREAM", 3, 16, 260, "H260", h0=True),
    _f64("STREAM", "", 2, 16, 1264, "most-lds", bwd=False, h0=True),
    _f64("STREAM", "STREAM", 2, 16, 632, "most-lds", h0=True, lengths=True),
    _f64("STREAM", "STREAM", 3, 1025, 200, "hs_ld201", hs_ld=201, lengths=True),
    # ---- STREAM: the vector body, one and two row tiles
    _f64("STREAM*1", "STREAM*1", 4, 1025, 192, "H192", h0=True, lengths=True),
    _f64("STREAM*1", "STREAM*1", 3, 1025, 200, "packed", resident_rows=0, packed=True, lengths=True),
    _f64("STREAM*2", "STREAM*1", 2, 3041, 200, "two-row-tiles", resident_rows=0, h0=True, lengths=True),
    _f64("STREAM*1", "STREAM*1", 2, 3040, 200, "one-row-tile", resident_rows=0),
    # ---- calls whose arrays are only 4-byte aligned
    _f64("STREAM", "STREAM", 3, 16, 200, "unaligned", unaligned="all", h0=True, lengths=True),
    _f64("STREAM", "STREAM", 3, 1025, 200, "unaligned", unaligned="all", lengths=True),
    _f64("STREAM", "STREAM", 4, 20, 64, "unaligned", unaligned="all", h0=True, lengths=True),
    _f64("STREAM*1", "STREAM*1", 4, 144, 200, "split-unaligned", unaligned="split", h0=True, lengths=True),
    _f64("RESIDENT", "STREAM*1", 3, 1024, 200, "split-unaligned", unaligned="split", resident_rows=512, h0=True),
    _f64("RESIDENT", "STREAM*1", 3, 1025, 200, "d_hn-unaligned", unaligned="d_hn", lengths=True),
)
# cases that share a shape do not share their inputs; seed 0 of the shared-buffer case has a row of its ragged second row tile that
# ends inside the sequence, which the planted defects of tests/test_gru_ref_host.py need
GRU_F64_CASES = tuple(dict(c, seed=c.get("seed", i)) for i, c in enumerate(GRU_F64_CASES))
assert len({c["id"] for c in GRU_F64_CASES}) == len(GRU_F64_CASES)
