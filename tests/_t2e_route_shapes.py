"""Shapes of the code decoder's dispatch tests (no torch, no device): the sweeps of the size-query pin
(tests/golden/t2e_route_sizes.npz) and T2E_ROUTE_SHAPES -- for every route and variant of g2v_attn_code_rollout_route, in both
directions, a shape that selects it and the nearest shapes that miss it.  Every row passes the level and the CU count explicitly.
tests/test_t2e_route_host.py holds the table to the query on the CPU; tests/test_gpu_text2embedding.py checks the older queries
against it at the device's own CU count."""
import itertools

from gesture2vec_amd import _lib

# the size queries' sweeps: (H, K, attention), (S1, B, H, K, Tw, attention), (B, H)
FWD_HKA = tuple(itertools.product((16, 48, 64, 100, 200, 208, 212, 256, 300), (4, 40, 512, 624, 1024), (0, 1)))
BWD_ARGS = tuple((S1, B, H, K, Tw, att) for S1, B, H, K, (Tw, att) in itertools.product(
    (0, 1, 3, 9), (1, 16, 24, 128, 305, 1024, 4096), (48, 200, 256), (40, 512), ((0, 0), (1, 1), (20, 1), (64, 1))))
BPTT_BH = tuple(itertools.product((1, 16, 17, 128, 304, 305, 1024, 4096), (16, 48, 200, 208, 212, 256)))

ROUTES = {k[len("G2V_CODE_ROUTE_"):]: v for k, v in _lib.CONSTANTS.items() if k.startswith("G2V_CODE_ROUTE_")}
FACTS = {k[len("G2V_CODE_PLAN_"):]: v for k, v in _lib.CONSTANTS.items() if k.startswith("G2V_CODE_PLAN_")}

_ARGS = ("S1", "B", "H", "K", "Tw", "att", "layers", "fused_min_rows", "persistent", "cus", "facts")


def route_name(S1, B, H, K, Tw=0, att=False, *, backward=0, layers=2, fused_min_rows=1024, persistent=1, cus=256, facts=()):
    """g2v_attn_code_rollout_route as ops.code_route names it, every argument explicit"""
    r = _lib.load().g2v_attn_code_rollout_route(int(backward), S1, B, H, K, Tw, int(att), layers, fused_min_rows, persistent, cus,
                                                sum(FACTS[f] for f in facts))
    name = [k for k, v in ROUTES.items() if v == (r & 0xff)][0] if r else ""
    return name + (f"*{r >> 8}" if r >> 8 else "")


def routes(case):
    """(forward, backward) route names of a call row; (g2v_code_cluster_bptt's own,) of a `bptt` row"""
    kw = {k: case[k] for k in _ARGS}
    if case.get("bptt"):
        return (route_name(backward=2, **kw),)
    return route_name(backward=0, **kw), route_name(backward=1, **kw)


def _case(name, route, B, H, K=40, *, S1=3, Tw=0, att=False, layers=2, fused_min_rows=1024, persistent=1, cus=256, facts=(), bptt=False):
    route = tuple(route.split("/"))
    assert len(route) == (1 if bptt else 2)
    return dict(name=name, route=route, S1=S1, B=B, H=H, K=K, Tw=Tw, att=att, layers=layers, fused_min_rows=fused_min_rows,
                persistent=persistent, cus=cus, facts=facts, bptt=bptt)


_ATT = dict(Tw=5, att=True)
T2E_ROUTE_SHAPES = (
    # ---- below the fused pair's row count, no attention: the cluster pair while the grid has a CU per workgroup
    _case("cluster pair, smallest", "CLUSTER/CLUSTER", 16, 48),
    _case("cluster pair, one row", "CLUSTER/CLUSTER", 1, 16, 4, S1=1),
    _case("cluster pair, shipped dims", "CLUSTER/CLUSTER", 128, 200, 512),
    _case("cluster pair, H = 200 up to the CU count", "CLUSTER/CLUSTER", 304, 200, 512),
    _case("chain: H = 200, the grid no longer fits", "CHAIN/CHAIN", 305, 200, 512),
    _case("cluster pair, H = 208 up to the CU count", "CLUSTER/CLUSTER", 304, 208, 512),
    _case("chain: H = 208, the grid no longer fits", "CHAIN/CHAIN", 320, 208, 512),
    _case("64 CUs: chain at H = 200, B = 304", "CHAIN/CHAIN", 304, 200, 512, cus=64),
    _case("64 CUs: chain at H = 200, B = 305", "CHAIN/CHAIN", 305, 200, 512, cus=64),
    _case("64 CUs: chain at H = 208, B = 304", "CHAIN/CHAIN", 304, 208, 512, cus=64),
    _case("64 CUs: chain at H = 208, B = 320", "CHAIN/CHAIN", 320, 208, 512, cus=64),
    _case("64 CUs: cluster pair up to four row groups", "CLUSTER/CLUSTER", 64, 200, 512, cus=64),
    _case("64 CUs: chain at five row groups", "CHAIN/CHAIN", 65, 200, 512, cus=64),
    _case("cluster pair, K tiles = 3 nt at H = 200", "CLUSTER/CLUSTER", 16, 200, 624),
    _case("chain: one K tile over at H = 200", "CHAIN/CHAIN", 16, 200, 628),
    _case("cluster pair, K tiles = 3 nt at H = 48", "CLUSTER/CLUSTER", 16, 48, 144),
    _case("chain: one K tile over at H = 48", "CHAIN/CHAIN", 16, 48, 148),
    _case("cluster pair, H = 208", "CLUSTER/CLUSTER", 16, 208),
    _case("chain: H = 212", "CHAIN/CHAIN", 16, 212),
    _case("chain: H % 4 != 0", "CHAIN/CHAIN", 16, 50),
    _case("chain: H = 12", "CHAIN/CHAIN", 16, 12),
    _case("chain: K % 4 != 0", "CHAIN/CHAIN", 16, 48, 42),
    _case("chain: level 0", "CHAIN/CHAIN", 16, 48, persistent=0),
    _case("cluster pair, level 2", "CLUSTER/CLUSTER", 16, 48, persistent=2),
    _case("chain: the cluster forward not accepted", "CHAIN/CHAIN", 16, 48, facts=("NO_CLUSTER_FWD",)),
    _case("cluster forward, chain behind it: the cluster BPTT not accepted", "CLUSTER/CHAIN", 16, 48, facts=("NO_CLUSTER_BPTT",)),
    _case("chain: three layers", "CHAIN/CHAIN", 16, 48, layers=3),
    _case("chain: one layer, large batch", "CHAIN/CHAIN", 2048, 48, layers=1),
    _case("refused: cluster pair with a workspace below the query's", "/", 16, 48, facts=("WS_SMALL",)),
    _case("chain needs no workspace", "CHAIN/CHAIN", 16, 212, facts=("WS_SMALL",)),
    # ---- attention: nothing below the row count but the chain
    _case("chain: attention below the row count", "CHAIN/CHAIN", 24, 48, **_ATT),
    _case("chain: attention, shipped dims", "CHAIN/CHAIN", 128, 200, 512, Tw=20, att=True),
    # ---- from fused_min_rows rows: the fused pair; its entry takes the cluster forward wherever the grid fits
    _case("fused pair, shipped dims at the row count", "STEP/STEP", 1024, 200, 512),
    _case("chain: one row below the row count", "CHAIN/CHAIN", 1023, 200, 512),
    _case("fused pair with attention", "STEP/STEP*1", 1024, 200, 512, Tw=20, att=True),
    _case("chain: attention one row below the row count", "CHAIN/CHAIN", 1023, 200, 512, Tw=20, att=True),
    _case("cluster forward of the fused pair: H = 48 at the row count", "CLUSTER/STEP", 1024, 48),
    _case("cluster pair: H = 48 one row below the row count", "CLUSTER/CLUSTER", 1023, 48),
    _case("fused pair: H = 48, the grid no longer fits", "STEP/STEP", 1376, 48),
    _case("cluster forward of the fused pair: lowered row count", "CLUSTER/STEP", 16, 48, fused_min_rows=16),
    _case("cluster pair one row below the lowered row count", "CLUSTER/CLUSTER", 15, 48, fused_min_rows=16),
    _case("cluster forward of the fused pair: row count 1", "CLUSTER/STEP", 16, 48, fused_min_rows=1),
    _case("... which no switch but the level turns off", "CLUSTER/STEP", 16, 48, fused_min_rows=1, facts=("NO_CLUSTER_FWD", "NO_CLUSTER_BPTT")),
    _case("fused pair: row count 1, level 0", "STEP/STEP", 16, 48, fused_min_rows=1, persistent=0),
    _case("fused pair: row count 1, H = 212", "STEP/STEP", 16, 212, fused_min_rows=1),
    _case("fused pair: row count 1, one K tile over", "STEP/STEP", 16, 48, 148, fused_min_rows=1),
    _case("fused pair: row count 1, 64 CUs", "STEP/STEP", 65, 200, 512, fused_min_rows=1, cus=64),
    _case("fused pair with attention: row count 1", "STEP/STEP*1", 24, 48, fused_min_rows=1, **_ATT),
    _case("chain: row count 1, three layers", "CHAIN/CHAIN", 16, 48, fused_min_rows=1, layers=3),
    _case("chain: row count 1, H % 4 != 0", "CHAIN/CHAIN", 16, 50, fused_min_rows=1),
    _case("refused: fused pair with a workspace below the query's", "/", 1024, 200, 512, facts=("WS_SMALL",)),
    # ---- the C entries themselves: no row-count rule, no chain
    _case("entry: cluster forward, step backward", "CLUSTER/STEP", 16, 48, facts=("ENTRY",)),
    _case("entry: level 0", "STEP/STEP", 16, 48, persistent=0, facts=("ENTRY",)),
    _case("entry: the grid no longer fits", "STEP/STEP", 305, 200, 512, facts=("ENTRY",)),
    _case("entry: H = 212", "STEP/STEP", 16, 212, facts=("ENTRY",)),
    _case("entry: H = 224 at the LDS bound", "STEP/STEP", 16, 224, facts=("ENTRY",)),
    _case("entry: attention", "STEP/STEP*1", 24, 48, facts=("ENTRY",), **_ATT),
    _case("entry: attention, Tw = 64", "STEP/STEP*1", 24, 200, 512, Tw=64, att=True, facts=("ENTRY",)),
    _case("entry: attention, smallest H", "STEP/STEP*1", 24, 20, Tw=5, att=True, facts=("ENTRY",)),
    _case("entry: attention, Tw fills the tile it borrows at H = 48", "STEP/STEP*1", 24, 48, Tw=26, att=True, facts=("ENTRY",)),
    _case("entry: H = 200 at the LDS bound", "STEP/STEP", 16, 200, 688, facts=("ENTRY",)),
    _case("entry refused: S1 = 0", "/", 16, 48, S1=0, facts=("ENTRY",)),
    _case("entry refused: B = 0", "/", 0, 48, facts=("ENTRY",)),
    _case("entry refused: K = 1028", "/", 16, 48, 1028, facts=("ENTRY",)),
    _case("entry refused: H = 260", "/", 16, 260, facts=("ENTRY",)),
    _case("entry refused: H % 4 != 0", "/", 16, 50, facts=("ENTRY",)),
    _case("entry refused: Tw = 65", "/", 24, 200, 512, Tw=65, att=True, facts=("ENTRY",)),
    _case("entry refused: attention without encoder steps", "/", 24, 48, Tw=0, att=True, facts=("ENTRY",)),
    _case("entry refused: attention at H = 16 has no tile to borrow", "/", 24, 16, Tw=5, att=True, facts=("ENTRY",)),
    _case("entry refused: Tw = 27 at H = 48", "/", 24, 48, Tw=27, att=True, facts=("ENTRY",)),
    _case("entry refused: H = 200, K = 692 needs more than 160 KB of LDS", "/", 16, 200, 692, facts=("ENTRY",)),
    _case("entry refused: H = 228 needs more than 160 KB of LDS", "/", 16, 228, facts=("ENTRY",)),
    _case("entry refused: three layers", "/", 16, 48, layers=3, facts=("ENTRY",)),
    _case("entry refused: workspace too small", "/", 16, 48, facts=("ENTRY", "WS_SMALL")),
    _case("chain where the entries refuse: S1 = 0", "CHAIN/CHAIN", 16, 48, S1=0),
    _case("chain where the entries refuse: K = 1028", "CHAIN/CHAIN", 2048, 48, 1028),
    _case("chain where the entries refuse: Tw = 65", "CHAIN/CHAIN", 2048, 200, 512, Tw=65, att=True),
    _case("chain where the entries refuse: the LDS bound", "CHAIN/CHAIN", 2048, 200, 692),
    # ---- g2v_code_cluster_bptt called by itself: the grid rule alone
    _case("bptt: smallest", "CLUSTER", 16, 48, bptt=True),
    _case("bptt: K, Tw, layers and the row count are not read", "CLUSTER", 16, 48, 0, Tw=99, layers=7, fused_min_rows=1, bptt=True),
    _case("bptt: H = 200 up to the CU count", "CLUSTER", 304, 200, bptt=True),
    _case("bptt refused: the grid no longer fits", "", 305, 200, bptt=True),
    _case("bptt refused: 64 CUs", "", 65, 200, cus=64, bptt=True),
    _case("bptt refused: H = 212", "", 16, 212, bptt=True),
    _case("bptt refused: H % 4 != 0", "", 16, 50, bptt=True),
    _case("bptt refused: level 0", "", 16, 48, persistent=0, bptt=True),
    _case("bptt refused: S1 = 0", "", 16, 48, S1=0, bptt=True),
    _case("bptt refused: workspace too small", "", 16, 48, facts=("WS_SMALL",), bptt=True),
)


# ---- CODE_F64_CASES: the calls tests/test_gpu_code_rollout_f64.py holds to the float64 restatement of tests/_code_ref.py, and
# tests/test_code_ref_host.py to the conditions of that reference.  Each names the forward and backward route the ENTRY must select
# at its level on 256 CUs (route_name(..., facts=("ENTRY",))).  kind "pair": g2v_attn_code_rollout_fwd, then (training)
# g2v_attn_code_rollout_bwd on the arrays it saved; with bptt also g2v_code_cluster_bptt on them, fed dh_top = d_logits W_out formed
# in float64.  S1 = 2 or 3; 4 where n_pre = 3 must leave a free-running step; 1 at the smallest shape.
# emb_drop False: keep_emb = NULL.  deferred: also run with bn_running_* = NULL and commit with g2v_bn_running_update_invstd.
# tie = (k1, k2, gain, lift): tests/_code_ref.py.  The seed of a case is the first at which tests/_code_ref.py's admissible() holds
# (_CODE_SEEDS; 0 where it is not listed).
_CODE_SEEDS = {}


def _f64(tag, route, B, H, K=40, *, S1=2, Tw=0, att=False, level=1, p=0.0, n_pre=1, training=True, emb_drop=True, deferred=False,
         bptt=False, tie=None):
    fwd, bwd = route.split("/")
    cid = f"{fwd}-{B}x{H}x{K}" + (f"xTw{Tw}" if att else "") + f"-{tag}"
    return dict(id=cid, route=fwd, route_bwd=bwd if training else "", S1=S1, B=B, H=H, K=K, Tw=Tw, att=att, level=level, p=p, n_pre=n_pre,
                training=training, emb_drop=emb_drop, deferred=deferred, bptt=bptt and training, tie=tie, seed=_CODE_SEEDS.get(cid, 0))


_S, _A, _C = "STEP/STEP", "STEP/STEP*1", "CLUSTER/STEP"
CODE_F64_CASES = (
    # ---- STEP / STEP, no attention: level 0, or a shape off the cluster grid at level 1
    _f64("one-row", _S, 1, 16, 4, S1=1, level=0),                           # B = 1 in training: variance 0
    _f64("plain", _S, 16, 48, S1=3, level=0, deferred=True),
    _f64("npre0", _S, 17, 48, S1=3, level=0, n_pre=0),                      # a second row group holding one row
    _f64("drop", _S, 33, 48, S1=3, level=0, p=0.2),                         # a third row group holding one row
    _f64("no-keep-emb", _S, 16, 20, level=0, emb_drop=False),               # H = 20 padded to 32
    _f64("drop", _S, 24, 200, 512, level=0, p=0.2),                         # H = 200 padded to 208
    _f64("npre3", _S, 16, 212, S1=4, n_pre=3),                              # H = 212: STEP at every level
    _f64("lds-bound", _S, 16, 224),                                         # the backward's LDS carve at its 160 KB bound in H
    _f64("lds-bound", _S, 16, 200, 688),                                    # ... and in K at H = 200
    _f64("forced", _S, 16, 48, 44, level=0, n_pre=9),                       # n_pre = S1 + 7: every step is fed from `codes`
    _f64("second-pass-one-tile", _S, 16, 48, 528),                          # out layer: 33 K tiles, 32 per pass
    _f64("second-pass-full", _S, 16, 48, 1024),                             # ... 64 K tiles
    _f64("one-k-tile-over", _S, 16, 48, 148),                               # ceil(K / 16) = 3 nt + 1: off the cluster grid
    # reduce_partials' 16-row unrolled loop (csrc/common.hpp) runs where a row segment holds per = ceil(nblk / nseg) >= 16 row
    # groups, nseg = min(threads, scratch / 4) / (2H / 4).  At H = 224 (112 float4 columns, the fewest segments a served H has):
    # code_step_fwd_kernel has 512 threads and, at every served shape, the 2048-float scratch (ct_scratch: its carve stays under
    # 160 KB - 8 KB), so nseg = 4 and per >= 16 from nblk = 61; code_bn_bwd_apply_kernel has 256 threads and 1024 floats, nseg = 2,
    # per >= 16 from nblk = 31.  B = 961 = 60 * 16 + 1 gives nblk = 61: per = 16 forward (three full segments, one of 13), per = 31
    # backward (16 unrolled + 15), and a last row group of one row.  (The 1024-float scratch the plan can hand the step kernels is
    # taken by the attention backward only, at H = 20, where 10 float4 columns leave nseg = 25.)
    _f64("unrolled-reduce", _S, 961, 224),
    _f64("eval", _S, 16, 48, S1=3, level=0, training=False),
    # ---- STEP / STEP*1: attention
    _f64("plain", _A, 24, 48, S1=3, Tw=5, att=True, deferred=True),
    _f64("one-position", _A, 24, 48, Tw=1, att=True),
    _f64("tw-fills-the-tile", _A, 24, 48, Tw=26, att=True),
    _f64("tw-max", _A, 24, 200, 512, Tw=64, att=True),
    _f64("smallest-h", _A, 24, 20, Tw=5, att=True),
    _f64("ragged", _A, 7, 48, Tw=5, att=True),
    _f64("drop-npre2", _A, 24, 48, S1=3, Tw=5, att=True, p=0.2, n_pre=2),
    # ---- CLUSTER forward through the entry at level 1, the STEP backward and the cluster BPTT behind it on the arrays it saved
    _f64("plain", _C, 16, 48, S1=3, deferred=True, bptt=True),
    _f64("one-row", _C, 1, 16, 4, S1=1, bptt=True),
    _f64("shipped-dims", _C, 17, 200, 512, bptt=True),
    _f64("h52", _C, 16, 52, bptt=True),
    _f64("h208", _C, 16, 208, bptt=True),
    _f64("k-tiles-3nt", _C, 16, 48, 144, bptt=True),
    _f64("k-tiles-3nt", _C, 16, 200, 624, bptt=True),
    _f64("largest-grid", _C, 304, 200, 512, bptt=True),                     # 13 x 19 workgroups
    _f64("npre3", _C, 16, 48, S1=4, n_pre=3, bptt=True),
    _f64("eval", _C, 16, 48, S1=3, training=False),
    # ---- ... with inter-layer dropout, over the same H / B set
    _f64("drop", _C, 16, 48, S1=3, p=0.2, bptt=True),
    _f64("one-row-drop", _C, 1, 16, 4, S1=1, p=0.2, bptt=True),
    _f64("drop", _C, 17, 200, p=0.2, bptt=True),
    _f64("drop", _C, 16, 52, p=0.2, bptt=True),
    _f64("drop", _C, 16, 208, p=0.2, bptt=True),
    _f64("drop", _C, 304, 200, p=0.2, bptt=True),
    # ---- a tie per forward kernel: codes 3 and 21 sit in different K tiles, which different waves (step) and different workgroups
    # (cluster) reduce; the pair is preferred at the free-running steps
    _f64("tie", _S, 16, 48, S1=3, level=0, tie=(3, 21, 3.0, 0.75)),
    _f64("tie", _C, 16, 48, S1=3, tie=(3, 21, 3.0, 0.75)),
)
