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
