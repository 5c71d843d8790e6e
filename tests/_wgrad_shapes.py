"""Shapes of the weight-gradient tests (no torch, no device): the sweep of the workspace pin (tests/golden/wgrad_workspace.npz) and
WGRAD_ROUTE_SHAPES, one call description per route of g2v_linear_bwd_weight_route -- and per variant of a route's launch -- at
the smallest shape that selects it, with the route it must select.  tests/test_wgrad_plan_host.py holds the table to the query
on the CPU; tests/test_gpu_ops.py runs every entry."""
from gesture2vec_amd import _lib

WORKSPACE_M = (1, 15, 16, 100, 511, 512, 640, 2560, 4095, 4096, 4097, 4111, 4112, 4113, 4127, 4128, 5000, 8192, 8197, 17408, 33825,
               139264, 139269)
WORKSPACE_KN = ((64, 192), (135, 64), (64, 135), (64, 64), (200, 600), (40, 200), (45, 600), (600, 514), (300, 600), (128, 512),
                (128, 128), (400, 512), (50, 150), (3, 5), (64, 2100), (200, 200))

ROUTES = {k[len("G2V_WGRAD_ROUTE_"):]: v for k, v in _lib.CONSTANTS.items() if k.startswith("G2V_WGRAD_ROUTE_")}


def route_name(M, K, N, *, nprob=1, bf16x3=False, keep=False, row_map=None, dual=False, lddy=None, ldx=None, align=16, **_):
    """g2v_linear_bwd_weight_route as names: "WAVE", "WAVE|RAGGED_TAIL", ...; "" where the call would be refused.  `align`: torch
    allocations are 16-byte aligned, which is what every test here hands over."""
    r = _lib.load().g2v_linear_bwd_weight_route(M, K, N, nprob, _lib.WGRAD_BF16X3 if bf16x3 else 0, int(keep), int(row_map is not None),
                                                int(dual), N if lddy is None else lddy, K if ldx is None else ldx, align)
    tail, main = r & ROUTES["RAGGED_TAIL"], r & ~ROUTES["RAGGED_TAIL"]
    names = [k for k, v in ROUTES.items() if v == main and k != "RAGGED_TAIL"] + (["RAGGED_TAIL"] if tail else [])
    return "|".join(names)


def _case(name, route, M, K, N, **kw):
    return dict(name=name, route=route, M=M, K=K, N=N, **kw)


# row_map=(B, T): x is a (B, T, K) tensor read in (T, B) row order, M = T * B.  ldx: x is (M, ldx) with K columns used.
WGRAD_ROUTE_SHAPES = (
    _case("one tile", "SMALL_TILE", 37, 50, 150),
    _case("one tile, row-mapped", "SMALL_TILE", 3 * 13, 45, 70, row_map=(13, 3)),
    _case("16 waves", "SMALL_WAVES16", 512, 40, 200),
    _case("masked", "SMALL_MASKED", 128, 200, 600, keep=True),
    _case("LDS-staged, XCD placement", "SMALL_LDS", 512, 200, 600, nprob=2),
    _case("LDS-staged, plain grid", "SMALL_LDS", 512, 200, 600, nprob=3),
    _case("register-tiled, XCD placement", "SMALL_RT", 512, 200, 600, nprob=2, ldx=201),
    _case("register-tiled, plain grid", "SMALL_RT", 512, 200, 600, nprob=3, ldx=201),
    _case("wave 192x64, 8-byte loads", "WAVE", 4096, 64, 192),
    _case("wave 192x64, dword loads", "WAVE", 4096, 64, 192, ldx=65),
    _case("wave 64x135", "WAVE", 4096, 135, 64),
    _case("wave 135x64", "WAVE", 4096, 64, 135),
    _case("wave 64x64", "WAVE", 4096, 64, 64),
    _case("wave 192x64, bf16x3", "WAVE", 4096, 64, 192, bf16x3=True),
    _case("wave 64x135, row-mapped", "WAVE", 4096, 135, 64, row_map=(128, 32)),
    _case("two addends", "WAVE_DUAL", 4096, 135, 64, dual=True),
    _case("two addends, row-mapped", "WAVE_DUAL", 4096, 135, 64, dual=True, row_map=(128, 32)),
    _case("output-blocked 192x64", "WAVE_GEN", 4096, 64, 514),
    _case("output-blocked 128x112", "WAVE_GEN", 4096, 200, 600),
    _case("output-blocked, row-mapped", "WAVE_GEN", 4096, 40, 200, row_map=(1024, 4)),
    _case("LDS-tiled, 64 columns", "LDS_TILED", 4100, 64, 64),
    _case("LDS-tiled, 128 columns", "LDS_TILED", 4100, 64, 128),
    _case("LDS-tiled, 192 columns", "LDS_TILED", 4100, 64, 192),
    _case("LDS-tiled, bf16x3 below 4096 rows", "LDS_TILED", 600, 50, 150, bf16x3=True),
    _case("ragged", "WAVE|RAGGED_TAIL", 4113, 64, 192),
    _case("ragged, row-mapped", "WAVE|RAGGED_TAIL", 33 * 129, 135, 64, row_map=(129, 33)),
    _case("ragged, output-blocked", "WAVE_GEN|RAGGED_TAIL", 4113, 200, 600),
)
