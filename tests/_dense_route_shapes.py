"""Shapes of the dense forward / data-gradient dispatch tests (no torch, no device): DENSE_ROUTE_SHAPES -- for every route, variant
and form of g2v_linear_route a call at the smallest shape that selects it, and the nearest calls that miss it, with the route each
must select.  Every row passes smallm_rows explicitly (1024 unless it says otherwise), so the answer does not depend on the bound
context.  tests/test_dense_route_host.py holds the table to the query on the CPU; tests/test_gpu_ops.py runs every entry."""
from gesture2vec_amd import _lib, ops

ROUTES = {k[len("G2V_DENSE_ROUTE_"):]: v for k, v in _lib.CONSTANTS.items() if k.startswith("G2V_DENSE_ROUTE_")}
FORMS = {k[len("G2V_DENSE_FORM_"):]: v for k, v in _lib.CONSTANTS.items() if k.startswith("G2V_DENSE_FORM_")}
ALIGN = {k[len("G2V_DENSE_ALIGN_"):]: v for k, v in _lib.CONSTANTS.items() if k.startswith("G2V_DENSE_ALIGN_")}
ROW_COUNTS = (1024, 4096, 16384)      # the row counts of the rule besides smallm_rows (STREAM, K4, the fused pair)


def strides(K, row_map):
    """row_map = (B, T): x is a (B, T, K) tensor read in (T, B) row order, M = T * B -> (rows_inner, stride_outer, stride_inner)"""
    return None if row_map is None else (row_map[0], K, row_map[1] * K)


def route(form, M, K, N, *, N_b=0, act=0, bias=True, keep=False, row_map=None, ldx=None, ldy=None, smallm_rows=1024, x_offset=0, **_):
    """ops.linear_route with the defaults of the table.  x_offset: x is a view that starts that many floats into its allocation."""
    return ops.linear_route(form, M, K, N, N_b=N_b, act=act, bias=bias, keep=keep, row_map=strides(K, row_map), ldx=ldx, ldy=ldy,
                            smallm_rows=smallm_rows, unaligned=("X",) if x_offset % 4 else ())


def _case(name, want, form, M, K, N, **kw):
    return dict(name=name, route=want, form=form, M=M, K=K, N=N, **kw)


DENSE_ROUTE_SHAPES = (
    # ---- SMALLM: one wave per output tile, up to smallm_rows rows
    _case("wave tiles 16 x 16", "SMALLM*1", "FWD", 128, 200, 600),
    _case("wave tiles 16 x 32: 2432 tiles", "SMALLM*2", "FWD", 1024, 200, 600),
    _case("wave tiles 16 x 64: 8316 tiles", "SMALLM*4", "FWD", 1000, 64, 2100),
    _case("wave tiles, keep mask", "SMALLM*1", "FWD", 128, 200, 600, keep=True),
    _case("wave tiles, tanh, no bias", "SMALLM*1", "FWD", 24, 48, 144, act=2, bias=False),
    _case("wave tiles, data gradient", "SMALLM*1", "BWD_DATA", 128, 200, 600),
    _case("wave tiles, data gradient, contraction over 2100", "SMALLM*1", "BWD_DATA", 1000, 64, 2100),
    _case("wave tiles, data gradient, 16 x 32", "SMALLM*2", "BWD_DATA", 1024, 600, 200),
    _case("K % 4 != 0: off the wave tiles", "TILED*1", "FWD", 200, 135, 64),
    _case("ldx % 4 != 0: off the wave tiles", "TILED*1", "FWD", 128, 200, 600, ldx=201),
    _case("x one float into its allocation: off the wave tiles", "TILED*1", "FWD", 128, 200, 600, x_offset=1),
    _case("smallm_rows + 1 rows: off the wave tiles", "TILED*4", "FWD", 1025, 200, 600),
    _case("smallm_rows + 1 rows, data gradient", "TILED*4", "BWD_DATA", 1025, 200, 600),
    _case("a lowered smallm_rows", "TILED*4", "FWD", 128, 200, 600, smallm_rows=127),
    # ---- STREAM: the four shapes of the streaming kernel, from 1024 rows
    _case("stream 64 -> 192", "STREAM*12x4", "FWD", 1024, 64, 192, smallm_rows=512),
    _case("stream 192 -> 64", "STREAM*4x12", "FWD", 1024, 192, 64, smallm_rows=512),
    _case("stream 128 -> 128", "STREAM*8x8", "FWD", 1024, 128, 128, smallm_rows=512),
    _case("stream 64 -> 64, ReLU", "STREAM*4x4", "FWD", 1024, 64, 64, act=1, smallm_rows=512),
    _case("stream, above the default smallm_rows", "STREAM*12x4", "FWD", 1025, 64, 192),
    _case("stream, data gradient 192 -> 64", "STREAM*4x12", "BWD_DATA", 1024, 64, 192, smallm_rows=512),
    _case("stream, 1023 rows", "TILED*4", "FWD", 1023, 64, 192, smallm_rows=512),
    _case("stream, 1023 rows, data gradient", "TILED*4", "BWD_DATA", 1023, 64, 192, smallm_rows=512),
    _case("stream, tanh", "TILED*4", "FWD", 1024, 64, 192, act=2, smallm_rows=512),
    _case("stream, N = 208", "TILED*4", "FWD", 1024, 64, 208, smallm_rows=512),
    _case("stream, ldy % 4 != 0", "TILED*4", "FWD", 1024, 64, 192, ldy=193, smallm_rows=512),
    _case("stream, 1024 rows at the default smallm_rows: wave tiles", "SMALLM*1", "FWD", 1024, 64, 192),
    # ---- K4: rows of 135 floats, from 4096 rows in whole groups of 16
    _case("k4", "K4", "FWD", 4096, 135, 64),
    _case("k4, row-mapped, ReLU", "K4*1", "FWD", 4096, 135, 64, row_map=(128, 32), act=1),
    _case("k4, 4095 rows", "TILED*1", "FWD", 4095, 135, 64),
    _case("k4, 4080 rows", "TILED*1", "FWD", 4080, 135, 64),
    _case("k4, 4100 rows", "TILED*1", "FWD", 4100, 135, 64),
    _case("k4, keep mask", "TILED*1", "FWD", 4096, 135, 64, keep=True),
    # ---- TILED: the LDS-tiled kernel, float4 or scalar operand loads
    _case("tiled, scalar, data gradient", "TILED*1", "BWD_DATA", 37, 50, 150),
    _case("tiled, row-mapped with a keep mask", "TILED*1", "FWD", 5 * 7, 135, 64, row_map=(7, 5), keep=True),
    _case("tiled, row-mapped, float4", "TILED*4", "FWD", 3 * 13, 48, 70, row_map=(13, 3)),
    _case("tiled, one row", "TILED*1", "FWD", 1, 3, 5),
    # ---- the pair: one launch on the float4 LDS-tiled kernel, N > 192, smallm_rows < M <= 16384
    _case("pair, one launch", "TILED*4|ONE_LAUNCH", "FWD_PAIR", 2560, 200, 600),
    _case("pair, one launch, first row count", "TILED*4|ONE_LAUNCH", "FWD_PAIR", 1025, 200, 600, act=1),
    _case("pair, one launch, last row count", "TILED*4|ONE_LAUNCH", "FWD_PAIR", 16384, 200, 600),
    _case("pair, 16385 rows", "TILED*4", "FWD_PAIR", 16385, 200, 600),
    _case("pair, smallm_rows rows", "SMALLM*2", "FWD_PAIR", 1024, 200, 600),
    _case("pair, the streaming kernel's shape", "STREAM*12x4", "FWD_PAIR", 2560, 64, 192),
    _case("pair, N = 192 off the streaming kernel: tiled, two launches", "TILED*4", "FWD_PAIR", 2560, 64, 192, act=2),
    _case("pair, K % 4 != 0", "TILED*1", "FWD_PAIR", 2560, 202, 600),
    # ---- the dual: one launch where both halves take 16 x 16 wave tiles
    _case("dual, one launch", "SMALLM*1|ONE_LAUNCH", "FWD_DUAL", 128, 200, 514, N_b=200),
    _case("dual, the second half over 2048 tiles", "SMALLM*1", "FWD_DUAL", 1024, 200, 200, N_b=600),
    _case("dual, the first half over 2048 tiles", "SMALLM*2", "FWD_DUAL", 1024, 200, 600, N_b=200),
    _case("dual, smallm_rows + 1 rows", "TILED*4", "FWD_DUAL", 1025, 200, 514, N_b=200),
)
