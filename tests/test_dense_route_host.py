"""CPU-only: the dense forward / data-gradient dispatch plan (csrc/linear.hip dense_plan) through g2v_linear_route.
DENSE_ROUTE_SHAPES (tests/_dense_route_shapes.py) names, for every route, variant and form, a call that selects it and the nearest
calls that miss it; the cascade of launchers the plan replaced is written out here as it stood and compared with the query over a
grid; and the bitwise contract of the bulk-z code assignment with g2v_linear_fwd is held to the query.  No kernel is launched."""
import itertools

import pytest

import _dense_route_shapes as DS
import _vq_route_shapes as VS
from gesture2vec_amd import _lib, ops


@pytest.mark.parametrize("case", DS.DENSE_ROUTE_SHAPES, ids=lambda c: c["name"])
def test_shape_selects_its_named_route(case):
    assert DS.route(**case) == case["route"]


def test_route_table_names_every_constant_of_the_header():
    shapes = DS.DENSE_ROUTE_SHAPES
    assert {part.split("*")[0] for c in shapes for part in c["route"].split("|")} == set(DS.ROUTES)
    assert DS.ROUTES == dict(SMALLM=1, STREAM=2, K4=3, TILED=4, ONE_LAUNCH=1 << 16)
    assert DS.FORMS == dict(FWD=0, BWD_DATA=1, FWD_PAIR=2, FWD_DUAL=3) and {c["form"] for c in shapes} == set(DS.FORMS)
    assert DS.ALIGN == dict(X=1, W=2, Y=4, BIAS=8, KEEP=16)
    got = {(c["form"], c["route"]) for c in shapes}
    assert got >= {("FWD", r) for r in ("SMALLM*1", "SMALLM*2", "SMALLM*4", "STREAM*12x4", "STREAM*4x12", "STREAM*8x8", "STREAM*4x4", "K4",
                                         "K4*1", "TILED*4", "TILED*1")}
    assert got >= {("BWD_DATA", r) for r in ("SMALLM*1", "SMALLM*2", "STREAM*4x12", "TILED*4", "TILED*1")}
    assert got >= {("FWD_PAIR", r) for r in ("TILED*4|ONE_LAUNCH", "TILED*4", "TILED*1", "STREAM*12x4", "SMALLM*2")}
    assert got >= {("FWD_DUAL", r) for r in ("SMALLM*1|ONE_LAUNCH", "SMALLM*1", "SMALLM*2", "TILED*4")}
    # each row count of the rule has its two neighbours in the table, smallm_rows included
    rows = {c["M"] for c in shapes}
    for n in DS.ROW_COUNTS:
        assert {n, n - 1} <= rows or {n, n + 1} <= rows, n
    assert any(c["M"] == c.get("smallm_rows", 1024) for c in shapes) and any(c["M"] == c.get("smallm_rows", 1024) + 1 for c in shapes)
    assert {1023, 1024, 4095, 4096, 16384, 16385} <= rows
    assert len({c["name"] for c in shapes}) == len(shapes)


def test_route_is_a_function_of_its_arguments_alone():
    """-1 for smallm_rows reads the bound context's value; an explicit value makes the answer independent of the context."""
    cur = _lib.Context.current()
    with cur.scoped(smallm_rows=4096):
        assert ops.linear_route("FWD", 2560, 200, 600) == "SMALLM*2"
        assert ops.linear_route("FWD", 2560, 200, 600, smallm_rows=1024) == "TILED*4"
        assert ops.linear_route("FWD_PAIR", 2560, 200, 600) == "SMALLM*2"
    with cur.scoped(smallm_rows=1024):
        assert ops.linear_route("FWD", 2560, 200, 600) == "TILED*4"
        assert ops.linear_route("FWD", 2560, 200, 600, smallm_rows=4096) == "SMALLM*2"
        assert ops.linear_route("FWD_PAIR", 2560, 200, 600) == "TILED*4|ONE_LAUNCH"
    for c in DS.DENSE_ROUTE_SHAPES[::5]:
        assert DS.route(**c) == DS.route(**c) == c["route"]


def test_route_query_refuses_what_the_calls_refuse():
    q = _lib.load().g2v_linear_route
    for form in DS.FORMS.values():
        assert q(form, 128, 200, 600, 200, 0, 1, 0, 0, 0, 0, 200, 600, 1024, 31) != 0
        for M, K, N, act in ((0, 200, 600, 0), (128, 0, 600, 0), (128, 200, -1, 0), (128, 200, 600, 3), (128, 200, 600, -1)):
            assert q(form, M, K, N, 200, act, 1, 0, 0, 0, 0, 200, 600, 1024, 31) == 0, (form, M, K, N, act)
    assert q(DS.FORMS["FWD_DUAL"], 128, 200, 600, 0, 0, 1, 0, 0, 0, 0, 200, 600, 1024, 31) == 0      # (no second half)
    assert q(4, 128, 200, 600, 0, 0, 1, 0, 0, 0, 0, 200, 600, 1024, 31) == 0 and q(-1, 128, 200, 600, 0, 0, 1, 0, 0, 0, 0, 200, 600, 1024, 31) == 0


# ---- the cascade of launchers as it stood before dense_plan (linear.hip of the parent commit), written out ----------------------
def _cdiv(a, b):
    return -(-a // b)


SMALLM, STREAM, K4, TILED, ONE = 1, 2, 3, 4, 1 << 16


def _old_launch_smallm(trans_b, M, C, N, lda, ldb, a16, b16, keep, keep4, smallm):
    if M > smallm or (C & 3) or (lda & 3) or not a16:
        return 0
    if not trans_b and ((ldb & 3) or not b16):
        return 0
    if keep and not keep4:
        return 0
    tiles16 = _cdiv(M, 16) * _cdiv(N, 16)
    return SMALLM | (1 if tiles16 <= 2048 else (2 if tiles16 <= 8192 else 4)) << 8


def _old_launch_stream(M, C, N, act, lda, ldc, a16, c16, bias, bias16):
    if M < 1024 or (C & 3) or (N & 15) or N > 192 or act == 2:
        return 0
    if not (a16 and (lda & 3) == 0) or not (c16 and (ldc & 3) == 0) or (bias and not bias16):
        return 0
    ks, ntw = (C + 15) >> 4, N >> 4
    for inst in ((12, 4), (4, 12), (8, 8), (4, 4)):
        if (ntw, ks) == inst:
            return STREAM | (ntw << 4 | ks) << 8
    return 0


def _old_launch_k4(rows_inner, M, C, N, act, ldc, c16, bias, bias16):
    if N != 64 or C != 135 or M < 4096 or (M & 15) or act == 2:
        return 0
    if not (c16 and (ldc & 3) == 0) or (bias and not bias16):
        return 0
    return K4 | (1 if rows_inner > 0 else 0) << 8


def _old_linear_fwd(M, K, N, act, bias, keep, ri, so, si, ldx, ldy, x16, w16, y16, bias16, keep4, smallm):
    r = ri == 0 and _old_launch_smallm(False, M, K, N, ldx, K, x16, w16, keep, keep4, smallm)
    r = r or (ri == 0 and not keep and _old_launch_stream(M, K, N, act, ldx, ldy, x16, y16, bias, bias16))
    r = r or (not keep and _old_launch_k4(ri, M, K, N, act, ldy, y16, bias, bias16))
    if r:
        return r
    a_vec = not keep and (K & 3) == 0 and x16 and (((so & 3) == 0 and (si & 3) == 0) if ri > 0 else (ldx & 3) == 0)
    return TILED | (4 if a_vec and w16 else 1) << 8


def _old_linear_bwd_data(M, K, N, lddy, lddx, dy16, w16, dx16, smallm):
    r = _old_launch_smallm(True, M, N, K, lddy, K, dy16, w16, False, True, smallm)
    r = r or _old_launch_stream(M, N, K, 0, lddy, lddx, dy16, dx16, False, True)
    if r:
        return r
    vec = (N & 3) == 0 and (K & 3) == 0 and (lddy & 3) == 0 and dy16 and w16
    return TILED | (4 if vec else 1) << 8


def _old_linear_fwd_pair(M, K, N, act, bias, ldx, ldy, x16, w16, y16, bias16, smallm):
    tiled = M > smallm and N > 192 and not (N == 64 and K == 135)
    vec = (K & 3) == 0 and (ldx & 3) == 0 and x16 and w16
    if tiled and vec and M <= 16384:
        return TILED | 4 << 8 | ONE
    return _old_linear_fwd(M, K, N, act, bias, False, 0, 0, 0, ldx, ldy, x16, w16, y16, bias16, True, smallm)


def _old_linear_fwd_dual(M, K, N_a, N_b, bias, ldx, ldya, x16, w16, y16, bias16, smallm):
    tiles_a, tiles_b = _cdiv(M, 16) * _cdiv(N_a, 16), _cdiv(M, 16) * _cdiv(N_b, 16)
    if M <= smallm and (K & 3) == 0 and (ldx & 3) == 0 and x16 and w16 and tiles_a <= 2048 and tiles_b <= 2048:
        return SMALLM | 1 << 8 | ONE
    return _old_linear_fwd(M, K, N_a, 0, bias, False, 0, 0, 0, ldx, ldya, x16, w16, y16, bias16, True, smallm)


GRID_M = (1, 15, 16, 1023, 1024, 1025, 2560, 4080, 4095, 4096, 4100, 16384, 16385, 65536)
GRID_KN = ((200, 600), (600, 200), (64, 2100), (135, 64), (64, 192), (192, 64), (128, 128), (64, 64), (64, 208), (202, 600),
           (200, 514), (200, 200), (50, 150), (48, 144), (48, 70), (3, 5))


def test_the_plan_decides_what_the_cascade_of_launchers_decided():
    """g2v_linear_route against the parent commit's g2v_linear_fwd / _bwd_data / _fwd_pair / _fwd_dual, written out above as they
    stood (oddities included): every row count of the rule and its neighbours, every shape the table names, every activation, keep
    mask / row map / bias on and off, every alignment fact on and off, both row strides whole float4s or not, all four forms."""
    q = _lib.load().g2v_linear_route
    F = DS.FORMS
    assert set(GRID_KN) >= {(c["K"], c["N"]) for c in DS.DENSE_ROUTE_SHAPES}
    # (alignment facts, ldx and ldy dense or one float longer): every fact with dense strides, every stride pair with all facts
    settings = [(al, 0, 0) for al in range(32)] + [(31, dx, dy) for dx, dy in ((1, 0), (0, 1), (1, 1))]
    checked = 0
    for smallm, M, (K, N), (al, dx, dy) in itertools.product((1024, 512), GRID_M, GRID_KN, settings):
        x16, w16, y16, b16, k4 = (bool(al & DS.ALIGN[n]) for n in ("X", "W", "Y", "BIAS", "KEEP"))
        ldx, ldy = K + dx, N + dy
        for act, bias, keep, mapped in itertools.product((0, 1, 2), (0, 1), (0, 1), (0, 1)):
            ri, so, si = (7, K, 3 * K) if mapped else (0, 0, 0)
            want = _old_linear_fwd(M, K, N, act, bias, keep, ri, so, si, ldx, ldy, x16, w16, y16, b16, k4, smallm)
            assert q(F["FWD"], M, K, N, 0, act, bias, keep, ri, so, si, ldx, ldy, smallm, al) == want, (M, K, N, act, bias, keep, mapped, al, dx, dy, smallm)
            checked += 1
            if keep or mapped:
                continue
            want = _old_linear_fwd_pair(M, K, N, act, bias, ldx, ldy, x16, w16, y16, b16, smallm)
            assert q(F["FWD_PAIR"], M, K, N, 0, act, bias, 0, 0, 0, 0, ldx, ldy, smallm, al) == want, ("pair", M, K, N, act, bias, al, dx, dy, smallm)
            if act == 0:
                for N_b in (200, 600):
                    want = _old_linear_fwd_dual(M, K, N, N_b, bias, ldx, ldy, x16, w16, y16, b16, smallm)
                    assert q(F["FWD_DUAL"], M, K, N, N_b, 0, bias, 0, 0, 0, 0, ldx, ldy, smallm, al) == want, ("dual", M, K, N, N_b, bias, al, dx, dy, smallm)
                if bias == 0:      # (dy (M, N) with row stride N + dx, dx (M, K) with row stride K + dy)
                    want = _old_linear_bwd_data(M, K, N, N + dx, K + dy, x16, w16, y16, smallm)
                    assert q(F["BWD_DATA"], M, K, N, 0, 0, 0, 0, 0, 0, 0, N + dx, K + dy, smallm, al) == want, ("bwd", M, K, N, al, dx, dy, smallm)
                    # what the data gradient's entry point has no argument for is ignored
                    assert q(F["BWD_DATA"], M, K, N, 9, 2, 1, 1, 7, 1, 1, N + dx, K + dy, smallm, al) == want
    assert checked == 2 * len(GRID_M) * len(GRID_KN) * 35 * 24


def test_bulk_z_rows_run_the_float4_tiled_projection():
    """vq_bulk_z.hip promises the bits of g2v_linear_fwd's LDS-tiled float4 kernel for the pre_linear product (forward, M = N rows,
    400 -> 400, bias, no mask): wherever the code-assignment plan answers BULK_Z -- the table's shapes, and smallm_rows swept around
    their row counts -- the dense plan answers TILED*4 for that product, and one row count later it no longer does."""
    bulk = [c for c in VS.VQ_ROUTE_SHAPES if c["route"] == "BULK_Z"]
    assert len(bulk) >= 5
    for c in bulk:
        N = c["N"]
        assert c["E"] == 400
        for s in sorted({c.get("smallm_rows", 1024), 0, 1024, 2047, N - 2, N - 1, N, N + 1, 1 << 20}):
            vq = VS.route(**{**c, "smallm_rows": s})
            dense = ops.linear_route("FWD", N, 400, 400, bias=True, smallm_rows=s)
            assert (vq == "BULK_Z") == (s < N), (c["name"], s)
            assert dense == "TILED*4" if vq == "BULK_Z" else dense.startswith("SMALLM"), (c["name"], s, dense)
