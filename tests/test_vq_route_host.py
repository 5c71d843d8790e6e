"""CPU-only: the code-assignment dispatch plan (csrc/vq.hip vq_route_plan) through g2v_vq_assign_route, the older *_ok queries
against it, and the size queries pinned to what the library returned before the dispatch moved into the plan
(tests/golden/vq_route_sizes.npz).  VQ_ROUTE_SHAPES (tests/_vq_route_shapes.py) names, for every route and variant, a shape that
selects it and the nearest shapes that miss it.  No kernel is launched."""
import os

import numpy as np
import pytest

import _vq_route_shapes as VS
from gesture2vec_amd import _lib, ops


def test_size_queries_are_pinned(golden_dir):
    fx = np.load(os.path.join(golden_dir, "vq_route_sizes.npz"))
    assert tuple(map(tuple, fx["bulk_NEK"])) == VS.BULK_NEK and tuple(map(tuple, fx["bulk_z_NEK"])) == VS.BULK_Z_NEK, "the sweep moved"
    assert tuple(map(tuple, fx["bx_KE"])) == VS.BX_KE, "the sweep moved: record again"
    assert int(fx["bulk"][0]) == 2 * 131072 + 256 + 2 * 2048 + 4 * 131072 and int(fx["bx"][3]) == 131072 + 2 * 2048 + 256
    lib = _lib.load()
    for nek, want in zip(VS.BULK_NEK, fx["bulk"]):
        assert lib.g2v_vq_assign_bulk_workspace(*nek) == int(want), nek
    for nek, want in zip(VS.BULK_Z_NEK, fx["bulk_z"]):
        assert lib.g2v_vq_assign_bulk_z_workspace(*nek) == int(want), nek
    for ke, want in zip(VS.BX_KE, fx["bx"]):
        assert lib.g2v_vq_bx_image_bytes(*ke) == int(want), ke


@pytest.mark.parametrize("case", VS.VQ_ROUTE_SHAPES, ids=lambda c: c["name"])
def test_shape_selects_its_named_route(case):
    assert VS.route(**case) == case["route"]


def test_route_table_names_every_constant_of_the_header():
    names = {part.split("*")[0] for c in VS.VQ_ROUTE_SHAPES for part in c["route"].split(">") if part}
    assert names == set(VS.ROUTES)
    assert len(VS.ROUTES) == 10 and sorted(VS.ROUTES.values()) == list(range(1, 11))
    assert {f for c in VS.VQ_ROUTE_SHAPES for f in c.get("facts", ())} == set(VS.FACTS)
    assert sorted(VS.FACTS.values()) == [1, 2, 4]
    assert {(c["form"], c["wants"]) for c in VS.VQ_ROUTE_SHAPES} == {(f, w) for f in ("ROWS", "RAW") for w in ("FULL", "IDX", "IDX_BULK")}
    got = {c["route"] for c in VS.VQ_ROUTE_SHAPES}
    assert got >= {"BX", "FUSED", "FUSED*1", "BULK_Z", "BULK*7", "PACKED*1", "PACKED*2", "PACKED*4", "RT*4", "FAST*1", "SPLIT*2", "SPLIT*3",
                   "SPLIT*8", "GENERIC", "", "PROJECT>BULK*9", "PROJECT>PACKED*4", "PROJECT>RT*4", "PROJECT>FAST*1", "PROJECT>SPLIT*8",
                   "PROJECT>GENERIC"}
    # each row count of the header has its two neighbours in the table
    rows = {(c["form"], c["N"]) for c in VS.VQ_ROUTE_SHAPES}
    for name, n in VS.ROWS.items():
        if name.endswith("_ROWS"):
            assert any((f, n) in rows for f in ("ROWS", "RAW")) and any((f, n - 1) in rows for f in ("ROWS", "RAW")), name
    assert len({c["name"] for c in VS.VQ_ROUTE_SHAPES}) == len(VS.VQ_ROUTE_SHAPES)


def test_callers_that_do_not_accept_bulk_never_get_it():
    """k-means and the autograd function ask as ROWS callers without a workspace; only VQ_Payam_EMA.assign accepts the bulk routes,
    and no indices-only call runs BX."""
    for c in VS.VQ_ROUTE_SHAPES:
        if c["wants"] != "IDX_BULK":
            assert "BULK" not in c["route"], c["name"]
        if c["wants"] != "FULL":
            assert "BX" not in c["route"] and "FUSED" not in c["route"], c["name"]


def test_route_is_a_function_of_its_arguments_alone():
    """-1 for smallm_rows reads the bound context's value; an explicit value makes the answer independent of the context."""
    cur = _lib.Context.current()
    with cur.scoped(smallm_rows=40000):
        assert ops.vq_route("RAW", "IDX_BULK", 40000, 400, 512) == "PROJECT>PACKED*4"
        assert ops.vq_route("RAW", "IDX_BULK", 40000, 400, 512, smallm_rows=1024) == "BULK_Z"
        assert not ops.vq_assign_bulk_z_ok(40000, 400, 512) and ops.vq_assign_bulk_z_ok(40001, 400, 512)
    with cur.scoped(smallm_rows=1024):
        assert ops.vq_route("RAW", "IDX_BULK", 40000, 400, 512) == "BULK_Z"
        assert ops.vq_route("RAW", "IDX_BULK", 40000, 400, 512, smallm_rows=40000) == "PROJECT>PACKED*4"
    for c in VS.VQ_ROUTE_SHAPES[::7]:
        assert VS.route(**c) == VS.route(**c) == c["route"]
    lib = _lib.load()
    assert lib.g2v_vq_assign_route(2, 0, 40, 128, 512, -1, 0) == 0 and lib.g2v_vq_assign_route(0, 3, 40, 128, 512, -1, 0) == 0


def test_older_queries_are_fields_of_the_plan():
    """g2v_vq_assign_packed_ok, g2v_vq_fused_assign_bx_ok and g2v_vq_assign_bulk_z_ok keep the answers they gave as hand-written
    conditions (written out here as they stood), and equal the route query of the call they describe."""
    lib = _lib.load()
    smallm = 1024
    with _lib.Context.current().scoped(smallm_rows=smallm):
        for N in (0, 1, 40, 2047, 2048, 4096, 40000):
            for E in (0, 16, 48, 100, 128, 384, 400, 608, 624, 640):
                for K in (0, 16, 24, 32, 48, 128, 256, 384, 512, 528, 640, 1024):
                    packed = N > 0 and E >= 16 and E % 16 == 0 and K >= 16 and K % 16 == 0 and (64 * (E + 4) + 64 + 1024 + 64 + 8) * 4 <= 160 * 1024
                    assert lib.g2v_vq_assign_packed_ok(N, E, K) == int(packed), (N, E, K)
                    assert lib.g2v_vq_fused_assign_bx_ok(N, E, K) == int(N > 0 and E == 128 and K % 128 == 0 and 128 <= K <= 512), (N, E, K)
                    bulk_z = N >= 2048 and N > smallm and E == 400 and 32 <= K <= 512 and K % 16 == 0 and packed
                    assert lib.g2v_vq_assign_bulk_z_ok(N, E, K) == int(bulk_z), (N, E, K)
                    assert (ops.vq_route("ROWS", "FULL", N, E, K, facts=("ENTRY",)).split("*")[0] == "PACKED") == packed
                    assert (ops.vq_route("RAW", "FULL", N, E, K) == "BX") == bool(lib.g2v_vq_fused_assign_bx_ok(N, E, K))
                    assert (ops.vq_route("RAW", "IDX_BULK", N, E, K, facts=("ENTRY",)) == "BULK_Z") == bulk_z
