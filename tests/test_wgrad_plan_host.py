"""CPU-only: the weight-gradient plan (csrc/linear.hip wgrad_plan) through its two host queries.  The workspace bound is pinned
to what the library returned before the dispatch moved into the plan (tests/golden/wgrad_workspace.npz), and WGRAD_ROUTE_SHAPES
(tests/_wgrad_shapes.py) names, for every route, a shape that selects it.  No kernel is launched."""
import os

import numpy as np
import pytest

import _wgrad_shapes as WS
from gesture2vec_amd import _lib


def test_workspace_query_is_pinned(golden_dir):
    fx = np.load(os.path.join(golden_dir, "wgrad_workspace.npz"))
    assert tuple(fx["M"]) == WS.WORKSPACE_M and tuple(map(tuple, fx["KN"])) == WS.WORKSPACE_KN, "the sweep moved: record again"
    assert fx["nbytes"].shape == (23, 16) and int(fx["nbytes"][0, 0]) == 49920 and int(fx["nbytes"].max()) == 25662000
    query = _lib.load().g2v_linear_bwd_weight_workspace
    for i, M in enumerate(WS.WORKSPACE_M):
        for j, (K, N) in enumerate(WS.WORKSPACE_KN):
            assert query(M, K, N) == int(fx["nbytes"][i, j]), (M, K, N)
    for M, K, N in ((0, 64, 192), (4096, 0, 192), (4096, 64, 0), (-1, 64, 192), (4096, -5, -5)):
        assert query(M, K, N) == 0, (M, K, N)


@pytest.mark.parametrize("case", WS.WGRAD_ROUTE_SHAPES, ids=lambda c: c["name"])
def test_shape_selects_its_named_route(case):
    assert WS.route_name(**case) == case["route"]


def test_route_table_names_every_route_of_the_header():
    named = {part for case in WS.WGRAD_ROUTE_SHAPES for part in case["route"].split("|")}
    assert named == set(WS.ROUTES) and len(WS.ROUTES) == 10
    assert len(set(WS.ROUTES.values())) == len(WS.ROUTES) and WS.ROUTES["RAGGED_TAIL"] > max(v for k, v in WS.ROUTES.items() if k != "RAGGED_TAIL")
    assert len({c["name"] for c in WS.WGRAD_ROUTE_SHAPES}) == len(WS.WGRAD_ROUTE_SHAPES)


def test_two_addend_query_agrees_with_the_route():
    ok = _lib.load().g2v_linear_bwd_weight_sum2_ok
    duals = [c for c in WS.WGRAD_ROUTE_SHAPES if c.get("dual")]
    assert len(duals) == 2
    for c in duals:
        assert ok(c["M"], c["K"], c["N"]) == 1 and WS.route_name(**c) == "WAVE_DUAL"
    assert ok(4095, 135, 64) == 0 and WS.route_name(4095, 135, 64, dual=True) == ""       # (refused, not another route)
    assert WS.route_name(4095, 135, 64) == "SMALL_WAVES16"        # (36 tiles, many rows)


def test_route_query_refuses_what_the_calls_refuse():
    route = _lib.load().g2v_linear_bwd_weight_route
    for M, K, N, nprob in ((0, 64, 192, 1), (4096, 0, 192, 1), (4096, 64, -1, 1), (4096, 64, 192, 0), (4096, 64, 192, 5)):
        assert route(M, K, N, nprob, 0, 0, 0, 0, N, K, 16) == 0
