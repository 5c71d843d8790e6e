"""CPU-only: the decoder rollout's dispatch plan (csrc/dec_rollout.hip dec_route_plan) through g2v_dec_rollout_route, and the two
workspace queries pinned to what the library returned before the dispatch moved into the plan
(tests/golden/dec_rollout_workspace.npz).  DEC_ROUTE_SHAPES (tests/_dec_route_shapes.py) names, for every route and direction, a
shape that selects it and the nearest shapes that miss it.  No kernel is launched."""
import os

import numpy as np
import pytest

import _dec_route_shapes as DS
from gesture2vec_amd import _lib


def test_workspace_queries_are_pinned(golden_dir):
    fx = np.load(os.path.join(golden_dir, "dec_rollout_workspace.npz"))
    assert tuple(fx["D"]) == DS.WORKSPACE_D and tuple(fx["H"]) == DS.WORKSPACE_H, "the sweep moved: record again"
    i40, i135, j64, j200 = DS.WORKSPACE_D.index(40), DS.WORKSPACE_D.index(135), DS.WORKSPACE_H.index(64), DS.WORKSPACE_H.index(200)
    assert fx["fwd"].shape == fx["bwd"].shape == (8, 8)
    assert (int(fx["fwd"][i40, j200]), int(fx["bwd"][i40, j200])) == (5498912, 28888096)
    assert (int(fx["fwd"][i135, j64]), int(fx["bwd"][i135, j64])) == (1347584, 14127104)
    lib = _lib.load()
    for i, D in enumerate(DS.WORKSPACE_D):
        for j, H in enumerate(DS.WORKSPACE_H):
            assert lib.g2v_dec_rollout_fwd_workspace(D, H) == int(fx["fwd"][i, j]), (D, H)
            assert lib.g2v_dec_rollout_bwd_workspace(D, H) == int(fx["bwd"][i, j]), (D, H)


@pytest.mark.parametrize("case", DS.DEC_ROUTE_SHAPES, ids=lambda c: c["name"])
def test_shape_selects_its_named_route(case):
    assert DS.route_name(**case) == case["route"]


def test_route_table_names_every_route_of_the_header_in_both_directions():
    for backward in (False, True):
        named = {c["route"].split("*")[0] for c in DS.DEC_ROUTE_SHAPES if c["route"] and bool(c.get("backward")) == backward}
        assert named == set(DS.ROUTES)
    assert len(DS.ROUTES) == 5 and sorted(DS.ROUTES.values()) == [1, 2, 3, 4, 5]
    assert DS.FLAGS == {"UNALIGNED": 1, "WGRAD": 2, "LOSS": 4}
    assert {c["route"] for c in DS.DEC_ROUTE_SHAPES} >= {"PERSIST*1", "PERSIST*2", "PERSIST*3", ""}
    assert len({c["name"] for c in DS.DEC_ROUTE_SHAPES}) == len(DS.DEC_ROUTE_SHAPES)


def test_route_is_a_function_of_its_arguments_alone():
    """persistent = -1 reads the bound context's level; any other value and every cus > 0 make the answer independent of the
    context and of the device -- which is what lets this file run without one."""
    with _lib.Context.current().scoped(persistent=0):
        assert DS.route_name(2, 16, 135, 64, persistent=-1) == "STEP_FAST" and DS.route_name(2, 16, 135, 64, persistent=1) == "PERSIST*1"
    with _lib.Context.current().scoped(persistent=3):
        assert DS.route_name(2, 48, 135, 64, persistent=-1) == "PERSIST*3" and DS.route_name(2, 48, 135, 64, persistent=1) == "PERSIST*1"
        assert DS.route_name(2, 48, 135, 64, persistent=7) == "PERSIST*3"        # (levels above 3 are 3, as the option clamps them)
