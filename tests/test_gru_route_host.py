"""CPU-only: the GRU sequence dispatch plan (csrc/gru.hip gru_route_plan) through g2v_gru_seq_route, and the workspace queries
pinned to what the library returned before the dispatch moved into the plan (tests/golden/gru_seq_workspace.npz).
GRU_ROUTE_SHAPES (tests/_gru_route_shapes.py) names, for every route, variant and direction of travel, a shape that selects it and
the nearest shapes that miss it.  No kernel is launched."""
import os

import numpy as np
import pytest

import _gru_route_shapes as GS
from gesture2vec_amd import _lib


def _device_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 0


def test_workspace_queries_are_pinned(golden_dir):
    """Both size queries depend on the CU count through the cluster kernels' records: the fixture holds one column recorded
    without a device (count 0) and one recorded on an MI355X (256)."""
    fx = np.load(os.path.join(golden_dir, "gru_seq_workspace.npz"))
    assert tuple(fx["H"]) == GS.WORKSPACE_H and tuple(map(tuple, fx["wslab_BH"])) == GS.WSLAB_BH, "the sweep moved: record again"
    assert fx["fwd"].shape == fx["bwd"].shape == (2, 2, len(GS.WORKSPACE_H)) and tuple(fx["cus"]) == (0, 256)
    j64, j200 = GS.WORKSPACE_H.index(64), GS.WORKSPACE_H.index(200)
    assert (int(fx["fwd"][0, 1, j64]), int(fx["bwd"][0, 1, j64])) == (1048576, 1146880)
    assert (int(fx["fwd"][0, 1, j200]), int(fx["bwd"][0, 1, j200])) == (3276800, 4236800)
    lib = _lib.load()
    for (B, H), want in zip(GS.WSLAB_BH, fx["wslab"]):
        assert lib.g2v_gru_seq_bwd_wslab_bytes(B, H) == int(want), (B, H)
    cus = _device_cus()
    if cus not in tuple(fx["cus"]):
        pytest.skip(f"the fixture has no column for a device with {cus} CUs")
    col = list(fx["cus"]).index(cus)
    for i, ndir in enumerate((1, 2)):
        for j, H in enumerate(GS.WORKSPACE_H):
            assert lib.g2v_gru_seq_fwd_workspace(ndir, H) == int(fx["fwd"][col, i, j]), (ndir, H)
            assert lib.g2v_gru_seq_bwd_workspace(ndir, H) == int(fx["bwd"][col, i, j]), (ndir, H)


@pytest.mark.parametrize("case", GS.GRU_ROUTE_SHAPES, ids=lambda c: c["name"])
def test_shape_selects_its_named_route(case):
    assert GS.route_name(**case) == case["route"]


def test_route_table_names_every_constant_of_the_header_in_both_directions():
    for backward in (False, True):
        rows = [c for c in GS.GRU_ROUTE_SHAPES if bool(c.get("backward")) == backward]
        assert {c["route"].split("*")[0] for c in rows if c["route"]} == set(GS.ROUTES)
        facts = {f for c in rows for f in c.get("facts", ())}
        other = {"GATHERED"} if backward else {"WGRAD_HH", "WGRAD_IH", "WGRAD_PARTIAL", "HN", "HN_UNUSABLE", "NO_DGI"}      # (the other entry point's fields)
        assert facts == set(GS.FACTS) - other
    assert len(GS.ROUTES) == 5 and sorted(GS.ROUTES.values()) == [1, 2, 3, 4, 5]
    assert sorted(GS.FACTS.values()) == [1 << k for k in range(20)]
    routes = {(bool(c.get("backward")), c["route"]) for c in GS.GRU_ROUTE_SHAPES}
    assert routes >= {(False, "FAST"), (False, "FAST*1"), (False, "STREAM"), (False, "STREAM*1"), (False, "STREAM*2"), (False, ""),
                      (True, "FAST"), (True, "FAST*1"), (True, "FAST*2"), (True, "FAST*3"), (True, "STREAM"), (True, "STREAM*1"), (True, "")}
    assert len({c["name"] for c in GS.GRU_ROUTE_SHAPES}) == len(GS.GRU_ROUTE_SHAPES)


def test_route_is_a_function_of_its_arguments_alone():
    """-1 for any of the three options reads the bound context's value; explicit values and every cus > 0 make the answer
    independent of the context and of the device -- which is what lets this file run without one."""
    cur = _lib.Context.current()
    with cur.scoped(gru_cluster=0):
        assert GS.route_name(4, 144, 200, cluster=-1) == "STEP" and GS.route_name(4, 144, 200, cluster=1) == "CLUSTER"
    with cur.scoped(gru_cluster=1):
        assert GS.route_name(4, 144, 200, cluster=-1) == "CLUSTER" and GS.route_name(4, 144, 200, cluster=0) == "STEP"
    with cur.scoped(gru_resident_rows=0):
        assert GS.route_name(4, 1025, 200, resident_rows=-1) == "STREAM*1" and GS.route_name(4, 1025, 200, resident_rows=1025) == "RESIDENT"
    with cur.scoped(gru_resident_rows=2000):
        assert GS.route_name(4, 1999, 200, resident_rows=-1) == "STREAM*1" and GS.route_name(4, 2000, 200, resident_rows=-1) == "RESIDENT"
        assert GS.route_name(4, 1999, 200, resident_rows=1025) == "RESIDENT"
    with cur.scoped(gru_resident_bwd=0):
        assert GS.route_name(4, 1025, 200, backward=True, resident_bwd=-1) == "STREAM*1"
        assert GS.route_name(4, 1025, 200, backward=True, resident_bwd=1) == "RESIDENT"
    with cur.scoped(gru_resident_bwd=1):
        assert GS.route_name(4, 1025, 200, backward=True, resident_bwd=-1) == "RESIDENT"
        assert GS.route_name(4, 1025, 200, backward=True, resident_bwd=0) == "STREAM*1"
