#!/usr/bin/env python
"""Writes tests/golden/dec_rollout_workspace.npz: g2v_dec_rollout_fwd_workspace(D, H) and g2v_dec_rollout_bwd_workspace(D, H) over
the sweep of tests/_dec_route_shapes.py (WORKSPACE_D x WORKSPACE_H), as the library of the commit BEFORE the decoder rollout's
dispatch moved into one plan returned them.

    python tests/golden/make_fixtures_dec_workspace.py [path/to/libg2v_hip.so of the commit to record]

Both queries size the cluster kernel's records for the device's CU count and fall back to 256 CUs -- an MI355X's -- when there is no
device, so the recording holds with and without one.  tests/test_dec_route_host.py demands equality on every entry, so that a
caller's buffer never changes size under a refactor of the dispatch."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]
import _dec_route_shapes as DS  # noqa: E402


def main():
    lib = ctypes.CDLL(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "gesture2vec_amd", "libg2v_hip.so"))
    out = {}
    for key in ("fwd", "bwd"):
        query = getattr(lib, f"g2v_dec_rollout_{key}_workspace")
        query.restype, query.argtypes = ctypes.c_size_t, [ctypes.c_int] * 2
        out[key] = np.array([[query(D, H) for H in DS.WORKSPACE_H] for D in DS.WORKSPACE_D], dtype=np.int64)
    i, j = DS.WORKSPACE_D.index(40), DS.WORKSPACE_H.index(200)
    print(f"{out['fwd'].size} shapes, (40, 200) -> {out['fwd'][i, j]} / {out['bwd'][i, j]}")
    np.savez(os.path.join(HERE, "dec_rollout_workspace.npz"), D=np.array(DS.WORKSPACE_D, dtype=np.int64),
             H=np.array(DS.WORKSPACE_H, dtype=np.int64), **out)


if __name__ == "__main__":
    main()
