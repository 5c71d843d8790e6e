#!/usr/bin/env python
"""Writes tests/golden/wgrad_workspace.npz: g2v_linear_bwd_weight_workspace(M, K, N) over the sweep of tests/_wgrad_shapes.py
(WORKSPACE_M x WORKSPACE_KN), as the library of the commit BEFORE the weight-gradient dispatch moved into one plan returned it.

    python tests/golden/make_fixtures_wgrad_workspace.py [path/to/libg2v_hip.so of the commit to record]

The query is host arithmetic: no device is needed.  tests/test_wgrad_plan_host.py demands equality on every entry, so that a
caller's buffer never changes size under a refactor of the dispatch."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]
import _wgrad_shapes as WS  # noqa: E402


def main():
    lib = ctypes.CDLL(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "gesture2vec_amd", "libg2v_hip.so"))
    query = lib.g2v_linear_bwd_weight_workspace
    query.restype, query.argtypes = ctypes.c_size_t, [ctypes.c_int] * 3
    nbytes = np.array([[query(M, K, N) for K, N in WS.WORKSPACE_KN] for M in WS.WORKSPACE_M], dtype=np.int64)
    print(f"{nbytes.size} values, (1, 64, 192) -> {nbytes[0, 0]}, largest {nbytes.max()}")
    np.savez(os.path.join(HERE, "wgrad_workspace.npz"), M=np.array(WS.WORKSPACE_M, dtype=np.int64),
             KN=np.array(WS.WORKSPACE_KN, dtype=np.int64), nbytes=nbytes)


if __name__ == "__main__":
    main()
