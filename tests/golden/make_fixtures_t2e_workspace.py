#!/usr/bin/env python
"""Writes tests/golden/t2e_route_sizes.npz: g2v_attn_code_rollout_fwd_workspace(H, K, attention), _bwd_workspace(S1, B, H, K, Tw,
attention) and g2v_code_cluster_bptt_workspace(B, H) over the sweeps of tests/_t2e_route_shapes.py, as the library of the commit
BEFORE the code decoder's dispatch moved into one plan returned them.

    python tests/golden/make_fixtures_t2e_workspace.py path/to/libg2v_hip.so     (of the commit to record)

The forward query sizes the cluster kernel's records for the device's CU count and falls back to 256 CUs -- an MI355X's -- when there
is no device, so the recording holds with and without one.  tests/test_t2e_route_host.py demands equality on every entry, so that a
caller's buffer never changes size under a refactor of the dispatch."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]
import _t2e_route_shapes as TS  # noqa: E402


def main():
    lib = ctypes.CDLL(sys.argv[1])
    out = {}
    for key, name, sweep in (("fwd", "g2v_attn_code_rollout_fwd_workspace", TS.FWD_HKA), ("bwd", "g2v_attn_code_rollout_bwd_workspace", TS.BWD_ARGS),
                             ("bptt", "g2v_code_cluster_bptt_workspace", TS.BPTT_BH)):
        query = getattr(lib, name)
        query.restype, query.argtypes = ctypes.c_size_t, [ctypes.c_int] * len(sweep[0])
        out[key + "_args"] = np.array(sweep, dtype=np.int64)
        out[key] = np.array([query(*a) for a in sweep], dtype=np.int64)
        print(f"{name}: {len(sweep)} entries, {sweep[len(sweep) // 2]} -> {out[key][len(sweep) // 2]}")
    np.savez(os.path.join(HERE, "t2e_route_sizes.npz"), **out)


if __name__ == "__main__":
    main()
