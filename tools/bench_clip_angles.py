#!/usr/bin/env python
"""Times the two kernels behind generate.clip_angles (csrc/clip_angles.hip) with device events around warmed calls (medians), at
J = 15 joints:
  one clip of 60 chunks (B = 1, F = 2040), 4096 clips of 6 chunks (F = 204), the codebook (B = 512, F = 34)
and sets each against the bytes it has to move (conversion: 36 B in + 12 B out per matrix; spline: y read twice, the float64
intermediate written and read, out written = 28 B per element) over the achievable HBM rate, and against the host tail the
reference runs on the same data: read-back, scipy's Rotation.from_matrix(...).as_euler("ZXY") per frame, one smoothing spline per
channel (scipy's make_smoothing_spline at lam = 1; csaps is not a dependency of this repository).  The host tail is timed on at
most --host-clips clips and scaled by the clip count; the record says from how many.  `spline_one_column_ms` is the same F with one
column: the factorisation plus one serial chain, which is what bounds the single long clip.

    python tools/bench_clip_angles.py --out profiles/clip_angles.jsonl"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gesture2vec_amd import generate, ops  # noqa: E402

DEV = "cuda:0"
HBM_GBS = 6300.0            # achievable, not peak
J = 15
SHAPES = {"clip60": (1, 2040), "clips4096x6": (4096, 204), "codebook512": (512, 34)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def median_ms(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    return statistics.median(timed(fn) for _ in range(reps))


def make_frames(B, F, seed):
    """decoder-like matrices: Rz Rx Ry of random angles (|X| <= 70 degrees) plus Gaussian noise of 0.05 on the entries"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    n = B * F * J
    z, y = ((torch.rand(n, generator=g, device=DEV) * 2 - 1) * np.pi for _ in range(2))
    x = (torch.rand(n, generator=g, device=DEV) * 2 - 1) * np.radians(70.0)
    cz, sz, cx, sx, cy, sy = z.cos(), z.sin(), x.cos(), x.sin(), y.cos(), y.sin()
    m = torch.stack([cz * cy - sz * sx * sy, -sz * cx, cz * sy + sz * sx * cy, sz * cy + cz * sx * sy, cz * cx, sz * sy - cz * sx * cy,
                     -cx * sy, sx, cx * cy], dim=1)
    m += 0.05 * torch.randn(n, 9, generator=g, device=DEV)
    return m.view(B, F, 9 * J).contiguous()


def host_tail(frames_dev, clips):
    from scipy.interpolate import make_smoothing_spline
    from scipy.spatial.transform import Rotation
    t0 = time.perf_counter()
    frames = frames_dev[:clips].cpu().numpy()
    out = np.empty(frames.shape[:2] + (3 * J,))
    for b in range(frames.shape[0]):
        for f in range(frames.shape[1]):
            out[b, f] = Rotation.from_matrix(frames[b, f].reshape(J, 3, 3)).as_euler("ZXY", degrees=True).reshape(-1)
        x = np.arange(frames.shape[1], dtype=np.float64)
        for c in range(3 * J):
            out[b, :, c] = make_smoothing_spline(x, out[b, :, c], lam=1.0)(x)
    return 1e3 * (time.perf_counter() - t0), out


def bench_shape(name, B, F, reps, host_clips):
    frames = make_frames(B, F, B + F)
    flat = frames.view(B * F, 9 * J)
    rec = {"shape": name, "B": B, "F": F, "J": J, "reps": reps}
    angles = None
    for method in generate.NEAREST:
        angles, bad = ops.rotmat_to_euler(flat, J, ops.ROT_METHODS[method])
        assert int(bad.item()) == 0
        rec[f"euler_{method}_ms"] = median_ms(lambda: ops.rotmat_to_euler(flat, J, ops.ROT_METHODS[method], out=angles, bad=bad), reps)
    angles, _ = ops.rotmat_to_euler(flat, J, ops.ROT_METHODS["markley"])
    y = angles.view(B, F, 3 * J)
    out = torch.empty_like(y)
    rec["spline_ms"] = median_ms(lambda: ops.smoothing_spline(y, 0.5, out=out), reps)
    one = y[:1, :, :1].contiguous()
    rec["spline_one_column_ms"] = median_ms(lambda: ops.smoothing_spline(one, 0.5), reps)
    rec["clip_angles_ms"] = median_ms(lambda: generate.clip_angles(frames), reps)        # both, with the counter's read-back
    euler_bytes, spline_bytes = 48 * B * F * J, 28 * B * F * 3 * J
    rec.update(euler_bytes=euler_bytes, spline_bytes=spline_bytes,
               euler_floor_ms=euler_bytes / HBM_GBS / 1e6, spline_floor_ms=spline_bytes / HBM_GBS / 1e6)
    rec["euler_markley_gbs"] = euler_bytes / rec["euler_markley_ms"] / 1e6
    rec["spline_gbs"] = spline_bytes / rec["spline_ms"] / 1e6
    try:
        clips = min(B, host_clips)
        ms, host = host_tail(frames, clips)
    except ImportError:
        rec["host_tail_ms"] = None
    else:
        import scipy
        rec.update(host_tail_ms=ms * B / clips, host_clips_timed=clips, host_scipy=scipy.__version__)
        if tuple(int(v) for v in scipy.__version__.split(".")[:2]) >= (1, 11):           # (it orthogonalises first)
            dev = generate.clip_angles(frames[:clips], nearest="procrustes").cpu().numpy()
            rec["host_max_abs_diff_deg"] = float(np.abs(dev - host).max())
        rec["host_over_device"] = rec["host_tail_ms"] / rec["clip_angles_ms"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-clips", dest="host_clips", type=int, default=4)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: there is nothing to time on a CPU"
    recs = []
    for name in a.shapes.split(","):
        B, F = SHAPES[name]
        recs.append(bench_shape(name, B, F, a.reps, a.host_clips))
        print(json.dumps(recs[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
