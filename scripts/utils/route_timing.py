"""Timing of alternative routes against each other in one process (scripts/time_vq_frame.py, scripts/time_vae_frame.py)."""
import statistics

import torch


def timed(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters      # microseconds per call


def compare(fns, iters, rounds, warmup):
    """{route: callable} -> {route: median, min and max of `rounds` timed loops}; the routes alternate round by round"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(timed(fn, iters))
    return {k: dict(median_us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2)) for k, v in times.items()}
