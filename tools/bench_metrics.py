#!/usr/bin/env python
"""Times the moments kernel (g2v_moments_accumulate) against the two routes available without it, alternating in one process:
  matmul : xc = x - shift (a centring pass), torch.matmul(xc^T, xc) in fp32
  wgrad  : xc = x - shift, g2v_linear_bwd_weight_batch with dy = x = xc (where that entry point accepts the shape)
at E = 400 and E = 128, N in {4096, 65536, 2^20}: device-synchronised medians (events around each call).  One JSON line per shape
with the times and the kernel's two roofline fractions: executed upper-triangle FLOP (2 N * 256 * tile pairs, ET (ET + 1) / 2 pairs
of 16-column tiles) over 157.3 TF/s, and the bytes of x over 8 TB/s.  --e2e also times gesture_metrics on 2^20 + 2^20 chunks.
--bleu times BLEU over code sequences (K = 512) at (B, L) = (65536, 8) and (256, 1024): the clipped-count kernel alone
(g2v_ngram_clipped_counts), `code_bleu` end to end (scores on the device, one number read back), and the host route a user had without
them: read the ids back, `Counter`s per pair (the restatement in tests/_bleu_ref.py), timed once.

    python tools/bench_metrics.py --out profiles/metrics_moments.jsonl [--e2e] [--only-new] [--bleu] [--shapes ""]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gesture2vec_amd import ops  # noqa: E402

PEAK_F32_MFMA, PEAK_HBM = 157.3e12, 8.0e12
DEV = "cuda:0"


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def bench_shape(N, E, reps, only_new):
    g = torch.Generator(device=DEV).manual_seed(N + E)
    x = torch.cumsum(torch.randn(N, E, generator=g, device=DEV), dim=1) * 0.1 + 0.3
    shift = x[:256].mean(0).contiguous()
    s1 = torch.zeros(E, dtype=torch.float64, device=DEV)
    s2 = torch.zeros(E, E, dtype=torch.float64, device=DEV)
    dw = torch.empty(E, E, device=DEV)
    routes = {"new": lambda: ops.moments_accumulate(x, shift, s1, s2)}
    if not only_new:
        routes["matmul"] = lambda: _matmul(x, shift)
        try:
            _wgrad(x, shift, dw, N, E)
            routes["wgrad"] = lambda: _wgrad(x, shift, dw, N, E)
        except Exception as e:                                             # the entry point refuses the shape
            print(f"wgrad route refused at N={N} E={E}: {e}", file=sys.stderr)
    for fn in routes.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in routes}
    for _ in range(reps):
        for k, fn in routes.items():                                      # alternating
            times[k].append(timed(fn))
    ET = (E + 15) // 16
    flop = 2.0 * N * 256 * (ET * (ET + 1) // 2)
    nbytes = 4.0 * N * E
    rec = {"N": N, "E": E, "reps": reps, "flop_upper_triangle": flop, "bytes_x": nbytes}
    for k, v in times.items():
        rec[f"{k}_ms_median"] = statistics.median(v)
        rec[f"{k}_ms_min"] = min(v)
    t = rec["new_ms_median"] * 1e-3
    rec["new_frac_mfma_f32_peak"] = flop / PEAK_F32_MFMA / t
    rec["new_frac_hbm_peak"] = nbytes / PEAK_HBM / t
    if not only_new:
        rec["new_over_best_other"] = rec["new_ms_median"] / min(rec[f"{k}_ms_median"] for k in times if k != "new")
    return rec


def _matmul(x, shift):
    xc = x - shift
    return torch.matmul(xc.t(), xc)


def _wgrad(x, shift, dw, N, E):
    xc = x - shift
    ops.linear_bwd_weight_batch([(xc, xc, dw, None)], E, E, M=N)
    return dw


def bench_e2e(n_chunks):
    import argparse as ap
    from gesture2vec_amd.metrics import gesture_metrics, LatentMoments
    from gesture2vec_amd.model.Autoencoder_VQVAE_model import Autoencoder_VQVAE
    from gesture2vec_amd.pipeline import chunk_latents
    args = ap.Namespace(rep_learning_dim=40, hidden_size=200, n_layers=2, dropout_prob=0.0, autoencoder_vae="False",
                        autoencoder_vq="True", autoencoder_vq_components=512, autoencoder_vq_commitment_cost=0.25, n_pre_poses=1,
                        autoencoder_conditioned="True", autoencoder_att="False", autoencoder_fixed_weight="False", n_poses=20)
    torch.manual_seed(3)
    net = Autoencoder_VQVAE(args, 40, 20).to(DEV)
    net.train(False)
    g = torch.Generator(device=DEV).manual_seed(1)
    real = torch.randn(n_chunks, 20, 40, generator=g, device=DEV)
    gen = torch.randn(n_chunks, 20, 40, generator=g, device=DEV) * 1.1
    gesture_metrics(net, real[:65536], gen[:65536])                       # warm-up of every kernel at the batch shape
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m = gesture_metrics(net, real, gen)
    torch.cuda.synchronize()
    total = time.perf_counter() - t0
    lat = chunk_latents(net, real[:65536])
    idx = net.vq_layer.assign(lat)
    mom = LatentMoments(lat.shape[1], DEV).update(lat)
    counts = ops.code_histogram(idx, 512)
    nb = 2 * (n_chunks // 65536)
    t_mom = statistics.median(timed(lambda: mom.update(lat)) for _ in range(20)) * nb
    t_hist = statistics.median(timed(lambda: ops.code_histogram(idx, 512, counts)) for _ in range(20)) * nb
    return {"e2e_chunks_per_set": n_chunks, "gesture_metrics_s": total, "moments_kernels_ms": t_mom, "histogram_kernels_ms": t_hist,
            "share_new_kernels": (t_mom + t_hist) * 1e-3 / total, "frechet": m["frechet"]}


def bench_bleu(B, L, K=512, reps=50):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import _bleu_ref as R
    from gesture2vec_amd.metrics import code_bleu
    g = torch.Generator(device=DEV).manual_seed(B + L)
    ref = torch.randint(0, K, (B, L), generator=g, device=DEV)
    cand = torch.where(torch.rand(B, L, generator=g, device=DEV) < 0.1, torch.randint(0, K, (B, L), generator=g, device=DEV), ref)
    start = torch.arange(B, dtype=torch.int64, device=DEV) * L
    lens = torch.full((B,), L, dtype=torch.int64, device=DEV)
    kernel = lambda: ops.ngram_clipped_counts(cand.view(-1), start, lens, ref.view(-1), start, lens, K, 4, L)
    for _ in range(3):
        kernel()
        code_bleu(cand, ref, K=K)
    torch.cuda.synchronize()
    t_kernel = [timed(kernel) for _ in range(reps)]                        # (with the two small allocations of the binding)
    t_e2e = []
    for _ in range(reps):
        t0 = time.perf_counter()
        scores = code_bleu(cand, ref, K=K)
        torch.cuda.synchronize()
        t_e2e.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    c_h, r_h = cand.cpu().numpy(), ref.cpu().numpy()
    host = [R.bleu(c, r) for c, r in zip(c_h, r_h)]
    t_host = (time.perf_counter() - t0) * 1e3
    err = max(abs(a - b) for a, b in zip(scores.cpu().tolist(), host))
    return {"bleu_B": B, "bleu_L": L, "K": K, "reps": reps, "kernel_ms_median": statistics.median(t_kernel), "kernel_ms_min": min(t_kernel),
            "code_bleu_ms_median": statistics.median(t_e2e), "host_counter_route_ms": t_host,
            "host_over_code_bleu": t_host / statistics.median(t_e2e), "mean_bleu": sum(host) / B, "max_abs_score_diff": err}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--bleu", action="store_true", help="BLEU over code sequences: kernel, code_bleu and the host Counter route")
    ap.add_argument("--only-new", action="store_true", help="the new kernel alone (for a rocprofv3 --kernel-trace --stats run)")
    ap.add_argument("--shapes", default="400x4096,400x65536,400x1048576,128x4096,128x65536,128x1048576")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: there is nothing to time on a CPU"
    recs = []
    for s in filter(None, a.shapes.split(",")):
        E, N = (int(v) for v in s.split("x"))
        recs.append(bench_shape(N, E, 30 if N >= 2 ** 20 else 100, a.only_new))
        print(json.dumps(recs[-1]), flush=True)
    if a.e2e:
        recs.append(bench_e2e(2 ** 20))
        print(json.dumps(recs[-1]), flush=True)
    if a.bleu:
        for B, L in ((65536, 8), (256, 1024)):
            recs.append(bench_bleu(B, L))
            print(json.dumps(recs[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
