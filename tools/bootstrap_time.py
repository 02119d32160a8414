"""Time the bootstrap histograms of ``bgflow_amd.analysis`` on f32 samples with f32 weights, 64 bins: N = 2^20 with 100 and 1000 replicates,
N = 2^24 with 100.  Per setting
(a) ``kernel``: the kernel path (csrc/bgk_hist.hip: digitize once, one resampling launch per batch of replicates, one merge),
(a') ``kernel_uniform``: the same on samples spread evenly over the 64 bins -- the same gathers, far fewer lanes of a wave adding into one
    bin; its distance from (a) is what the same-address LDS adds of the peaked samples cost,
(b) ``torch_ops``: the formulation in torch ops on the same device, per replicate ``randint`` + two gathers + ``bucketize`` + ``scatter_add_``,
(c) ``torch_path``: the package's own torch path on the same device (digitize once, batched ``randint`` / gather / ``index_add_``),
(d) ``numpy``: the reference's routine on this box's host (the package's numpy path makes the reference's numpy calls), timed on
    ``--numpy-replicates`` replicates and reported per replicate.
Host clock around calls that end in a device synchronise, every run warmed up, (a) - (c) alternated, median / min / max of the repetitions.
(b) and (c) add into 64 f64 destinations per replicate with global atomics and take seconds per call: they are timed on
``--baseline-replicates`` replicates and reported per replicate and scaled to the setting's replicate count.
A second pass under torch.profiler gives the kernel path's split over its three kernels and, from the resampling kernel's time, the
gather rate in records per second.  One JSON line per setting (DESIGN.md "Bootstrap histogram").

    python tools/bootstrap_time.py [--reps 5] [--baseline-replicates 4] [--numpy-replicates 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import bgflow_amd as bg  # noqa: E402
from bgflow_amd import analysis  # noqa: E402

L, R, N_EDGES = 0.5, 2.5, 65


def samples(n, dev):
    """the fixture's recipe: two Gaussians at 1.0 and 2.0 (sigma 0.15, 40 % each) + 20 % uniform on [0.5, 2.5]; W = exp(2 g - max)"""
    rng = np.random.default_rng(20264)
    k = rng.integers(0, 5, n)
    D = np.where(k < 2, 1.0 + 0.15 * rng.standard_normal(n), np.where(k < 4, 2.0 + 0.15 * rng.standard_normal(n), rng.uniform(0.5, 2.5, n)))
    logw = 2.0 * rng.standard_normal(n)
    D, W = D.astype(np.float32), np.exp(logw - logw.max()).astype(np.float32)
    return D, W, torch.from_numpy(D).to(dev), torch.from_numpy(W).to(dev)


def torch_ops(D, W, edges_t, sample):
    """per replicate: randint, two gathers, bucketize, scatter_add_ (f64 sums, np.histogram's bins)"""
    n, nb = D.numel(), edges_t.numel() - 1
    out = torch.zeros(sample, nb + 1, dtype=torch.float64, device=D.device)        # column nb: dropped samples
    for s in range(sample):
        idx = torch.randint(n, (n,), device=D.device)
        d, w = D[idx].double(), W[idx].double()
        b = (torch.bucketize(d, edges_t, right=True) - 1).clamp_(0, nb - 1)
        b = torch.where((d >= edges_t[0]) & (d <= edges_t[-1]), b, torch.full_like(b, nb))
        out[s].scatter_add_(0, b, w)
    return out[:, :nb]


def timed(runs, reps):
    for fn, _ in runs.values():
        fn()
    torch.cuda.synchronize()
    out = {k: [] for k in runs}
    for _ in range(reps):
        for k, (fn, inner) in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t0) * 1e3 / inner)
    return out


def kernel_split(fn):
    """{kernel name: ms per call} of one profiled call (device time)"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    split = {}
    for e in prof.key_averages():
        if e.device_type != torch.autograd.DeviceType.CUDA:
            continue
        us = getattr(e, "self_device_time_total", None)
        us = getattr(e, "self_cuda_time_total", 0.0) if us is None else us
        name = next((s for s in ("hist_digitize_kernel", "hist_resample_kernel", "hist_merge_kernel") if s in e.key), e.key[:40])
        split[name] = round(split.get(name, 0.0) + us / 1e3, 4)
    return split


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline-replicates", type=int, default=4)
    ap.add_argument("--numpy-replicates", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    edges = np.linspace(L, R, N_EDGES)
    edges_t = torch.from_numpy(edges).to(dev)
    for n, sample in ((2 ** 20, 100), (2 ** 20, 1000), (2 ** 24, 100)):
        Dn, Wn, D, W = samples(n, dev)
        assert analysis._kernel_eligible([D], [W])
        base = min(sample, args.baseline_replicates)
        U = torch.from_numpy(np.random.default_rng(7).uniform(L, R, n).astype(np.float32)).to(dev)
        runs = {
            "kernel": (lambda: bg.bootstrap_histogram(D, edges, sample, weights=W, seed=1), 10 if n * sample <= 2 ** 28 else 3),
            "kernel_uniform": (lambda: bg.bootstrap_histogram(U, edges, sample, weights=W, seed=1), 10 if n * sample <= 2 ** 28 else 3),
            "torch_ops": (lambda: torch_ops(D, W, edges_t, base), 1),
            "torch_path": (lambda: analysis._hist_torch(D, W, edges, base, 1), 1),
        }
        times = timed(runs, args.reps)
        line = {"device": torch.cuda.get_device_name(0), "n": n, "bins": N_EDGES - 1, "sample": sample, "dtype": "float32", "reps": args.reps,
                "n_chunks": analysis._n_chunks(n, sample)}
        for k, v in times.items():
            line[k] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
            if not k.startswith("kernel"):
                line[k].update(replicates=base, scaled_to_sample_ms=round(statistics.median(v) * sample / base, 1))
        try:
            split = kernel_split(runs["kernel"][0])
            line["kernel_split_ms"] = split
            if split.get("hist_resample_kernel"):
                line["gather_records_per_s"] = round(n * sample / (split["hist_resample_kernel"] * 1e-3), 0)
        except Exception as e:          # no kernel tracer on this box
            line["kernel_split_ms"] = f"torch.profiler unavailable: {e!r}"
        t0 = time.perf_counter()
        np.random.seed(1)
        analysis._free_energy_bootstrap_numpy(Dn, L, R, N_EDGES, args.numpy_replicates, Wn, None, 1.0, None, None)
        line["numpy"] = {"s_per_replicate": round((time.perf_counter() - t0) / args.numpy_replicates, 4), "replicates": args.numpy_replicates}
        # the two device paths agree on what they count (other random numbers: totals only)
        k_sum = float(bg.bootstrap_histogram(D, edges, 4, seed=1).sum(1).mean())
        t_sum = float(analysis._hist_torch(D, None, edges, 4, 1)[0].sum(1).mean())
        line["mean_count_kernel_torch"] = [k_sum, t_sum]
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
