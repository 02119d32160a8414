"""Time one Bennett-acceptance-ratio solve (``bgflow_amd.free_energy``) on f32 work values at 2^20 / 2^19 and at 10^4 / 2 10^4:
(a) the kernel path (csrc/bgk_bar.hip: two launches per evaluation, one read-back per ``BAR_CHUNK`` evaluations), (b) the torch path with
the same stop rule (the same state machine in torch ops, one read-back per evaluation), (c) the torch path forced through all
``maximum_iterations`` = 500 iterations, which is what the reference does for a positive estimate (its stop test never fires,
utils/free_energy.py:149-165).  Host clock around calls that end in a read-back, every run warmed up, alternated, median of the
repetitions; one JSON line per shape with the evaluations and host read-backs of each (DESIGN.md "Bennett acceptance ratio").

    python tools/bar_time.py [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import bgflow_amd as bg  # noqa: E402
from bgflow_amd import free_energy as fe  # noqa: E402


def work_values(nf, nr, dev):
    """u1 = x^2 / 2 on N(0, 1), u2 = (x - 0.5)^2 / 2 + 1.5 on N(0.5, 1): delta_f = 1.5"""
    g = torch.Generator().manual_seed(1)
    x1 = torch.randn(nf, generator=g, dtype=torch.float64)
    x2 = 0.5 + torch.randn(nr, generator=g, dtype=torch.float64)
    wf = (1.5 + 0.5 * (x1 - 0.5) ** 2) - 0.5 * x1 ** 2
    wr = 0.5 * x2 ** 2 - (1.5 + 0.5 * (x2 - 0.5) ** 2)
    return wf.float().to(dev), wr.float().to(dev)


def timed(runs, reps):
    """{name: [ms per solve, ...]}, {name: last result}: every run warmed up once, then ``reps`` rounds that alternate the runs; a
    timed window is ``inner`` solves back to back (a single solve of a few hundred microseconds would measure the clock)"""
    last = {k: fn() for k, (fn, _) in runs.items()}
    torch.cuda.synchronize()
    out = {k: [] for k in runs}
    for _ in range(reps):
        for k, (fn, inner) in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                last[k] = fn()
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t0) * 1e3 / inner)
    return out, last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for nf, nr in ((2 ** 20, 2 ** 19), (10 ** 4, 2 * 10 ** 4)):
        wf, wr = work_values(nf, nr, dev)
        runs = {
            "kernel": (lambda: bg.bar_solve(wf, wr, path="kernel"), 200),
            "torch": (lambda: bg.bar_solve(wf, wr, path="torch"), 20),
            "torch_all_iterations": (lambda: fe._bar_torch(wf, wr, 500, 1e-12, stop=False), 1),
        }
        times, last = timed(runs, args.reps)
        line = {"device": torch.cuda.get_device_name(0), "n_forward": nf, "n_reverse": nr, "dtype": "float32", "reps": args.reps,
                "chunk": fe.BAR_CHUNK}
        for k, r in last.items():
            line[k] = {"median_ms": round(statistics.median(times[k]), 4), "min_ms": round(min(times[k]), 4),
                       "max_ms": round(max(times[k]), 4), "evaluations": r.n_evaluations, "readbacks": r.n_readbacks,
                       "status": fe.STATUS_NAMES[r.status], "delta_f": float(r.delta_f)}
        print(json.dumps(line))


if __name__ == "__main__":
    main()
