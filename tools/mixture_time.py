"""Time ``MixtureDistribution`` at B = 2^18 rows for (K, d) in {(8, 2), (40, 2), (40, 66), (64, 128)}: (a) the kernel path of
csrc/bgk_mixture.hip (``fused = "always"``), (b) the class's own general path on the same device and the same inputs (``fused = False``:
K component energies, the [B, 1, K] stack and the logsumexp in torch ops -- what a user had before the kernel).  Four workloads:

    energy            no autograd
    energy + grad     the gradient with respect to x
    + weights         the gradients with respect to x and the trainable log-weights
    sample            ``sample(B)``: (a) ``sample_fused=True`` (one launch, i.i.d. rows), (b) the multinomial counts + per-component draws

HIP-event timed, every run warmed up once, then ``--reps`` rounds that alternate (a) and (b); median and min .. max in ms.  Every second
component carries a diagonal covariance.  Also printed: the largest difference of the two paths' energies on the timed inputs,
relative to 1 + |u|, and the model of DESIGN.md's "Gaussian mixture" (bytes and f32 operations per sample).  Prints the tables of that section.

    python tools/mixture_time.py [--reps 5] [--rows 262144]
"""
import argparse
import copy
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bgflow_amd as bg  # noqa: E402
from bgflow_amd import mixture  # noqa: E402
from bgflow_amd.distributions import _kernel_plan  # noqa: E402
from mcmc_time import timed  # noqa: E402

SHAPES = ((8, 2), (40, 2), (40, 66), (64, 128))


def make(K, d, dev, trainable):
    g = torch.Generator().manual_seed(1000 * K + d)
    comps = []
    for k in range(K):
        mean = 3.0 * torch.randn(d, generator=g)
        cov = torch.diag(0.2 + 2.0 * torch.rand(d, generator=g)) if k % 2 else None
        comps.append(bg.NormalDistribution(d, mean, cov))
    return bg.MixtureDistribution(comps, torch.randn(K, generator=g), trainable_weights=trainable).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1 << 18)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mixture_time.py measures on a HIP device"
    dev = torch.device("cuda:0")
    B = args.rows
    print(f"{torch.cuda.get_device_name(0)}; B = {B} rows; median of {args.reps} (min .. max), ms")
    print("| (K, d) | workload | (a) kernel | (b) general | (b) / (a) |")
    print("|---|---|---|---|---|")
    for K, d in SHAPES:
        fused = make(K, d, dev, True)
        fused.fused = "always"
        general = copy.deepcopy(fused)
        general.fused = False
        x = 4.0 * torch.randn(B, d, generator=torch.Generator().manual_seed(7)).to(dev)
        plan = _kernel_plan(fused, 1.0)
        assert plan is not None and mixture._kernel_operands(plan, (x,)) is not None and _kernel_plan(general, 1.0) is None
        with torch.no_grad():
            ua, ub = fused.energy(x), general.energy(x)
        diff = float(((ua - ub).abs() / (1.0 + ub.abs())).max())

        def energy(m):
            with torch.no_grad():
                return m.energy(x)

        def grad(m, weights):
            xg = x.detach().requires_grad_(True)
            return torch.autograd.grad(m.energy(xg).sum(), (xg, m._unnormed_log_weights) if weights else (xg,))

        def sample(m):
            with torch.no_grad():
                return m.sample(B)

        sampler_a, sampler_b = copy.deepcopy(fused), copy.deepcopy(general)
        sampler_a.sample_fused = True
        sampler_a.sample(64)
        assert sampler_a.__dict__.get("_philox_last") is not None, "the fused draw must take the kernel"
        work = (("energy", lambda: energy(fused), lambda: energy(general)),
                ("energy + grad", lambda: grad(fused, False), lambda: grad(general, False)),
                ("+ weights", lambda: grad(fused, True), lambda: grad(general, True)),
                ("sample", lambda: sample(sampler_a), lambda: sample(sampler_b)))
        for label, fa, fb in work:
            t = timed({"a": fa, "b": fb}, args.reps)
            ma, mb = statistics.median(t["a"]), statistics.median(t["b"])
            print(f"| ({K}, {d}) | {label} | {ma:.3f} ({min(t['a']):.3f} .. {max(t['a']):.3f}) | {mb:.3f} ({min(t['b']):.3f} .. {max(t['b']):.3f}) | "
                  f"{mb / ma:.1f} |")
        ops, byts = 3 * K * d + 30 * K, 4 * (d + 1)
        print(f"<!-- ({K}, {d}): max |u_a - u_b| / (1 + |u_b|) = {diff:.2e}; model per sample: {ops} f32 operations (3 K d + ~30 K for the exps), "
              f"{byts} bytes forward -->")


if __name__ == "__main__":
    main()
